#!/usr/bin/env python3
"""Extract the rows and constants of the reference's follower-side log tests into tests/golden/follower_log.json (data only: no
test CODE is copied; tests/test_follower_host.py replays them against tests/follower_model.py).

Run where the reference tree exists (as tests/golden/make_golden.py):

    python tests/golden/make_follower_golden.py

From src/raft_log.rs:
    test_log_maybe_append   previous_ents, (last_index, last_term, commit, persist) + the rows
                            (log_term, index, committed, ents, wlasti, wcommit, wpersist, wpanic); new_entry(index, term)
    test_find_conflict      previous_ents + the rows (ents, wconflict)
    test_term               offset, num, the snapshot's term, the range of the loop that appends (offset + i, i) + the rows (index, w)
From harness/tests/integration_cases/test_raft.rs:
    test_handle_msg_append  the initial log (empty_entry(term, index)) + the rows (nm(term, log_term, index, commit, ents as
                            (index, term)), w_index, w_commit, w_reject)
    test_handle_heartbeat   the stored log, commit + the rows (nw(from, to, term, commit), w_commit)
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402 -- _matching

REF = "/root/reference"
DST = os.path.join(HERE, "follower_log.json")


def fn_span(src, fn):
    a = src.index("fn " + fn + "()")
    lb = src.index("{", a)
    rb = make_golden._matching(src, lb, "{", "}")
    return a, rb


def constants(head):
    """`let name = 3u64;` and `let (a, b) = (3u64, 5u64);` in front of the table."""
    env = {}
    for m in re.finditer(r"let\s+(\w+)\s*=\s*(\d+)(?:u64|usize)?\s*;", head):
        env[m.group(1)] = int(m.group(2))
    for m in re.finditer(r"let\s+\(([\w\s,]+)\)\s*=\s*\(([^)]*)\)\s*;", head):
        for k, v in zip([x.strip() for x in m.group(1).split(",")], m.group(2).split(",")):
            env[k] = int(re.match(r"\s*(\d+)", v).group(1))
    return env


def literal(text, env, extra=None):
    """A Rust literal of tuples, vec!s, numbers, the constants of `env` and a few constructors, as plain lists."""
    body = re.sub(r"//[^\n]*", "", text)
    body = re.sub(r"(\d+)(?:u64|usize|u32|i64)", r"\1", body)
    body = body.replace("vec![", "[").replace("&[", "[")
    body = re.sub(r"\b(?:empty_entry|new_entry)\(", "L(", body)
    body = body.replace("cmp::min(", "min(")
    body = re.sub(r"\bSome\(", "S(", body)
    body = re.sub(r"\btrue\b", "True", body)
    body = re.sub(r"\bfalse\b", "False", body)
    body = body.replace("/", "//")
    scope = {"L": lambda *x: list(x), "S": lambda x: x, "None": None, "True": True, "False": False, "min": min, "__builtins__": {}}
    scope.update(env)
    scope.update(extra or {})
    val = eval(body, scope)  # noqa: S307 -- a literal of numbers, the constants and the constructors above

    def plain(x):
        if isinstance(x, (tuple, list)):
            return [plain(y) for y in x]
        return x
    return plain(val)


def table(rel, fn, extra=None):
    src = open(os.path.join(REF, rel), encoding="utf-8").read()
    a, rb_fn = fn_span(src, fn)
    m = re.compile(r"let\s+(?:mut\s+)?tests\s*=\s*vec!\[").search(src, a)
    lb = m.end() - 1
    rb = make_golden._matching(src, lb, "[", "]")
    head = src[a:lb]
    env = constants(head)
    rows = literal(src[lb - 4:rb + 1], env, extra)
    line = lambda p: src.count("\n", 0, p) + 1  # noqa: E731
    return {"source": f"{rel}:{line(a)}-{line(rb_fn)} {fn}", "constants": env, "rows": rows}, src[a:rb_fn + 1], env


def extract():
    out = {}
    log_rs, harness = "src/raft_log.rs", "harness/tests/integration_cases/test_raft.rs"

    for key, fn in (("LOG_MAYBE_APPEND", "test_log_maybe_append"), ("FIND_CONFLICT", "test_find_conflict")):
        t, body, env = table(log_rs, fn)
        t["previous_ents"] = literal(re.search(r"let previous_ents = (vec!\[.*?\]);", body, flags=re.S).group(1), env)
        out[key] = t

    t, body, env = table(log_rs, "test_term")
    t["snapshot"] = [re.search(r"new_snapshot\((\w+),\s*(\d+)\)", body).group(1), int(re.search(r"new_snapshot\((\w+),\s*(\d+)\)", body).group(2))]
    lo, hi = re.search(r"for i in (\d+)\.\.(\w+)", body).groups()
    assert re.search(r"new_entry\(offset \+ i, i\)", body)
    t["appended"] = {"i_from": int(lo), "i_below": hi, "entry": ["offset + i", "i"]}
    out["TERM"] = t

    def nm(term, log_term, index, commit, ents):
        return {"term": term, "log_term": log_term, "index": index, "commit": commit, "entries": ents}
    t, body, env = table(harness, "test_handle_msg_append", {"nm": nm})
    t["log"] = literal(re.search(r"MemStorage::new\(\),\s*(&\[.*?\]),", body, flags=re.S).group(1), env)
    out["HANDLE_MSG_APPEND"] = t

    def nw(frm, to, term, commit):
        return {"from": frm, "to": to, "term": term, "commit": commit}
    t, body, env = table(harness, "test_handle_heartbeat", {"nw": nw})
    t["log"] = literal(re.search(r"\.append\((&\[.*?\])\)", body, flags=re.S).group(1), env)
    out["HANDLE_HEARTBEAT"] = t
    return out


def main():
    out = extract()
    with open(DST, "w", encoding="utf-8") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print({k: len(v["rows"]) for k, v in out.items()}, "->", DST)


if __name__ == "__main__":
    sys.exit(main())
