#!/usr/bin/env python3
"""Extract the rows and constants of the reference's ReadIndex tests into tests/golden/read_only.json (data only: no test
CODE is copied; tests/test_read_index_host.py replays them against tests/readonly_model.py).

Run where the reference tree exists (as tests/golden/make_golden.py):

    python tests/golden/make_readonly_golden.py

From harness/tests/integration_cases/test_raft.rs:
    test_read_only_option_safe           voters + six rows (id, proposals, wri, ctxs, pending)
    test_read_only_with_learner          voters, learners + four rows (id, proposals, wri, ctx)
    test_read_only_option_lease          voters + six rows (id, proposals, wri, ctx)
    test_read_only_for_new_leader        node_configs rows (id, committed, applied, compact_index), the stored entries, windex, wctx
    test_read_when_quorum_becomes_less   number of peers, the committed index asserted after the election, the context bytes
    test_raft_frees_read_only_mem        voters, the context
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402 -- extract_table: the rows of a `let mut tests = vec![...]`

REL = "harness/tests/integration_cases/test_raft.rs"
DST = os.path.join(HERE, "read_only.json")


def body_of(src, fn):
    a = src.index("fn " + fn + "()")
    lb = src.index("{", a)
    rb = make_golden._matching(src, lb, "{", "}")
    return src[lb:rb + 1], src.count("\n", 0, a) + 1, src.count("\n", 0, rb) + 1


def ints(s):
    return [int(x) for x in re.findall(r"\d+", s)]


def extract():
    src = open(os.path.join("/root/reference", REL), encoding="utf-8").read()
    out = {}

    def table(fn):
        t = make_golden.extract_table(REL, fn, {})
        body, _, _ = body_of(src, fn)
        return t, body

    t, body = table("test_read_only_option_safe")
    m = re.search(r"new_test_raft\(1,\s*vec!\[([\d,\s]*)\]", body)
    out["option_safe"] = {"source": t["source"], "voters": ints(m.group(1)), "rows": t["rows"]}

    t, body = table("test_read_only_with_learner")
    m = re.search(r"new_test_learner_raft\(1,\s*vec!\[([\d,\s]*)\],\s*vec!\[([\d,\s]*)\]", body)
    out["with_learner"] = {"source": t["source"], "voters": ints(m.group(1)), "learners": ints(m.group(2)), "rows": t["rows"]}

    t, body = table("test_read_only_option_lease")
    m = re.search(r"new_test_raft\(1,\s*vec!\[([\d,\s]*)\]", body)
    out["option_lease"] = {"source": t["source"], "voters": ints(m.group(1)), "rows": t["rows"]}

    body, la, lb = body_of(src, "test_read_only_for_new_leader")
    m = re.search(r"let node_configs = vec!\[(.*?)\];", body, flags=re.S)
    rows = [ints(r) for r in re.findall(r"\(([^()]*)\)", m.group(1))]
    voters = ints(re.search(r"new_with_conf_state\(\(vec!\[([\d,\s]*)\]", body).group(1))
    entries = [[int(t_), int(i)] for t_, i in re.findall(r"empty_entry\((\d+),\s*(\d+)\)", re.search(r"let entries = vec!\[(.*?)\];", body, flags=re.S).group(1))]
    out["for_new_leader"] = {"source": f"{REL}:{la}-{lb} test_read_only_for_new_leader", "voters": voters, "node_configs": rows,
                             "entries": entries, "hard_state_term": int(re.search(r"hs\.term = (\d+)", body).group(1)),
                             "windex": int(re.search(r"let windex = (\d+)", body).group(1)),
                             "wctx": re.search(r'let wctx = "(\w+)"', body).group(1)}

    body, la, lb = body_of(src, "test_read_when_quorum_becomes_less")
    peers = re.search(r"Network::new\(vec!\[([^\]]*)\]", body).group(1).count("None")
    out["quorum_becomes_less"] = {"source": f"{REL}:{la}-{lb} test_read_when_quorum_becomes_less", "peers": peers,
                                  "committed_after_election": int(re.search(r"raft_log\.committed,\s*(\d+)\)", body).group(1)),
                                  "removed": int(re.search(r"remove_node\((\d+)\)", body).group(1)),
                                  "ctx": re.search(r'b"(\w+)"', body).group(1)}

    body, la, lb = body_of(src, "test_raft_frees_read_only_mem")
    m = re.search(r"new_test_raft\(1,\s*vec!\[([\d,\s]*)\]", body)
    out["frees_read_only_mem"] = {"source": f"{REL}:{la}-{lb} test_raft_frees_read_only_mem", "voters": ints(m.group(1)),
                                  "ctx": re.search(r'let ctx = "(\w+)"', body).group(1),
                                  "ack_from": int(re.search(r"new_message\((\d+),\s*1,\s*MessageType::MsgHeartbeatResponse", body).group(1))}
    return out


def main():
    out = extract()
    with open(DST, "w", encoding="utf-8") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print({k: len(v.get("rows", [])) for k, v in out.items()}, "->", DST)


if __name__ == "__main__":
    sys.exit(main())
