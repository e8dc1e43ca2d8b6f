#!/usr/bin/env python3
"""Extract the rows and constants of the reference's vote-request tests, as far as they concern the RECIPIENT of the request,
into tests/golden/vote_gate.json (data only: no test CODE is copied; tests/test_follow_gate_host.py replays them against
tests/gate_model.py, tests/test_follow_gate_gpu.py against the engine).

Run where the reference tree exists (as tests/golden/make_follower_golden.py):

    python tests/golden/make_vote_golden.py

From harness/tests/integration_cases/test_raft.rs:
    test_recv_msg_request_vote_for_type   the stored log (empty_entry(term, index)), election / heartbeat ticks, the sender, and the
                                          rows (state, index, log_term, vote_for, w_reject); both terms are max(last_term, log_term).
                                          Rows whose state is Leader are listed by index in "skipped_leader_rows": a leader's group
                                          is not in the follower arena.
    test_advance_commit_index_by_vote_request   voters, learners, the conf-change cases (type names and node ids) and the
                                          use_prevote values its two callers pass
From harness/tests/integration_cases/test_raft_paper.rs:
    test_follower_vote   rows (vote, nvote, wreject); the term of the hard state and of the request
    test_voter           rows (ents, log_term, index, wreject); the request's term and sender
    test_vote_request    rows (ents, wterm): the append that builds the log (term wterm - 1, from index 0), and the number of
                         tick_election calls after which the request must have gone out
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402 -- _matching
from make_follower_golden import REF, constants, literal  # noqa: E402

DST = os.path.join(HERE, "vote_gate.json")
ROLES = {"Follower": 0, "PreCandidate": 1, "Candidate": 2, "Leader": 3}


def table(rel, fn, extra=None):
    src = open(os.path.join(REF, rel), encoding="utf-8").read()
    a = re.search(r"fn " + fn + r"\(", src).start()
    lb_fn = src.index("{", src.index(")", a))
    rb_fn = make_golden._matching(src, lb_fn, "{", "}")
    m = re.compile(r"let\s+(?:mut\s+)?tests\s*=\s*vec!\[").search(src, a)
    body = src[a:rb_fn + 1]
    line = lambda p: src.count("\n", 0, p) + 1  # noqa: E731
    out = {"source": f"{rel}:{line(a)}-{line(rb_fn)} {fn}"}
    if m and m.start() < rb_fn:
        lb = m.end() - 1
        rb = make_golden._matching(src, lb, "[", "]")
        text = re.sub(r"StateRole::(\w+)", lambda r: str(ROLES[r.group(1)]), src[lb - 4:rb + 1])
        out["rows"] = literal(text, dict(constants(src[a:lb]), INVALID_ID=0), extra)
    return out, body


def extract():
    out = {}
    raft, paper = "harness/tests/integration_cases/test_raft.rs", "harness/tests/integration_cases/test_raft_paper.rs"

    t, body = table(raft, "test_recv_msg_request_vote_for_type")
    t["log"] = literal(re.search(r"let ents = (&\[.*?\]);", body, flags=re.S).group(1), {})
    e, h = re.search(r"new_test_raft\(1, vec!\[1\], (\d+), (\d+),", body).groups()
    t["constants"] = {"election_tick": int(e), "heartbeat_tick": int(h), "from": int(re.search(r"new_message\((\d+), 0, msg_type, 0\)", body).group(1))}
    assert re.search(r"let term = cmp::max\(sm\.raft_log\.last_term\(\), log_term\);", body)
    t["term_rule"] = "max(last_term, log_term)"
    t["skipped_leader_rows"] = [k for k, r in enumerate(t["rows"]) if r[0] == ROLES["Leader"]]
    out["RECV_MSG_REQUEST_VOTE"] = t

    t, body = table(paper, "test_follower_vote")
    term, commit = re.search(r"hard_state\((\d+), (\d+), vote\)", body).groups()
    e, h = re.search(r"new_test_raft\(1, vec!\[1, 2, 3\], (\d+), (\d+),", body).groups()
    t["constants"] = {"election_tick": int(e), "heartbeat_tick": int(h), "hard_state_term": int(term), "hard_state_commit": int(commit),
                      "m_term": int(re.search(r"m\.term = (\d+);", body).group(1))}
    out["FOLLOWER_VOTE"] = t

    t, body = table(paper, "test_voter")
    e, h = re.search(r"new_test_config\(1, (\d+), (\d+)\)", body).groups()
    t["constants"] = {"election_tick": int(e), "heartbeat_tick": int(h), "m_term": int(re.search(r"m\.term = (\d+);", body).group(1)),
                      "from": int(re.search(r"new_message\((\d+), 1, MessageType::MsgRequestVote, 0\)", body).group(1))}
    out["VOTER"] = t

    t, body = table(paper, "test_vote_request")
    e, h = re.search(r"new_test_raft\(1, vec!\[1, 2, 3\], (\d+), (\d+),", body).groups()
    assert re.search(r"m\.term = wterm - 1;", body) and re.search(r"for _ in 1\.\.r\.election_timeout\(\) \* 2", body)
    t["constants"] = {"election_tick": int(e), "heartbeat_tick": int(h), "from": int(re.search(r"new_message\((\d+), 1, MessageType::MsgAppend, 0\)", body).group(1)),
                      "m_log_term": int(re.search(r"m\.log_term = (\d+);", body).group(1)), "m_index": int(re.search(r"m\.index = (\d+);", body).group(1))}
    t["append_term"] = "wterm - 1"
    t["ticks"] = "2 * election_tick - 1"
    out["VOTE_REQUEST"] = t

    t, body = table(raft, "test_advance_commit_index_by_vote_request")
    src = open(os.path.join(REF, raft), encoding="utf-8").read()
    voters, learners = re.search(r"vec!\[([\d, ]+)\],\s*vec!\[([\d, ]+)\],\s*&l,\s*use_prevote", body).groups()
    t["voters"] = [int(x) for x in voters.split(",")]
    t["learners"] = [int(x) for x in learners.split(",")]
    cases = re.search(r"let mut cases: Vec<Box<dyn ConfChangeI>> = vec!\[(.*?)\n    \];", body, flags=re.S).group(1)
    pair = re.compile(r"ConfChangeType::(\w+),\s*(\d+)\)|\((\d+),\s*ConfChangeType::(\w+)\)")  # conf_change(type, id) / new_conf_change_single(id, type)
    t["cases"] = [[[ty1 or ty2, int(id1 or id2)] for ty1, id1, id2, ty2 in pair.findall(c)] for c in re.split(r"Box::new\(", cases)[1:]]
    t["use_prevote"] = sorted({"false": False, "true": True}[x] for x in re.findall(r"test_advance_commit_index_by_vote_request\((true|false)\)", src))
    t["candidate"], t["recipient"] = 2, 4
    assert re.search(r"let p2 = nt\.peers\.get_mut\(&2\)", body) and re.search(r"let p4 = nt\.peers\.get_mut\(&4\)", body)
    out["ADVANCE_COMMIT_BY_VOTE"] = t
    return out


def main():
    out = extract()
    with open(DST, "w", encoding="utf-8") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print({k: len(v.get("rows", v.get("cases"))) for k, v in out.items()}, "->", DST)


if __name__ == "__main__":
    sys.exit(main())
