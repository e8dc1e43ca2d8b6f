#!/usr/bin/env python3
"""Extract the rows and constants of the reference's election tests, as far as they concern the CANDIDATE, into
tests/golden/elect.json (data only: no test CODE is copied; tests/test_follow_elect_host.py replays them against
tests/elect_model.py, tests/test_follow_elect_gpu.py against the engine).

Run where the reference tree exists (as tests/golden/make_vote_golden.py):

    python tests/golden/make_elect_golden.py

From harness/tests/integration_cases/test_raft_paper.rs:
    test_leader_election_in_one_round_rpc   the rows (size, votes, state): a cluster of ids 1..=size, node 1 campaigns, `votes`
                                            are the responses {id: granted} it then gets at its own term; the expected role and term
    test_nonleader_start_election           the election timeout, the peers, the number of ticks, the expected term and the two
                                            request targets
    test_candidate_fallback                 the peers and the terms of the two MsgAppend a candidate falls back on
From harness/tests/integration_cases/test_raft.rs:
    test_single_node_candidate / test_sinle_node_pre_candidate   one node, a MsgHup, the expected role; pre_vote off / on
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402 -- _matching
from make_follower_golden import REF  # noqa: E402

DST = os.path.join(HERE, "elect.json")
ROLES = {"Follower": 0, "PreCandidate": 1, "Candidate": 2, "Leader": 3}
PAPER, RAFT = "harness/tests/integration_cases/test_raft_paper.rs", "harness/tests/integration_cases/test_raft.rs"


def body_of(rel, fn):
    src = open(os.path.join(REF, rel), encoding="utf-8").read()
    a = re.search(r"fn " + fn + r"\(", src).start()
    lb = src.index("{", src.index(")", a))
    rb = make_golden._matching(src, lb, "{", "}")
    line = lambda p: src.count("\n", 0, p) + 1  # noqa: E731
    return f"{rel}:{line(a)}-{line(rb)} {fn}", src[a:rb + 1]


def ids(text):
    return [int(x) for x in text.split(",") if x.strip()]


def extract():
    out = {}
    source, body = body_of(PAPER, "test_leader_election_in_one_round_rpc")
    m = re.search(r"let mut tests = vec!\[", body)
    lb = m.end() - 1
    table = re.sub(r"//[^\n]*", "", body[lb + 1:make_golden._matching(body, lb, "[", "]")])
    rows = []
    for size, votes, state in re.findall(r"\(\s*(\d+),\s*map!\(([^)]*)\),\s*StateRole::(\w+),?\s*\)", table):
        rows.append([int(size), [[int(i), v == "true"] for i, v in re.findall(r"(\d+)\s*=>\s*(true|false)", votes)], ROLES[state]])
    et, hb = re.search(r"new_test_raft\(1, \(1\.\.=size as u64\)\.collect\(\), (\d+), (\d+),", body).groups()
    assert re.search(r"m\.term = r\.term;", body) and re.search(r"m\.reject = !vote;", body)
    out["LEADER_ELECTION_IN_ONE_ROUND_RPC"] = {"source": source, "rows": rows, "w_term": int(re.search(r"if r\.term != (\d+)", body).group(1)),
                                               "constants": {"election_tick": int(et), "heartbeat_tick": int(hb), "id": 1}}

    source, body = body_of(PAPER, "test_nonleader_start_election")
    peers, hb = re.search(r"new_test_raft\(1, vec!\[([\d, ]+)\], et, (\d+),", body).groups()
    lead_term, lead = re.search(r"r\.become_follower\((\d+), (\d+)\)", body).groups()
    assert re.search(r"for _ in 1\.\.2 \* et", body)
    out["NONLEADER_START_ELECTION"] = {
        "source": source, "election_tick": int(re.search(r"let et = (\d+);", body).group(1)), "heartbeat_tick": int(hb), "id": 1, "peers": ids(peers),
        "follower_term": int(lead_term), "follower_lead": int(lead), "ticks": "2 * election_tick - 1",
        "w_term": int(re.search(r"assert_eq!\(r\.term, (\d+)\);", body).group(1)), "w_role": ROLES[re.search(r"assert_eq!\(r\.state, StateRole::(\w+)\);", body).group(1)],
        "request_term": int(re.search(r"m\.term = (\d+);", body).group(1)),
        "targets": [int(x) for x in re.findall(r"new_message_ext\(1, (\d+)\)", body)], "roles": [ROLES["Follower"], ROLES["Candidate"]]}

    source, body = body_of(PAPER, "test_candidate_fallback")
    peers, et, hb = re.search(r"new_test_raft\(1, vec!\[([\d, ]+)\], (\d+), (\d+),", body).groups()
    out["CANDIDATE_FALLBACK"] = {"source": source, "peers": ids(peers), "election_tick": int(et), "heartbeat_tick": int(hb),
                                 "messages": [[int(f), int(t)] for f, t in re.findall(r"new_message_ext\((\d+), 1, (\d+)\)", body)],
                                 "w_role": ROLES["Follower"]}

    for key, fn, pre in (("SINGLE_NODE_CANDIDATE", "test_single_node_candidate", False), ("SINGLE_NODE_PRE_CANDIDATE", "test_sinle_node_pre_candidate", True)):
        source, body = body_of(RAFT, fn)
        assert bool(re.search(r"config\.pre_vote = true;", body)) == pre and re.search(r"vec!\[None\]", body)
        out[key] = {"source": source, "peers": [1], "pre_vote": pre, "w_role": ROLES[re.search(r"\.state, StateRole::(\w+)\)", body).group(1)]}
    return out


def main():
    out = extract()
    assert len(out["LEADER_ELECTION_IN_ONE_ROUND_RPC"]["rows"]) == 13
    with open(DST, "w", encoding="utf-8") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print({k: len(v.get("rows", v.get("messages", v["peers"] if "peers" in v else []))) for k, v in out.items()}, "->", DST)


if __name__ == "__main__":
    sys.exit(main())
