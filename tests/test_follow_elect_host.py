"""CPU only: the candidate half -- campaign, vote responses and poll. (1) tests/elect_model.py is pinned with the rows of the
reference's election tests, committed as data (tests/golden/elect.json from tests/golden/make_elect_golden.py), and with a
restatement of test_advance_commit_index_by_vote_response; (2) the arithmetic of csrc/rg_elect.h -- what the election kernels
run -- is compiled for the HOST with g++ (tests/host_check/elect_twin.cpp, a stand-alone program) and diffed against the model
over seeded random streams, (3) once more under AddressSanitizer + UBSan; (4) what the streams contain is asserted from the model
alone; (5) the refusals; (6) the new kernels use no scratch; (7) every new name is declared, exported and bound.

Citations: pingcap/raft-rs v0.6.0."""
import ctypes
import json
import os
import random
import re
import shutil
import subprocess
from concurrent.futures import ProcessPoolExecutor

import pytest

import elect_model as M
import follower_model as F
import gate_model as G

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = json.load(open(os.path.join(HERE, "golden", "elect.json")))
NEW_NAMES = ("rg_follow_elect_enable", "rg_follow_elect_write", "rg_follow_elect_read", "rg_follow_campaign_device", "rg_follow_campaign",
             "rg_follow_vote_resps", "rg_follow_vote_resps_device")
NEW_KERNELS = ("k_elect_campaign", "k_elect_list", "k_elect_dense")


def cluster_node(cfg, size, self_id=1, group=0, log=None):
    """Node `self_id` of a cluster of ids 1..=size (id i sits in slot i - 1), promotable, as new_test_raft leaves it."""
    n = M.Node(cfg, group, log, self_id=self_id, incoming=range(size), self_slot=self_id - 1)
    n.promotable = True
    return n


def replay_round(n, votes):
    """MsgHup, then the responses {id: granted} at the node's own term -> the answers"""
    out = [n.record(M.Rec(M.HUP))]
    for peer, granted in votes:
        out.append(n.record(M.Rec(M.VOTE, term=n.term, frm=peer - 1, reject=not granted)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1. the model, pinned by the reference's rows
# ---------------------------------------------------------------------------------------------------------------------
def test_model_leader_election_in_one_round_rpc_rows():
    """test_raft_paper.rs test_leader_election_in_one_round_rpc: rows (size, votes, state); a Leader row is result WON with
    leader_id == self_id (the arena's form of a group handed to the leader engine)."""
    t = GOLD["LEADER_ELECTION_IN_ONE_ROUND_RPC"]
    assert len(t["rows"]) == 13 and t["w_term"] == 1
    for k, (size, votes, state) in enumerate(t["rows"]):
        n = cluster_node(G.Config(t["constants"]["election_tick"]), size, t["constants"]["id"])
        answers = replay_round(n, votes)
        assert n.term == t["w_term"] and answers[-1][2] == t["w_term"], (k, n.term)
        if state == 3:
            assert n.lead == n.self_id and n.role == G.FOLLOWER and n.cells()[2:] == (0, 0), (k, answers)
            res = [a[0] for a in answers]  # one win; the grants that straggle in behind it are ignored
            assert res.count(M.WON) == 1 and set(res[res.index(M.WON) + 1:]) <= {M.IGNORED}, (k, answers)
        else:
            res = [a[0] for a in answers]  # a loss ends the election: the denials that straggle in behind it are ignored
            assert n.role == state and n.lead == 0 and M.WON not in res, (k, answers)
            assert (res.count(M.LOST) == 1 and set(res[res.index(M.LOST) + 1:]) <= {M.IGNORED}) if state == G.FOLLOWER else M.LOST not in res, (k, answers)
        if size > 1:
            assert answers[0][0] == M.REQUESTS and answers[0][3] == M.VOTE and answers[0][4] == (1 << size) - 2 and answers[0][6] == 1, (k, answers[0])


def test_model_nonleader_start_election():
    """test_raft_paper.rs test_nonleader_start_election: a follower (of node 2, term 1) and a candidate (term 1) both time out
    within 2 * election_tick - 1 ticks and start an election at term 2 with requests to the two others."""
    t = GOLD["NONLEADER_START_ELECTION"]
    assert t["peers"] == [1, 2, 3] and t["targets"] == [2, 3] and t["ticks"] == "2 * election_tick - 1" and t["roles"] == [0, 2]
    for role in t["roles"]:
        for seed in range(20):
            n = cluster_node(G.Config(t["election_tick"], seed=seed), len(t["peers"]), t["id"])
            n._events = 0
            if role == G.FOLLOWER:
                n.become_follower(t["follower_term"], t["follower_lead"])
            else:
                n.become_candidate()
            answers = [n.record(M.Rec(M.HUP)) for _ in range(2 * t["election_tick"] - 1) if n.tick()]
            assert len(answers) == 1, (role, seed)
            a = dict(zip(M.ANSWER_FIELDS, answers[0]))
            assert (n.term, n.role, a["term"]) == (t["w_term"], t["w_role"], t["w_term"])
            assert n.votes == {t["id"] - 1: True} and n.vote == t["id"]
            assert (a["result"], a["req_kind"], a["req_term"]) == (M.REQUESTS, M.VOTE, t["request_term"])
            assert a["targets"] == sum(1 << (p - 1) for p in t["targets"]) and a["events"] & G.EV_HARD_STATE


def test_model_candidate_fallback_and_single_node():
    """test_raft_paper.rs test_candidate_fallback: a candidate that gets a MsgAppend at its own term or a later one is a
    follower at that term (through the gate of gate_model, which this model extends). test_raft.rs test_single_node_candidate /
    test_sinle_node_pre_candidate: one node wins on its MsgHup, with and without pre-vote."""
    t = GOLD["CANDIDATE_FALLBACK"]
    assert len(t["messages"]) == 2
    for frm, term in t["messages"]:
        n = cluster_node(G.Config(t["election_tick"]), len(t["peers"]))
        assert n.record(M.Rec(M.HUP))[0] == M.REQUESTS and n.role == G.CANDIDATE and n.votes
        gate, ev, resp_term, resp = n.step(G.Msg(G.APPEND, term, frm))
        assert (n.role, n.term, n.lead) == (t["w_role"], term, frm) and ev & G.EV_BECAME_FOLLOWER and n.cells()[2:] == (0, 0)
    for key in ("SINGLE_NODE_CANDIDATE", "SINGLE_NODE_PRE_CANDIDATE"):
        t = GOLD[key]
        assert t["peers"] == [1] and t["w_role"] == 3
        n = cluster_node(G.Config(10, flags=G.PRE_VOTE if t["pre_vote"] else 0), 1)
        a = n.record(M.Rec(M.HUP))
        assert a[0] == M.WON and a[2] == 1 and n.lead == n.self_id and n.vote == n.self_id and a[1] == G.EV_HARD_STATE | G.EV_LEADER_CHANGED


@pytest.mark.parametrize("use_prevote", [False, True])
def test_model_advance_commit_index_by_vote_response(use_prevote):
    """test_raft.rs test_advance_commit_index_by_vote_response, node 2's side, restated by hand (the conf change's bytes stay on
    the host: only its index matters). Node 2 holds entries 1..2 of term 1 and knows commit 1; cc_index = 2.
    (a) The reference's case: voters 1..4, node 1 isolated; node 3 grants, node 4 -- its log is longer -- rejects with its commit
        info. The election stays open, the commit advances and RG_GATE_EV_CONF_CHECK tells the host to count the conf entries
        (the reference then steps down). (b) With voters 1..3 and node 1's reject already in, the same reject makes the
        candidate LOSE -- and it still advances its commit, without the conf check."""
    cfg = G.Config(10, flags=G.PRE_VOTE if use_prevote else 0)
    kind = M.PREVOTE if use_prevote else M.VOTE
    cc_index = 2
    for size, first in ((4, (3, False)), (3, (1, True))):
        n = cluster_node(cfg, size, self_id=2, log=F.Log(0, 0, [1, 1], 1))
        n.load(1, 0, 0, 0, G.FOLLOWER, 0, 0, True)
        a = dict(zip(M.ANSWER_FIELDS, n.record(M.Rec(M.HUP))))
        assert n.role == (G.PRE_CANDIDATE if use_prevote else G.CANDIDATE)
        assert (a["result"], a["req_kind"], a["req_term"], a["req_index"], a["req_log_term"], a["req_commit"], a["req_commit_term"]) == (M.REQUESTS, kind, 2, 2, 1, 1, 1)
        term = n.term if not use_prevote else n.term + 1
        peer, reject = first
        assert n.record(M.Rec(kind, term=term if not reject else n.term, frm=peer - 1, reject=reject))[0] == M.PENDING
        a = dict(zip(M.ANSWER_FIELDS, n.record(M.Rec(kind, term=n.term, frm=4 - 1 if size == 4 else 3 - 1, reject=True, commit=cc_index, commit_term=1))))
        assert n.log.committed >= cc_index and a["events"] & G.EV_HARD_STATE
        if size == 4:
            assert a["result"] == M.PENDING and a["events"] & G.EV_CONF_CHECK and n.role != G.FOLLOWER
        else:
            assert a["result"] == M.LOST and not a["events"] & G.EV_CONF_CHECK and a["events"] & G.EV_BECAME_FOLLOWER and n.role == G.FOLLOWER


# ---------------------------------------------------------------------------------------------------------------------
# 2.-4. the host twin of csrc/rg_elect.h against the model
# ---------------------------------------------------------------------------------------------------------------------
N_FOLLOW = 300
GROUPS = [0, 1, 7, 100, 254, 255, 256, 257, 298, 299] + list(range(20, 50))
# 12 x 20 000 = 240 000 operations: every combination of the two flags, a wide and a narrow timeout range
CONFIGS = [(s, G.Config(et, lo, hi, flags, seed=0x9E3779B9 * s)) for s, (et, lo, hi, flags) in enumerate(
    [(10, 0, 0, f) for f in range(4)] + [(3, 0, 0, f) for f in range(4)] + [(5, 5, 6, 3), (7, 9, 30, 1), (1, 0, 0, 2), (10, 0, 0, 0)], start=1)]
OPS_PER_SEED = 20000


def build_twin(tmp_path, name, extra):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build the host twin")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, os.path.join(HERE, "host_check", "elect_twin.cpp"), "-o", exe])
    return exe


def state_text(c):
    return "%d %d %d %d %d%s" % (c["committed"], c["last_index"], c["dummy_index"], c["dummy_term"], len(c["runs"]),
                                 "".join(" %d %d" % r for r in c["runs"]))


def soft_text(s):
    return "%d %d %d %d %d %d %d %d" % tuple(s)


def rec_text(g, m):
    if m.kind in (M.HUP, M.TIMEOUT_NOW):
        return "C %d %d %d %d" % (g, (1 if m.kind == M.TIMEOUT_NOW else 0) | (2 if m.blocked else 0), m.term, m.frm)
    return "M %d %d %d %d %d %d %d" % (g, m.kind, m.term, m.frm, m.reject, m.commit, m.commit_term)


def answer_text(a):
    return "R " + " ".join("%d" % x for x in a)


def twin_io(cfg, events, seed):
    """(stdin of the twin, the stdout the model expects)."""
    rng = random.Random(seed)
    lines, expect = ["N %d %d %d %d %d %d" % (N_FOLLOW, cfg.election_tick, cfg.min_timeout, cfg.max_timeout, cfg.flags, cfg.seed)], []

    def rec(ev):
        _, g, m, a, c, s, e = ev
        lines.extend([rec_text(g, m), "S %d" % g, "Q %d" % g, "V %d" % g])
        expect.extend([answer_text(a), "S " + state_text(c), "Q " + soft_text(s), "V %d %d %d %d" % e])
    for ev in events:
        if ev[0] == "W":
            lines.append("W %d %s" % (ev[1], state_text(ev[2])))
            expect.append("W 0")
        elif ev[0] == "G":
            lines.extend(["G %d %s" % (ev[1], soft_text(ev[2])), "Q %d" % ev[1]])
            expect.extend(["G 0", "Q " + soft_text(ev[3])])
        elif ev[0] == "E":
            lines.extend(["E %d %d %d %d %d" % ((ev[1],) + ev[2]), "V %d" % ev[1]])
            expect.extend(["E 0", "V %d %d %d %d" % ev[3]])
        elif ev[0] == "K":
            lines.append("K %d" % N_FOLLOW)
            expect.append("K %d%s" % (len(ev[1]), "".join(" %d" % g for g in ev[1])))
            for g in ev[1] + rng.sample(GROUPS, 4):
                lines.append("Q %d" % g)
                expect.append("Q " + soft_text(ev[2][g]))
            for r in ev[4]:
                rec(r)
        else:
            rec(ev)
    return "\n".join(lines) + "\n", expect


def run_stream(args):
    exe, (seed, cfg), n_ops = args
    events, cov = M.make_stream(seed, cfg, GROUPS, n_ops)
    text, expect = twin_io(cfg, events, seed)
    out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, (seed, out.returncode, out.stderr[-2000:])
    got = out.stdout.split("\n")[:-1]
    assert len(got) == len(expect), (seed, len(got), len(expect))
    for k, (a, b) in enumerate(zip(got, expect)):
        assert a == b, (seed, k, text.split("\n")[k + 1], a, b)
    return n_ops, cov


def _cov_of(args):
    return M.make_stream(args[0], args[1], GROUPS, 4000)[1]


def test_stream_coverage_from_the_model_alone():
    """Every stream the twin and the GPU tests use contains: every result value and every events bit; both response kinds at
    m.term <, =, > term in each of the three roles; majority and joint configurations, a singleton, a self slot that is not a
    voter; a repeated vote of one slot with the opposite answer; MsgTimeoutNow in each role with promotable both ways, and a
    granted transfer campaign; blocked campaigns; the hup of a group this store leads; clock ticks with their hups. And as a
    condition on the generator: at most 10 % of the records of any stream answer RG_FOLLOW_HOST."""
    with ProcessPoolExecutor(max_workers=4) as ex:
        covs = list(ex.map(_cov_of, CONFIGS))
    for (seed, cfg), cov in zip(CONFIGS, covs):
        M.check_coverage(cov, cfg)
    assert {cfg.flags for _, cfg in CONFIGS} == {0, 1, 2, 3}
    for plan in (M.GPU_PLAN, M.GPU_PLAN_NO_PREVOTE):  # ... and the streams the GPU file runs
        M.check_coverage(M.plan_rounds(*plan)[1], plan[2])


def test_host_twin_matches_the_model(tmp_path):
    """>= 200 000 operations under all four flag combinations: every answer field, canonical log, soft state and election cells."""
    exe = build_twin(tmp_path, "elect_twin", [])
    with ProcessPoolExecutor(max_workers=4) as ex:
        res = list(ex.map(run_stream, [(exe, sc, OPS_PER_SEED) for sc in CONFIGS]))
    assert sum(n for n, _ in res) >= 200000
    for (seed, cfg), (_, cov) in zip(CONFIGS, res):
        M.check_coverage(cov, cfg)


def test_host_twin_is_clean_under_asan_and_ubsan(tmp_path):
    """The same program, -fsanitize=address,undefined -fno-sanitize-recover=all, run directly (a stand-alone executable)."""
    exe = build_twin(tmp_path, "elect_twin_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    for sc in (CONFIGS[3], CONFIGS[4]):
        n, cov = run_stream((exe, sc, 5000))
        assert n == 5000
        M.check_coverage(cov, sc[1])


# ---------------------------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_host_twin_refusals(tmp_path):
    """Election cells with self_id 0, a slot both yes and no, or conf bits above bit 18 are refused and nothing is written; a
    campaign record with unknown flags or a MsgTimeoutNow with a term or a from of 0, and a response record with a slot above 7, a
    kind that is not exactly one of the two or a term of 0, are refused and nothing is applied."""
    exe = build_twin(tmp_path, "elect_twin", [])
    conf = M.conf_word((0, 1, 2), (), 1)
    lines = ["N 4 10 10 20 0 1", "G 1 3 102 0 0 2 0 12 1", "E 1 102 %d 2 4" % conf, "V 1"]
    for bad in ("0 %d 2 4" % conf, "102 %d 6 4" % conf, "102 %d 2 4" % (conf | 1 << 19)):
        lines += ["E 1 " + bad, "V 1"]
    lines += ["C 1 4 0 0", "C 1 1 0 5", "C 1 1 3 0", "C 1 3 0 5", "M 1 4 3 8 0 0 0", "M 1 12 3 0 0 0 0", "M 1 0 3 0 0 0 0", "M 1 16 3 0 0 0 0", "M 1 4 0 0 0 0 0",
              "Q 1", "V 1"]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")[:-1]
    assert out[:3] == ["G 0", "E 0", "V 102 %d 2 4" % conf]
    for k, rule in enumerate((1, 2, 3)):  # (rg_follow_elect_check's numbering)
        assert out[3 + 2 * k] == "E %d" % rule and out[4 + 2 * k] == out[2], (k, out[3 + 2 * k])
    assert out[9:18] == ["R malformed"] * 9 and out[18] == "Q 3 102 0 0 2 0 12 1" and out[19] == out[2]


def test_api_refusals_are_host_checks():
    """What rg_follow_elect_write / rg_follow_campaign / rg_follow_vote_resps refuse is decided on the host, before anything is
    staged: the group bound, the duplicate-group rule and the shared well-formedness checks stand in front of RG_ENTER."""
    src = open(os.path.join(ROOT, "raft_rs_amd", "csrc", "abi_elect.hip")).read()
    for fn, needles in (("rg_follow_elect_write", ("rg_follow_elect_check", "seen.emplace", "group >= fo->cols.n")),
                        ("rg_follow_campaign", ("rg_elect_campaign_well_formed", "seen.emplace", "group >= fo->cols.n")),
                        ("rg_follow_vote_resps", ("rg_elect_resp_well_formed", "group >= fo->cols.n"))):
        body = src[src.index('extern "C" int %s(' % fn):]
        body = body[:body.index("} RG_ABI_GUARD")]
        enter = body.index("RG_ENTER(h)")
        for needle in needles:
            assert 0 <= body.find(needle) < enter, (fn, needle)


# ---------------------------------------------------------------------------------------------------------------------
# 6. resources, 7. the boundary
# ---------------------------------------------------------------------------------------------------------------------
def test_elect_kernels_use_no_scratch():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc is needed (the engine is built with it)")
    cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-c", os.path.join(ROOT, "raft_rs_amd", "csrc", "abi_elect.hip"),
           "-o", os.devnull, "-Wno-pass-failed", "-Rpass-analysis=kernel-resource-usage"]
    err = subprocess.run(cmd, stderr=subprocess.PIPE, stdout=subprocess.PIPE, text=True).stderr
    rows, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
        if not m:
            continue
        txt = m.group(1).strip()
        if txt.startswith("Function Name:"):
            cur = rows.setdefault(txt.split(":", 1)[1].strip(), {})
        elif cur is not None and ":" in txt:
            k, v = txt.split(":", 1)
            cur[k.strip()] = v.strip()
    for name in NEW_KERNELS + ("k_elect_write", "k_elect_read"):
        row = [v for k, v in rows.items() if name in k]
        assert len(row) == 1, (name, sorted(rows), err[-2000:])
        print(name, row[0])
        assert int(row[0]["ScratchSize [bytes/lane]"]) == 0, (name, row[0])
        # no LDS of their own; the dense kernel's __syncthreads_or keeps one word per wave of the largest block (64 x 4 bytes)
        assert int(row[0]["LDS Size [bytes/block]"]) <= (256 if name == "k_elect_dense" else 0), (name, row[0])
    for bad in ("k_follow_gate_dense", "k_follow_gate_list", "k_follow_clock"):
        assert not [k for k in rows if bad in k], bad


def test_every_new_name_is_declared_exported_and_bound(rg):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_bindings
    from raft_rs_amd import engine as E
    declared = {name for name, _, _ in gen_rust_bindings.parse(open(os.path.join(ROOT, "include", "raftgroups.h"), encoding="utf-8").read())[3]}
    lib = ctypes.CDLL(rg.LIB_PATH)
    for name in NEW_NAMES:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in E.SYMBOLS, name
    hdr = open(os.path.join(ROOT, "include", "raftgroups.h")).read()
    for k, v in (("RG_ELECT_NONE", E.ELECT_NONE), ("RG_ELECT_IGNORED", E.ELECT_IGNORED), ("RG_ELECT_BLOCKED", E.ELECT_BLOCKED), ("RG_ELECT_REQUESTS", E.ELECT_REQUESTS),
                 ("RG_ELECT_PENDING", E.ELECT_PENDING), ("RG_ELECT_LOST", E.ELECT_LOST), ("RG_ELECT_WON", E.ELECT_WON), ("RG_ELECT_STEPPED_DOWN", E.ELECT_STEPPED_DOWN),
                 ("RG_ELECT_REQ_TRANSFER", E.ELECT_REQ_TRANSFER), ("RG_CAMPAIGN_TIMEOUT_NOW", E.CAMPAIGN_TIMEOUT_NOW), ("RG_CAMPAIGN_BLOCKED", E.CAMPAIGN_BLOCKED)):
        assert int(re.search(r"#define %s (0x[0-9a-f]+|\d+)u" % k, hdr).group(1), 0) == v, k
    assert (M.NONE, M.IGNORED, M.BLOCKED, M.REQUESTS, M.PENDING, M.LOST, M.WON, M.STEPPED_DOWN) == tuple(range(8))
    assert E.elect_conf_make(0x07, 0x19, 2) == M.conf_word((0, 1, 2), (0, 3, 4), 2)
    assert [f for f, _ in E.FollowElectOut._fields_] == list(E.ELECT_OUT_COLUMNS) and [f for f, _ in E.FollowVoteCols._fields_] == list(E.VOTE_COLUMNS)
