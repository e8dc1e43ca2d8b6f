"""CPU only: the follower's term gate, vote step and election clock. (1) tests/gate_model.py is pinned with the rows of the
reference's vote-request tests, committed as data (tests/golden/vote_gate.json from tests/golden/make_vote_golden.py); (2) the
gate arithmetic of csrc/rg_follow.h -- what the gated kernels run -- is compiled for the HOST with g++
(tests/host_check/gate_twin.cpp, a stand-alone program) and diffed against the model over seeded random streams, (3) once more
under AddressSanitizer + UBSan; (4) what the streams contain is asserted from the model alone; (5) the three new kernels use no
scratch.

Citations: pingcap/raft-rs v0.6.0."""
import json
import os
import random
import re
import shutil
import subprocess
from concurrent.futures import ProcessPoolExecutor

import pytest

import follower_model as F
import gate_model as G

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = json.load(open(os.path.join(HERE, "golden", "vote_gate.json")))


def log_of(term_index_pairs, committed=0):
    """A log from [(term, index)] (empty_entry(term, index)) with consecutive indices from 1."""
    assert [i for _, i in term_index_pairs] == list(range(1, len(term_index_pairs) + 1))
    return F.Log(0, 0, [t for t, _ in term_index_pairs], committed)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the model, pinned by the reference's rows
# ---------------------------------------------------------------------------------------------------------------------
def test_model_recv_msg_request_vote_rows():
    """test_raft.rs test_recv_msg_request_vote_for_type (MsgRequestVote): rows (state, index, log_term, vote_for, w_reject) on the
    log [(2, 1), (2, 2)]; both terms are max(last_term, log_term). The one Leader row is not a follower's."""
    t = GOLD["RECV_MSG_REQUEST_VOTE"]
    c = t["constants"]
    assert len(t["rows"]) == 21 and t["skipped_leader_rows"] == [18] and t["term_rule"] == "max(last_term, log_term)"
    ran = 0
    for k, (state, index, log_term, vote_for, w_reject) in enumerate(t["rows"]):
        if k in t["skipped_leader_rows"]:
            assert state == 3
            continue
        n = G.Node(G.Config(c["election_tick"]), 0, log_of(t["log"]))
        term = max(t["log"][-1][0], log_term)
        n.load(term, vote_for, 0, 0, state, 0, 0, True)
        gate, ev, resp_term, resp = n.step(G.Msg(G.VOTE, term, c["from"], index=index, log_term=log_term))
        assert gate in (G.G_VOTE_GRANT, G.G_VOTE_REJECT) and (gate == G.G_VOTE_REJECT) == w_reject, (k, gate)
        assert resp_term == term, k
        ran += 1
    assert ran == 20


def test_model_follower_vote_rows():
    """test_raft_paper.rs test_follower_vote: rows (vote, nvote, wreject): a follower votes for at most one candidate per term."""
    t = GOLD["FOLLOWER_VOTE"]
    c = t["constants"]
    assert len(t["rows"]) == 6
    for k, (vote, nvote, wreject) in enumerate(t["rows"]):
        n = G.Node(G.Config(c["election_tick"]), 0)
        n.load(c["hard_state_term"], vote, 0, 0, G.FOLLOWER, 0, 0, True)
        gate, ev, resp_term, resp = n.step(G.Msg(G.VOTE, c["m_term"], nvote))
        assert (gate, resp_term) == (G.G_VOTE_REJECT if wreject else G.G_VOTE_GRANT, c["m_term"]), k
        assert n.vote == (vote if wreject else nvote), k
        assert bool(ev & G.EV_HARD_STATE) == (not wreject and vote != nvote), k


def test_model_voter_rows():
    """test_raft_paper.rs test_voter: rows (ents, log_term, index, wreject): the voter denies a candidate whose log is behind."""
    t = GOLD["VOTER"]
    c = t["constants"]
    assert len(t["rows"]) == 9
    for k, (ents, log_term, index, wreject) in enumerate(t["rows"]):
        n = G.Node(G.Config(c["election_tick"]), 0, log_of(ents))
        gate, ev, resp_term, resp = n.step(G.Msg(G.VOTE, c["m_term"], c["from"], index=index, log_term=log_term))
        assert gate == (G.G_VOTE_REJECT if wreject else G.G_VOTE_GRANT), k
        assert n.term == c["m_term"] and resp_term == c["m_term"] and ev & G.EV_HARD_STATE, k
        assert n.vote == (0 if wreject else c["from"]), k


def test_model_vote_request_rows():
    """test_raft_paper.rs test_vote_request, the recipient's side: rows (ents, wterm). The append of term wterm - 1 builds the
    log; within 2 * election_tick - 1 ticks the group is due exactly once, and the request its hup() sends carries the log's
    last entry and the term wterm."""
    t = GOLD["VOTE_REQUEST"]
    c = t["constants"]
    assert len(t["rows"]) == 2 and t["append_term"] == "wterm - 1" and t["ticks"] == "2 * election_tick - 1"
    for k, (ents, wterm) in enumerate(t["rows"]):
        for seed in range(20):
            n = G.Node(G.Config(c["election_tick"], seed=seed), k)
            n.promotable = True
            assert [i for _, i in ents] == list(range(1, len(ents) + 1))
            gate, ev, resp_term, resp = n.step(G.Msg(G.APPEND, wterm - 1, c["from"], index=c["m_index"], log_term=c["m_log_term"], ents=[x for x, _ in ents]))
            assert (gate, resp[0], resp_term) == (G.G_PASS, F.ACCEPT, wterm - 1), k
            assert ev == G.EV_HARD_STATE | G.EV_LEADER_CHANGED and n.lead == c["from"]
            due = [n.tick() for _ in range(2 * c["election_tick"] - 1)]
            assert sum(due) == 1, (k, seed, due)
            assert (n.term + 1, n.log.last_index, n.log.terms[-1]) == (wterm, ents[-1][1], ents[-1][0]), k


def test_model_advance_commit_index_by_vote_request():
    """test_raft.rs test_advance_commit_index_by_vote_request, node 4's side, for use_prevote in (false, true) and both conf-change
    cases (the entry's bytes stay on the host: only its index matters here). Node 1 led term 1: the noop (1), the conf change
    (cc_index = 2), one more proposal (3) that only node 4 got; node 4 knows commit 1. Node 2 holds entries 1..2, knows commit 2
    and campaigns: node 4 rejects it -- its own log is longer -- and takes the commit index from the request."""
    t = GOLD["ADVANCE_COMMIT_BY_VOTE"]
    assert t["voters"] == [1, 2, 3] and t["learners"] == [4] and (t["candidate"], t["recipient"]) == (2, 4)
    assert t["use_prevote"] == [False, True] and len(t["cases"]) == 2
    cc_index = 2
    for case in t["cases"]:
        for use_prevote in t["use_prevote"]:
            n = G.Node(G.Config(10, flags=G.PRE_VOTE if use_prevote else 0), t["recipient"], F.Log(0, 0, [1, 1, 1], 1))
            n.load(1, 1, 1, 0, G.FOLLOWER, 0, 0, False)  # a learner is not promotable
            assert n.log.committed < cc_index
            assert not any(n.tick() for _ in range(n.timeout)) and n.role == G.FOLLOWER  # it cannot start an election
            m = G.Msg(G.PREVOTE if use_prevote else G.VOTE, 2, t["candidate"], index=2, log_term=1, commit=cc_index, commit_term=1)
            gate, ev, resp_term, resp = n.step(m)
            assert gate == G.G_VOTE_REJECT and resp[2] == 1 and resp[5] == 1  # commit_info, taken before
            assert n.log.committed >= cc_index and ev & G.EV_HARD_STATE and not ev & G.EV_CONF_CHECK
            assert (n.term, resp_term) == ((1, 1) if use_prevote else (2, 2))


# ---------------------------------------------------------------------------------------------------------------------
# 2.-4. the host twin of the gate in csrc/rg_follow.h against the model
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
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, os.path.join(HERE, "host_check", "gate_twin.cpp"), "-o", exe])
    return exe


def state_text(c):
    return "%d %d %d %d %d%s" % (c["committed"], c["last_index"], c["dummy_index"], c["dummy_term"], len(c["runs"]),
                                 "".join(" %d %d" % r for r in c["runs"]))


def soft_text(s):
    term, vote, lead, priority, role, elapsed, timeout, promotable = s
    return "%d %d %d %d %d %d %d %d" % (term, vote, lead, priority, role, elapsed, timeout, promotable)


def msg_text(g, m):
    if m.kind == G.APPEND:
        rs = F.entry_runs(m.ents)
    else:
        rs = [(m.commit_term, 0)]
    return "M %d %d %d %d %d %d %d %d %d %d%s" % (g, m.kind, m.term, m.frm, m.priority, G.FORCE if m.force else 0, m.index, m.log_term, m.commit,
                                                  len(rs), "".join(" %d %d" % x for x in rs))


def answer_text(a):
    gate, ev, resp_term, resp = a
    return "R %d %d %d %d %d %d %d %d %d" % ((gate, ev, resp_term) + tuple(resp))


def twin_io(cfg, events, seed):
    """(stdin of the twin, the stdout the model expects)."""
    rng = random.Random(seed)
    lines, expect = ["N %d %d %d %d %d %d" % (N_FOLLOW, cfg.election_tick, cfg.min_timeout, cfg.max_timeout, cfg.flags, cfg.seed)], []
    for ev in events:
        if ev[0] == "W":
            lines.append("W %d %s" % (ev[1], state_text(ev[2])))
            expect.append("W 0")
        elif ev[0] == "G":
            lines.append("G %d %s" % (ev[1], soft_text(ev[2])))
            expect.append("G 0")
            lines.append("Q %d" % ev[1])
            expect.append("Q " + soft_text(ev[3]))
        elif ev[0] == "K":
            lines.append("K %d" % N_FOLLOW)
            expect.append("K %d%s" % (len(ev[1]), "".join(" %d" % g for g in ev[1])))
            for g in ev[1] + rng.sample(GROUPS, 4):
                lines.append("Q %d" % g)
                expect.append("Q " + soft_text(ev[2][g]))
        else:
            _, g, m, a, c, s = ev
            lines.append(msg_text(g, m))
            expect.append(answer_text(a))
            lines.append("S %d" % g)
            expect.append("S " + state_text(c))
            lines.append("Q %d" % g)
            expect.append("Q " + soft_text(s))
    return "\n".join(lines) + "\n", expect


def run_stream(args):
    exe, (seed, cfg), n_ops = args
    events, cov = G.make_stream(seed, cfg, GROUPS, n_ops)
    text, expect = twin_io(cfg, events, seed)
    out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, (seed, out.returncode, out.stderr[-2000:])
    got = out.stdout.split("\n")[:-1]
    assert len(got) == len(expect), (seed, len(got), len(expect))
    for k, (a, b) in enumerate(zip(got, expect)):
        assert a == b, (seed, k, text.split("\n")[k + 1], a, b)
    return n_ops, cov


def _cov_of(args):
    return G.make_stream(args[0], args[1], GROUPS, 4000)[1]


def test_stream_coverage_from_the_model_alone():
    """Every stream the twin and the GPU tests use contains: all five kinds at m.term <, =, > term, every role at each of the
    three, every gate answer (STALE_LEADER under either flag), every status of the log step with HOST and FAULT, every events
    bit, clock ticks and hups."""
    with ProcessPoolExecutor(max_workers=4) as ex:
        covs = list(ex.map(_cov_of, CONFIGS))
    for (seed, cfg), cov in zip(CONFIGS, covs):
        G.check_coverage(cov, cfg)
    lease = [cov.get(("gate", G.G_IGNORED), 0) for _, cov in zip(CONFIGS, covs)]
    assert all(lease)
    assert {cfg.flags for _, cfg in CONFIGS} == {0, 1, 2, 3}


def test_host_twin_matches_the_model(tmp_path):
    """>= 200 000 operations: every gate answer, events word, response term, log response, canonical log state and soft state."""
    exe = build_twin(tmp_path, "gate_twin", [])
    with ProcessPoolExecutor(max_workers=4) as ex:
        res = list(ex.map(run_stream, [(exe, sc, OPS_PER_SEED) for sc in CONFIGS]))
    assert sum(n for n, _ in res) >= 200000
    for (seed, cfg), (_, cov) in zip(CONFIGS, res):
        G.check_coverage(cov, cfg)


def test_host_twin_refusals(tmp_path):
    """Malformed records (a term or a sender of 0, flags that are not exactly one kind, a vote with entries) are refused; a soft
    state that breaks a rule of rg_follow_soft_write is refused and nothing is written; the clock's cap holds due groups back
    without restarting them."""
    exe = build_twin(tmp_path, "gate_twin", [])
    good = (5, 2, 3, -1, 0, 4, 12, 1)
    bad = [(5, 2, 3, 0, 3, 4, 12, 1), (5, 2, 3, 0, 1, 4, 12, 1), (5, 2, 0, 0, 0, 4, 9, 1), (5, 2, 0, 0, 0, 4, 20, 1), (5, 2, 0, 0, 0, 32768, 12, 1),
           (5, 2, 0, 0, 0, 4, 12, 2)]
    lines = ["N 4 10 10 20 0 1", "G 1 " + soft_text(good), "Q 1"]
    for b in bad:
        lines += ["G 1 " + soft_text(b), "Q 1"]
    lines += ["M 1 1 0 3 0 0 0 0 0 1 0 0", "M 1 1 5 0 0 0 0 0 0 1 0 0", "M 1 3 5 3 0 0 0 0 0 1 0 0", "M 1 0 5 3 0 0 0 0 0 1 0 0", "M 1 4 5 3 0 0 0 0 0 1 0 1",
              "M 1 32 5 3 0 0 0 0 0 1 0 0", "Q 1"]
    # clock: groups 0, 2, 3 promotable with timeout 10 and elapsed 9 -> all due; cap 2 delivers the first two only
    lines += ["G %d 1 0 0 0 0 9 10 1" % g for g in (0, 2, 3)] + ["K 2", "Q 0", "Q 2", "Q 3", "K 4", "Q 3"]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")[:-1]
    assert out[0] == "G 0" and out[1] == "Q " + soft_text(good)
    for k, rule in enumerate((1, 2, 3, 3, 4, 5)):  # (rg_follow_soft_check's numbering)
        assert out[2 + 2 * k] == "G %d" % rule and out[3 + 2 * k] == out[1], (k, out[2 + 2 * k])
    p = 2 + 2 * len(bad)
    assert out[p:p + 6] == ["R malformed"] * 6 and out[p + 6] == out[1]
    p += 7 + 3
    assert out[p] == "K 2 0 2" and out[p + 1:p + 4] == ["Q 1 0 0 0 0 0 10 1", "Q 1 0 0 0 0 0 10 1", "Q 1 0 0 0 0 10 10 1"]
    assert out[p + 4] == "K 1 3" and out[p + 5] == "Q 1 0 0 0 0 0 10 1"


def test_host_twin_is_clean_under_asan_and_ubsan(tmp_path):
    """The same program, -fsanitize=address,undefined -fno-sanitize-recover=all, run directly (a stand-alone executable)."""
    exe = build_twin(tmp_path, "gate_twin_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    for sc in (CONFIGS[3], CONFIGS[4]):
        n, cov = run_stream((exe, sc, 5000))
        assert n == 5000
        G.check_coverage(cov, sc[1])


# ---------------------------------------------------------------------------------------------------------------------
# 5. resources
# ---------------------------------------------------------------------------------------------------------------------
def test_gate_kernels_use_no_scratch():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc is needed (the engine is built with it)")
    cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-c", os.path.join(ROOT, "raft_rs_amd", "csrc", "abi_follow.hip"),
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
    for name in ("k_follow_gate_dense", "k_follow_gate_list", "k_follow_clock"):
        row = [v for k, v in rows.items() if name in k]
        assert len(row) == 1, (name, sorted(rows), err[-2000:])
        print(name, row[0])
        assert int(row[0]["ScratchSize [bytes/lane]"]) == 0, (name, row[0])
