"""CPU only: ReadIndex. (1) tests/readonly_model.py is pinned with the reference's own ReadIndex tests, whose rows and constants
are committed as data (tests/golden/read_only.json, extracted by tests/golden/make_readonly_golden.py); (2) csrc/rg_read.h -- the
arithmetic the kernels run -- is compiled for the HOST with g++ (tests/host_check/read_twin.cpp, a stand-alone program) and
diffed against the model over seeded random operations, once more under AddressSanitizer + UBSan.

Citations: pingcap/raft-rs v0.6.0, harness/tests/integration_cases/test_raft.rs."""
import json
import os
import random
import shutil
import subprocess

import pytest

import readonly_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = json.load(open(os.path.join(HERE, "golden", "read_only.json"), encoding="utf-8"))


def cfg_make(incoming, outgoing, self_slot, present):
    return (incoming & 0xff) | ((outgoing & 0xff) << 8) | ((self_slot & 7) << 16) | ((present & 0xff) << 24)


def mask(slots):
    return sum(1 << s for s in slots)


class Handles:
    """The host's side of the boundary: context bytes <-> 64-bit handle."""

    def __init__(self):
        self.by_ctx, self.by_handle = {}, {}

    def of(self, ctx):
        if ctx not in self.by_ctx:
            h = len(self.by_ctx) + 1
            self.by_ctx[ctx], self.by_handle[h] = h, ctx
        return self.by_ctx[ctx]


def leader_of(voters, learners=(), self_id=1):
    """ids -> slots in id order; the leader is id 1 in every one of these tests"""
    ids = sorted(set(voters) | set(learners))
    slot = {i: k for k, i in enumerate(ids)}
    return slot, cfg_make(mask(slot[v] for v in voters), 0, slot[self_id], mask(slot.values()))


def heartbeat_round(g, slot, ctx, from_ids):
    """bcast_heartbeat_with_ctx(ctx) answered by from_ids: the read-only halves of their MsgHeartbeatResponses"""
    out = []
    for i in from_ids:
        out += g.ack(slot[i], ctx)
    return out


def test_option_safe_rows():
    """test_read_only_option_safe: three voters, the leader is 1. Each row sends [ctx_a, ctx_a, ctx_b]: Network::send steps the
    three requests first (their heartbeats queue up behind them) -- QUEUED, DUPLICATE, QUEUED, and the duplicate STILL
    broadcasts (raft.rs:2077-2081) -- then the responses. In the `pending` rows the responses of that round are dropped and a
    later request for ctx_b alone -- a duplicate -- triggers the round that answers both."""
    t = GOLD["option_safe"]
    assert len(t["rows"]) == 6 and t["voters"] == [1, 2, 3]
    slot, cfg = leader_of(t["voters"])
    hs = Handles()
    g = M.Group(cfg, commit=1, term_lo=1, term=1)  # the election's empty entry is committed: index 1
    others = [i for i in t["voters"] if i != 1]
    assert sum(1 for r in t["rows"] if r[4]) == 3
    for id_, proposals, wri, ctxs, pending in t["rows"]:
        g.commit += proposals
        a, b = hs.of(ctxs[0]), hs.of(ctxs[1])
        got = []
        sts = [g.request(c) for c in (a, a, b)]
        assert [s for s, _ in sts] == [M.QUEUED, M.DUPLICATE, M.QUEUED] and not any(rs for _, rs in sts)
        if pending:
            assert g.queue() == [(a, wri, 1 << slot[1]), (b, wri, 1 << slot[1])]  # MsgHeartbeatResponse ignored: both stay
            s, rs = g.request(b)
            assert s == M.DUPLICATE and rs == []
            got += heartbeat_round(g, slot, b, others)
        else:
            for c in (a, a, b):  # three heartbeat rounds, the duplicate's included
                got += heartbeat_round(g, slot, c, others)
        assert [(hs.by_handle[c], i) for c, i in got] == [(ctxs[0], wri), (ctxs[1], wri)]
        assert g.queue() == []


def test_with_learner_rows():
    """test_read_only_with_learner: one voter and one learner: a singleton answers at once (raft.rs:2063-2069)."""
    t = GOLD["with_learner"]
    assert len(t["rows"]) == 4
    slot, cfg = leader_of(t["voters"], t["learners"])
    assert M.is_singleton(cfg)
    g = M.Group(cfg, commit=1, term_lo=1, term=1)
    for _id, proposals, wri, ctx in t["rows"]:
        g.commit += proposals
        assert g.request(Handles().of(ctx)) == (M.READY, [(1, wri)])
    # ... and where the learner's ack is asked for, it is recorded and never counts: two voters and a learner
    slot, cfg = leader_of([1, 2], [3])
    g = M.Group(cfg, commit=5, term_lo=1, term=1)
    assert g.request(7) == (M.QUEUED, [])
    assert g.ack(slot[3], 7) == [] and g.queue() == [(7, 5, 0b101)]
    assert g.ack(slot[2], 7) == [(7, 5)]


def test_option_lease_rows():
    """test_read_only_option_lease: LeaseBased answers with raft_log.committed at once (raft.rs:2083-2088)."""
    t = GOLD["option_lease"]
    assert len(t["rows"]) == 6
    _, cfg = leader_of(t["voters"])
    g = M.Group(cfg, commit=1, term_lo=1, term=1)
    for _id, proposals, wri, ctx in t["rows"]:
        g.commit += proposals
        assert g.request(3, lease=True) == (M.READY, [(3, wri)])
        assert g.queue() == []


def test_for_new_leader_gate():
    """test_read_only_for_new_leader: node 1 holds the stored entries, committed = 1; elected (term hard_state_term + 1) it
    appends its empty entry at last_index + 1 and cannot commit it (MsgAppend dropped): commit_to_current_term() is false
    and the request is dropped. Once a proposal commits index `windex` the same request is served."""
    t = GOLD["for_new_leader"]
    _, cfg = leader_of(t["voters"])
    slot, _ = leader_of(t["voters"])
    committed = {r[0]: r[1] for r in t["node_configs"]}[1]
    last = t["entries"][-1][1]
    g = M.Group(cfg, commit=committed, term_lo=last + 1, term=t["hard_state_term"] + 1)
    assert g.request(9) == (M.NOT_READY, []) and g.queue() == []
    g.commit = last + 2  # the empty entry and the proposal
    assert g.commit == t["windex"]
    assert g.request(9) == (M.QUEUED, [])
    assert heartbeat_round(g, slot, 9, [2, 3]) == [(9, t["windex"])]


def test_quorum_becomes_less_recheck():
    """test_read_when_quorum_becomes_less: two voters, the response of peer 2 is dropped, then peer 2 is removed:
    post_conf_change acks the last pending read from the leader itself and the quorum -- now 1 of 1 -- holds."""
    t = GOLD["quorum_becomes_less"]
    assert t["peers"] == 2 and t["removed"] == 2
    slot, cfg = leader_of([1, 2])
    g = M.Group(cfg, commit=t["committed_after_election"], term_lo=1, term=1)
    h = Handles().of(t["ctx"])
    assert g.request(h) == (M.QUEUED, [])
    assert g.ack(0, 0, M.ACK_LAST_SELF) == []  # (the re-check alone does not make a quorum of two)
    g.cfg = cfg_make(mask([slot[1]]), 0, slot[1], mask([slot[1]]))
    assert g.ack(0, 0, M.ACK_LAST_SELF) == [(h, t["committed_after_election"])]
    assert g.queue() == []


def test_frees_read_only_mem():
    """test_raft_frees_read_only_mem: queue and map hold the read until the follower's ack, and nothing afterwards."""
    t = GOLD["frees_read_only_mem"]
    slot, cfg = leader_of(t["voters"])
    g = M.Group(cfg, commit=1, term_lo=1, term=1)
    h = Handles().of(t["ctx"])
    assert g.request(h) == (M.QUEUED, [])
    assert g.last_pending() == h  # the heartbeat the step sends carries the ctx
    assert g.read_only.pending_read_count() == 1 and list(g.read_only.pending_read_index) == [h]
    assert g.ack(slot[t["ack_from"]], h) == [(h, 1)]
    assert g.read_only.pending_read_count() == 0 and not g.read_only.pending_read_index


def test_term_change_drops_pending_reads_and_full_is_loud():
    """Raft::reset (raft.rs:957) replaces the ReadOnly; the engine's one bound refuses, loudly, instead of dropping."""
    _, cfg = leader_of([1, 2, 3])
    g = M.Group(cfg, commit=4, term_lo=2, term=3, depth=2)
    assert [g.request(c)[0] for c in (5, 6, 7, 6)] == [M.QUEUED, M.QUEUED, M.FULL, M.DUPLICATE]
    g.set_term(4)
    assert g.queue() == [] and g.ack(1, 6) == []


def test_same_term_reset_drops_pending_reads_and_emits_nothing():
    """Group.reset() is `ReadOnly::new` at the UNCHANGED term (raft.rs:957, reached through become_follower(term, INVALID_ID) of a
    check-quorum step-down): the queue and the map are empty, last_pending_request_ctx is None, nothing is emitted -- neither by
    the reset nor by the acks that would have formed a quorum --, the term is what it was, and the whole depth is free again.
    set_term at the same term, by contrast, is no reset."""
    src = open(os.path.join(HERE, "readonly_model.py")).read()
    body = src[src.index("    def reset(self):"):src.index("    def commit_to_current_term")]
    assert "raft.rs:957" in body and "ReadOnly::new" in body
    slot, cfg = leader_of([1, 2, 3])
    for pending in (0, 1, 3, 4):
        g = M.Group(cfg, commit=4, term_lo=2, term=3, depth=4)
        ctxs = list(range(10, 10 + pending))
        assert [g.request(c) for c in ctxs] == [(M.QUEUED, [])] * pending
        if pending:
            assert g.ack(slot[1], ctxs[-1]) == []  # (a half-answered queue: the leader's own ack, one short of the quorum)
        g.set_term(3)
        assert len(g.queue()) == pending
        assert g.reset() is None
        assert g.term == 3 and g.queue() == [] and g.last_pending() == 0 and g.read_only.last_pending_request_ctx() is None
        assert g.read_only.pending_read_count() == 0 and not g.read_only.pending_read_index
        for c in ctxs:
            assert heartbeat_round(g, slot, c, [2, 3]) == []
        assert g.ack(0, 0, M.ACK_LAST_SELF) == [] and g.queue() == []
        fresh = list(range(20, 24))
        assert [g.request(c)[0] for c in fresh + [30]] == [M.QUEUED] * 4 + [M.FULL]
        assert heartbeat_round(g, slot, fresh[-1], [2]) == [(c, 4) for c in fresh]


def test_committed_golden_file_is_what_the_extractor_produces():
    import importlib.util
    if not os.path.isfile("/root/reference/harness/tests/integration_cases/test_raft.rs"):
        pytest.skip("reference tree not present")
    spec = importlib.util.spec_from_file_location("make_readonly_golden", os.path.join(HERE, "golden", "make_readonly_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    assert mg.extract() == GOLD


# ---------------------------------------------------------------------------------------------------------------------
# the host twin of csrc/rg_read.h
# ---------------------------------------------------------------------------------------------------------------------
def build_twin(tmp_path, name, extra):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build the host twin")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "raft_rs_amd", "csrc"),
                           os.path.join(HERE, "host_check", "read_twin.cpp"), "-o", exe])
    return exe


def random_cfg(rng, P):
    """majority / joint / learner-carrying / singleton configurations over P slots"""
    slots = list(range(P))
    kind = rng.choice(["majority", "joint", "learner", "singleton", "sparse"])
    if kind == "singleton" or P == 1:
        v = [rng.choice(slots)]
        learners = [s for s in slots if s not in v and rng.random() < 0.5]
        return cfg_make(mask(v), 0, v[0], mask(v + learners))
    if kind == "majority":
        inc, out, present = slots, [], slots
    elif kind == "joint":
        inc = rng.sample(slots, rng.randint(1, P))
        out = rng.sample(slots, rng.randint(1, P))
        present = sorted(set(inc) | set(out) | {s for s in slots if rng.random() < 0.3})
    elif kind == "learner":
        inc = rng.sample(slots, rng.randint(1, P - 1))
        out = []
        present = slots
    else:  # voters of which some have no Progress, slots that do not exist
        inc = rng.sample(slots, rng.randint(1, P))
        out = []
        present = [s for s in slots if rng.random() < 0.7]
    voters = sorted(set(inc) | set(out))
    self_slot = rng.choice(voters)
    present = sorted(set(present) | {self_slot})
    return cfg_make(mask(inc), mask(out), self_slot, mask(present))


def make_script(seed, P, depth, G, n_ops):
    """-> (script text, the output the model expects); ops counts the records applied"""
    rng = random.Random(seed)
    lines, want = [f"{P} {depth} {G}"], []
    groups = []
    next_ctx = [1]
    p_request = 0.45 if depth <= 4 else 0.8  # (a deep ring fills only under more requests than acks)
    for g in range(G):
        cfg = random_cfg(rng, P)
        lo = rng.randint(1, 5)
        grp = M.Group(cfg, commit=rng.randint(0, 8), term_lo=lo, term=rng.randint(1, 3), depth=depth)
        groups.append(grp)
        lines.append(f"c {g} {cfg} {grp.commit} {grp.term_lo} {grp.term}")
    ops = 0
    while ops < n_ops:
        g = rng.randrange(G)
        grp = groups[g]
        r = rng.random()
        if r < 0.12:  # the state under the queue moves: commit, a new term (Raft::reset), a configuration change
            k = rng.random()
            recheck = False
            if k < 0.5:
                grp.commit += rng.randint(0, 3)
            elif k < 0.7:
                grp.set_term(grp.term + 1)
                grp.term_lo = grp.commit + rng.randint(0, 2)
            else:
                grp.cfg = random_cfg(rng, P)
                recheck = True
            lines.append(f"c {g} {grp.cfg} {grp.commit} {grp.term_lo} {grp.term}")
            if not recheck:
                continue
            recs = [("a", 0, 0, M.ACK_LAST_SELF)]  # post_conf_change's re-check follows the change
        else:
            recs = []
            for _ in range(rng.choice([1, 1, 1, 2, 3, 4])):
                pend = [c for c, _, _ in grp.queue()]
                k = rng.random()
                if k < p_request:
                    if pend and rng.random() < 0.25:
                        ctx = rng.choice(pend)  # a duplicate
                    else:
                        ctx = next_ctx[0]
                        next_ctx[0] += 1
                    recs.append(("r", ctx, 1 if rng.random() < 0.05 else 0, 0))
                elif k < 0.95:
                    j = rng.random()
                    ctx = pend[-1] if pend and j < 0.6 else rng.choice(pend) if pend and j < 0.8 else 0 if j < 0.9 else rng.randint(1, next_ctx[0] + 3)
                    recs.append(("a", rng.randrange(P + 1 if P < 8 else P), ctx, 0))  # (slot P: one the engine does not have)
                else:
                    recs.append(("a", 0, 0, M.ACK_LAST_SELF))
                # (the pending set the next record of the batch draws from is the model's, after this one)
                if recs[-1][0] == "r":
                    grp_states = grp.request(recs[-1][1], bool(recs[-1][2]))
                    recs[-1] = recs[-1] + (grp_states,)
                else:
                    recs[-1] = recs[-1] + (grp.ack(recs[-1][1], recs[-1][2], recs[-1][3]),)
        lines.append(f"b {g} {len(recs)}")
        sts, ems = [], []
        for rec in recs:
            lines.append(f"{rec[0]} {rec[1]} {rec[2]} {rec[3]}")
            if len(rec) == 4:  # (the re-check record: not applied yet)
                rec = rec + (grp.ack(rec[1], rec[2], rec[3]),)
            if rec[0] == "r":
                sts.append(rec[4][0])
                ems += rec[4][1]
            else:
                ems += rec[4]
        want.append("s" + "".join(f" {s}" for s in sts))
        want += [f"e {g} {c} {i}" for c, i in ems]
        ops += len(recs)
    for g, grp in enumerate(groups):
        q = grp.queue()
        want.append(f"q {g} {len(q)}" + "".join(f" {c}:{i}:{a}" for c, i, a in q))
    return "\n".join(lines) + "\n", "\n".join(want) + "\n", ops


# (depth 7: the ring wraps at a size that is no power of two; depth 16: RG_READ_MAX_DEPTH, the whole RgReadCopy)
CASES = [(P, depth) for P in range(1, 9) for depth in (1, 2, 4, 7, 16)]


def run_twin(exe, tmp_path, n_per_case):
    total = 0
    seen, full_at = set(), set()
    for k, (P, depth) in enumerate(CASES):
        # (the cases of depth 1, 2 and 4 keep the seeds they had before depths 7 and 16 joined them)
        seed = 1000 + (P - 1) * 3 + (1, 2, 4).index(depth) if depth <= 4 else 2000 + k
        script, want, ops = make_script(seed, P, depth, 12, n_per_case)
        path = tmp_path / f"script_{P}_{depth}.txt"
        path.write_text(script)
        r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, (P, depth, r.returncode, r.stderr[-2000:])
        if r.stdout != want:
            got, exp = r.stdout.split("\n"), want.split("\n")
            i = next(i for i in range(min(len(got), len(exp))) if got[i] != exp[i])
            pytest.fail(f"P={P} depth={depth}: line {i}: twin {got[i]!r}, model {exp[i]!r}")
        total += ops
        for line in want.split("\n"):
            if line.startswith("s "):
                seen |= set(line.split()[1:])
                if str(M.FULL) in line.split()[1:]:
                    full_at.add(depth)
    return total, seen, full_at


def test_host_twin_matches_the_model(tmp_path):
    """>= 200 000 seeded random operations over P = 1..8 x depth 1, 2, 4, 7, 16: joint configurations, learners, singletons, voters
    without a Progress, term bumps, configuration changes followed by the re-check, duplicates, unknown contexts, absent slots.
    Statuses, emitted states and final queues must be the model's, line for line."""
    exe = build_twin(tmp_path, "read_twin", [])
    total, seen, full_at = run_twin(exe, tmp_path, 8500)
    assert total >= 200000
    assert full_at == {1, 2, 4, 7, 16}  # every ring was full at some point, the deepest included
    assert seen == {str(s) for s in (M.NOT_READY, M.READY, M.QUEUED, M.DUPLICATE, M.FULL)}


def test_host_twin_is_clean_under_asan_and_ubsan(tmp_path):
    """The same program, -fsanitize=address,undefined -fno-sanitize-recover=all, run directly (a stand-alone executable)."""
    exe = build_twin(tmp_path, "read_twin_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    total, _, full_at = run_twin(exe, tmp_path, 1500)
    assert total >= len(CASES) * 1500 and full_at == {1, 2, 4, 7, 16}
