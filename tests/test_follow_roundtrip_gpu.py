"""GPU: the plumbing the follower side's sparse calls share -- one staging round trip, one run cutter, one table of layers -- seen
from outside: a batch that outgrows the record staging between two small ones, which of two faults in one batch is reported, and
the bookkeeping of the arena's three layers. Every answer and every cell against the models the follower, gate, election and
hand-off tests use. No test provokes a device fault: every bad argument is refused on the host."""
import random

import numpy as np
import pytest

import elect_model as M
import follower_model as F
import gate_model as G
import handoff_model as H
import handoff_rig as R
from test_follow_elect_gpu import Arena, cells_array
from test_follow_gate_gpu import answer, canon_of, records_arrays, soft_array, states_array
from test_follower_gpu import records_arrays as step_arrays, resp_tuple
from test_handoff_gpu import Rig

pytestmark = pytest.mark.gpu

N = 300  # followed groups: one full workgroup of 256 lanes and a partial one, inside a stride of 512
CFG = G.Config(3, flags=G.CHECK_QUORUM | G.PRE_VOTE, seed=77)
FIRST = 65536  # the first capacity of the record staging
NO_LEAD = 0xFFFFFFFFFFFFFFFF  # RG_HANDOFF_NO_LEAD: a vote record of a group this store does not lead


def align(x):
    return (x + 255) & ~255


def first_past(staged):
    """The smallest record count whose staged bytes exceed the staging's first capacity"""
    n = 1
    while staged(n) <= FIRST:
        n += 1
    return n


class Trip(Arena):
    """The election tests' arena of N groups with all three layers, and the model's node of every group."""

    def __init__(self, rg, seed):
        super().__init__(rg, N, CFG)
        E = self.E
        # what loads and checks the arena stays inside the first capacity, so the staging grows in the call under test
        assert align(N * 8) + N * max(E.FOLLOW_STATE_DTYPE.itemsize, E.FOLLOW_SOFT_DTYPE.itemsize, E.FOLLOW_ELECT_DTYPE.itemsize) <= FIRST
        self.rng = rng = random.Random(seed)
        self.nodes = [M.Node(CFG, g) for g in range(N)]
        loads = []
        for nd in self.nodes:  # (as elect_model.plan_rounds loads a group)
            log = M.random_log(rng)
            w = M.random_soft(rng, CFG, log)
            e = M.random_elect(rng, w)
            if w[4] == M.CANDIDATE:
                w = (w[0], e[0]) + w[2:]
            nd.log = log
            nd.load(*w)
            nd.load_elect(*e[:4])
            loads.append((log.canonical(), w, e[:4]))
        self.load(list(range(N)), [x[0] for x in loads], [x[1] for x in loads], [x[2] for x in loads])
        self.check_nodes(self.nodes, "load")

    def batch(self, n, draw, apply):
        """n records over random groups, several of one group in array order -> ([(g, record)], the model's answers)"""
        recs, want = [], []
        for _ in range(n):
            g = self.rng.randrange(N)
            m = draw(self.nodes[g])
            recs.append((g, m))
            want.append(apply(self.nodes[g], m))
        return recs, want

    def small_big_small(self, big, draw, apply, call):
        assert big > 3
        for n in (3, big, 3):
            recs, want = self.batch(n, draw, apply)
            got = call(recs)
            bad = [(i, recs[i][0], got[i], want[i]) for i in range(n) if got[i] != want[i]]
            assert not bad, (n, bad[:3])
            self.check_nodes(self.nodes, n)


# ---------------------------------------------------------------------------------------------------------------------
# A. staging growth: 3 records, a batch past the first capacity, 3 records again
# ---------------------------------------------------------------------------------------------------------------------
def test_staging_growth_follow_step(rg):
    t = Trip(rg, 1)
    big = first_past(lambda n: n * t.E.FOLLOW_MSG_DTYPE.itemsize)  # (the records alone; orig, runs, ext and resp come on top)
    t.small_big_small(big, lambda nd: F.random_op(t.rng, nd.log), lambda nd, op: F.step(nd.log, op),
                      lambda recs: [resp_tuple(r) for r in t.eng.follow_step(*step_arrays(rg, recs))])
    t.close()


def test_staging_growth_follow_step_gated(rg):
    t = Trip(rg, 2)
    big = first_past(lambda n: n * t.E.FOLLOW_MSG_DTYPE.itemsize)

    def call(recs):
        resp, gate = t.eng.follow_step_gated(*records_arrays(t.E, recs))
        return [answer(r, g) for r, g in zip(resp, gate)]

    def step(nd, m):
        votes = dict(nd.votes)
        a = nd.step(m)
        if a[3][0] in (F.FAULT, F.HOST):  # gate_model's step took its node back; of the votes elect_model's reset cleared it knows nothing
            nd.votes = votes
        return a
    t.small_big_small(big, lambda nd: G.random_msg(t.rng, nd), step, call)
    t.close()


def test_staging_growth_follow_vote_resps(rg):
    t = Trip(rg, 3)
    big = first_past(lambda n: n * t.E.FOLLOW_VOTE_REC_DTYPE.itemsize)  # (they are staged wider, as RgElectStaged)

    def response(nd):
        while True:
            m = M.random_rec(t.rng, nd)
            if m.kind in (M.VOTE, M.PREVOTE):
                return m
    t.small_big_small(big, response, lambda nd, m: nd.record(m), t.responses)
    t.close()


def test_staging_growth_follow_read(rg):
    t = Trip(rg, 4)
    size = t.E.FOLLOW_STATE_DTYPE.itemsize
    big = first_past(lambda n: align(n * 8) + n * size)
    for n in (3, big, 3):
        groups = np.array([t.rng.randrange(N) for _ in range(n)], dtype=np.uint64)  # (a read may name a group twice)
        got = t.eng.follow_read(groups)
        assert (got["group"] == groups).all()
        bad = [(i, int(g)) for i, g in enumerate(groups) if canon_of(got[i]) != t.nodes[int(g)].log.canonical()]
        assert not bad, (n, bad[:3])
        t.check_nodes(t.nodes, n)
    t.close()


class BigRig(Rig):
    """The hand-off tests' rig with an arena and a leader engine of `n` groups x 3 slots. A promotion names no group twice, so a
    batch past the staging's first capacity needs more than 300 followed groups: this arena is the smallest that holds the three
    batches. Loads and read-backs go in pieces of 256 records, so that the staging grows in the promotion alone."""

    def __init__(self, rg, n):
        self.rg, self.E, self.P, self.G, self.n = rg, rg.engine, 3, n, n
        self.eng = rg.Engine(n, 3)
        self.eng.follow_enable(n)
        self.stride = self.eng.follow_stride()
        self.eng.follow_gate_enable(CFG.election_tick, CFG.min_timeout, CFG.max_timeout, CFG.flags, CFG.seed)
        self.eng.follow_elect_enable()

    def arena(self):
        out = []
        for k in range(0, self.n, 256):
            self.all = np.arange(k, min(k + 256, self.n), dtype=np.uint64)
            out += super().arena()
        return out


def test_staging_growth_follow_promote(rg):
    E = rg.engine
    big = first_past(lambda n: align(n * E.HANDOFF_REC_DTYPE.itemsize) + n * E.HANDOFF_RESP_DTYPE.itemsize)
    n = 3 + big + 3
    assert n % 256 and big > 256
    rng = random.Random(5)
    lead_of = list(range(n))
    rng.shuffle(lead_of)
    cases = []
    for g in range(n):
        f, lead, persisted = H.random_case(rng, 3)
        lead = H.make_lead(3, lead["cfg"], rng)  # (the sweep's cfg word on a lead group as a previous leadership left it)
        cases.append(H.Case("g%d" % g, g, lead_of[g], f, lead, persisted, H.promote(f, H.copy_lead(lead), 3, persisted)[0]))
    assert {c.expect for c in cases} == {H.DONE, H.NOT_WON, H.CONF, H.NOT_PERSISTED, H.FAULT}
    r = BigRig(rg, n)
    st = R.state_with(n, 3, r.eng.stride, cases)
    r.load_lead(st)
    for k in range(0, n, 256):
        r.load_arena(cases[k:k + 256])
    arena = r.arena()
    assert all(arena[c.g][0] == c.f.canonical() for c in cases)
    rng.shuffle(cases)
    for batch in (cases[:3], cases[3:3 + big], cases[3 + big:]):
        st, answers = R.model_state(st, batch)
        r.promote(batch, False, answers)
        d = R.diff(st, r.read_lead())
        assert not d, (len(batch), d)
        assert r.arena() == arena, "a promotion leaves all three layers of the arena alone"
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# B. of two faults in one batch, the first record's is reported: range, rule and repeated group are checked per record
# ---------------------------------------------------------------------------------------------------------------------
def soft_recs(E, rows):
    return soft_array(E, [g for g, _ in rows], [(2, 0, 0, 0, role, 0, 0, 1) for _, role in rows])


def elect_recs(E, rows):
    return cells_array(E, [g for g, _ in rows], [(self_id, 7 | 1 << 16, 0, 0) for _, self_id in rows])


def campaign_recs(E, rows):
    a = np.zeros(len(rows), dtype=E.FOLLOW_CAMPAIGN_REQ_DTYPE)
    for k, (g, flags) in enumerate(rows):
        a[k]["group"], a[k]["flags"] = g, flags
    return a


def handoff_recs(E, rows):
    a = np.zeros(len(rows), dtype=E.HANDOFF_REC_DTYPE)
    for k, (g, L) in enumerate(rows):
        a[k]["follow_group"], a[k]["lead_group"] = g, L
    return a


def depose_recs(E, rows):
    a = np.zeros(len(rows), dtype=E.DEPOSE_REC_DTYPE)
    for k, (g, L, reserved) in enumerate(rows):
        a[k]["follow_group"], a[k]["lead_group"], a[k]["term"], a[k]["reserved"] = g, L, 9, reserved
    return a


def vote_recs(E, rows):
    a = np.zeros(len(rows), dtype=E.VOTE_REC_DTYPE)
    for k, (g, L, term) in enumerate(rows):
        a[k]["follow_group"], a[k]["lead_group"], a[k]["term"], a[k]["from"], a[k]["kind"] = g, L, term, 3, E.FOLLOW_MSG_VOTE
    return a


# call -> (its entry point, records from rows, [(rows, the message behind "<entry point>: " -- or, where it begins with the entry
# point's name, the whole message)]); rows of the cell writes: (group, role) / (group, self_id); of the campaign: (group, flags); of
# the hand-off and the step-down: (follow group, lead group); of the deposition: (follow group, lead group, reserved); of the vote:
# (follow group, lead group, term). The engine leads 300 groups and follows 300.
TWO_FAULTS = {
    "follow_soft_write": ("rg_follow_soft_write", soft_recs, [
        ([(5, 0), (5, 0), (300, 0)], "records 0 and 1 name group 5"),
        ([(5, 0), (300, 0), (5, 0)], "record 1: group 300 of 300"),
        ([(5, 0), (6, 3), (5, 0)], "record 1 (group 6) breaks rule 1 of rg_follow_soft_check"),
        ([(5, 0), (5, 3), (300, 0)], "record 1 (group 5) breaks rule 1 of rg_follow_soft_check"),  # (the rule stands before the repeat)
        ([(5, 0), (6, 0), (7, 0), (6, 0), (5, 0)], "records 1 and 3 name group 6")]),
    "follow_elect_write": ("rg_follow_elect_write", elect_recs, [
        ([(5, 9), (5, 9), (300, 9)], "records 0 and 1 name group 5"),
        ([(5, 9), (300, 9), (5, 9)], "record 1: group 300 of 300"),
        ([(5, 9), (6, 0), (5, 9)], "record 1 (group 6) breaks rule 1 of rg_follow_elect_check"),
        ([(5, 9), (5, 0), (300, 9)], "record 1 (group 5) breaks rule 1 of rg_follow_elect_check"),
        ([(5, 9), (6, 9), (7, 9), (6, 9), (5, 9)], "records 1 and 3 name group 6")]),
    "follow_campaign": ("rg_follow_campaign", campaign_recs, [
        ([(5, 0), (5, 0), (300, 0)], "records 0 and 1 name group 5"),
        ([(5, 0), (300, 0), (5, 0)], "record 1: group 300 of 300, flags 0, term 0, from 0"),
        ([(5, 0), (6, 1), (5, 0)], "record 1: group 6 of 300, flags 0x1, term 0, from 0"),  # (MsgTimeoutNow without term and sender)
        ([(5, 0), (5, 4), (300, 0)], "record 1: group 5 of 300, flags 0x4, term 0, from 0"),
        ([(5, 0), (6, 0), (7, 0), (6, 0), (5, 0)], "records 1 and 3 name group 6")]),
    "follow_promote": ("rg_follow_promote", handoff_recs, [
        ([(5, 7), (5, 8), (300, 9)], "records 0 and 1 name follow group 5"),
        ([(5, 7), (6, 300), (5, 8)], "record 1: follow group 6 of 300, lead group 300 of 300"),
        ([(5, 7), (300, 8), (6, 7)], "record 1: follow group 300 of 300, lead group 8 of 300"),
        ([(5, 7), (5, 7), (6, 300)], "records 0 and 1 name follow group 5"),  # (both repeat: the follow group is looked at first)
        ([(5, 7), (6, 7), (5, 8)], "records 0 and 1 name lead group 7")]),
    # the three extension calls: the promotion's rows, and the record's own rule in front of a repeat and a range fault
    "follow_step_down": ("rgx_follow_step_down", handoff_recs, [
        ([(5, 7), (5, 8), (300, 9)], "rgx_follow_step_down (follow): records 0 and 1 name group 5"),
        ([(5, 7), (6, 300), (5, 8)], "record 1: follow group 6 of 300, lead group 300 of 300"),
        ([(5, 7), (300, 8), (6, 7)], "record 1: follow group 300 of 300, lead group 8 of 300"),
        ([(5, 7), (5, 7), (6, 300)], "rgx_follow_step_down (follow): records 0 and 1 name group 5"),
        ([(5, 7), (6, 7), (5, 8)], "rgx_follow_step_down (lead): records 0 and 1 name group 7")]),
    "follow_depose": ("rgt_follow_depose", depose_recs, [
        ([(5, 7, 0), (5, 8, 0), (300, 9, 0)], "rgt_follow_depose (follow): records 0 and 1 name group 5"),
        ([(5, 7, 0), (6, 300, 0), (5, 8, 0)], "record 1: follow group 6 of 300, lead group 300 of 300"),
        ([(5, 7, 0), (300, 8, 0), (6, 7, 0)], "record 1: follow group 300 of 300, lead group 8 of 300"),
        ([(5, 7, 0), (5, 7, 0), (6, 300, 0)], "rgt_follow_depose (follow): records 0 and 1 name group 5"),
        ([(5, 7, 0), (6, 7, 0), (5, 8, 0)], "rgt_follow_depose (lead): records 0 and 1 name group 7"),
        ([(5, 7, 0), (5, 7, 1), (300, 9, 0)], "record 1: reserved is 1"),  # (the rule stands before both repeats)
        ([(5, 7, 0), (6, 8, 4), (5, 9, 0)], "record 1: reserved is 4")]),
    "follow_vote": ("rgv_follow_vote", vote_recs, [
        ([(5, 7, 2), (5, 8, 2), (300, 9, 2)], "rgv_follow_vote (follow): records 0 and 1 name group 5"),
        ([(5, 7, 2), (6, 300, 2), (5, 8, 2)], "record 1: follow group 6 of 300, lead group 300 of 300"),
        ([(5, 7, 2), (300, 8, 2), (6, 7, 2)], "record 1: follow group 300 of 300, lead group 8 of 300"),
        ([(5, 7, 2), (5, 7, 2), (6, 300, 2)], "rgv_follow_vote (follow): records 0 and 1 name group 5"),
        ([(5, 7, 2), (6, 7, 2), (5, 8, 2)], "rgv_follow_vote (lead): records 0 and 1 name group 7"),
        ([(5, 7, 2), (5, 7, 0), (300, 9, 2)], "record 1: kind 0x4, term 0, from 3, flags 0x0"),
        ([(5, 7, 2), (6, 8, 0), (5, 9, 2)], "record 1: kind 0x4, term 0, from 3, flags 0x0"),
        # (no lead group, twice: not a repeat; the lead group that is one stands behind it)
        ([(5, NO_LEAD, 2), (6, NO_LEAD, 2), (7, 8, 2), (9, 8, 2)], "rgv_follow_vote (lead): records 2 and 3 name group 8")]),
}
TWO_FAULTS["follow_demote"] = ("rg_follow_demote",) + TWO_FAULTS["follow_promote"][1:]


@pytest.mark.parametrize("call", sorted(TWO_FAULTS))
def test_first_fault_wins(rg, call):
    t = Trip(rg, 6)
    before = t.states()
    entry, make, table = TWO_FAULTS[call]
    for rows, text in table:
        with pytest.raises(rg.EngineError) as ei:
            getattr(t.eng, call)(make(t.E, rows))
        assert ei.value.code == t.E.ERR["INVALID_ARG"], (rows, str(ei.value))
        want = text if text.startswith(entry) else "%s: %s" % (entry, text)
        assert str(ei.value) == "raftgroups error -1: " + want, (rows, str(ei.value))
        assert t.states() == before, rows
    t.check_nodes(t.nodes, "after the refusals")
    t.close()


# ---------------------------------------------------------------------------------------------------------------------
# C. the layers' bookkeeping
# ---------------------------------------------------------------------------------------------------------------------
def enables(eng):
    return (lambda: eng.follow_enable(N), lambda: eng.follow_gate_enable(CFG.election_tick, seed=CFG.seed), eng.follow_elect_enable)


def enable_prefix(eng, k):
    for enable in enables(eng)[:k]:
        enable()


def test_engine_bytes_after_each_enable(rg):
    eng = rg.Engine(300, 3)
    S = 512
    # the log summary: six u64 columns, two tables of TERM_RUNS u64 rows, one byte per group; the soft cells: term, lead, vote,
    # priority (8 bytes each), clock (4), role (1), then the clock's two count words; the election cells: self_id (8), conf (4), votes (2)
    sizes = (S * 8 * (6 + 2 * rg.engine.TERM_RUNS) + S, S * (8 + 8 + 8 + 8 + 4 + 1) + 16, S * (8 + 4 + 2))
    assert sizes == (S * 177, S * 37 + 16, S * 14)
    want = eng.device_info()["engine_bytes"]
    for k, (enable, size) in enumerate(zip(enables(eng), sizes)):
        assert bool(eng.follow_clock_counts()) == (k == 2)  # null until the gate is enabled
        enable()
        want += size
        assert eng.follow_stride() == S and eng.device_info()["engine_bytes"] == want, k
    eng.close()


def test_checkpoint_and_restore_carry_all_three_layers(rg):
    t = Trip(rg, 7)
    saved = t.states()
    t.eng.checkpoint()
    gs = [0, 255, 256, N - 1]
    t.load(gs, [H.canon(0, 0, [(1, 5)], 9, 4)] * 4, [(11, 0, 3, 0, G.FOLLOWER, 1, 4, 1)] * 4, [(42, 3 | 1 << 16, 2, 1)] * 4)
    changed = t.states()
    for g in gs:
        assert all(changed[g][k] != saved[g][k] for k in range(3)), g
    t.eng.restore()
    assert t.states() == saved
    t.check_nodes(t.nodes, "restore")
    t.eng.checkpoint()  # (the copies exist now: a second checkpoint and restore reuse them)
    t.load(gs[:1], [H.canon(0, 0, [], 0)])
    t.eng.restore()
    assert t.states() == saved
    t.close()


@pytest.mark.parametrize("layers", [0, 1, 2, 3])
def test_destroy_after_every_prefix_of_the_enables(rg, layers):
    eng = rg.Engine(300, 3)
    enable_prefix(eng, layers)
    if layers:
        eng.checkpoint()  # (the checkpoint copies are the layers' to free as well)
        assert len(eng.follow_read(np.arange(N, dtype=np.uint64))) == N
    eng.sync()
    eng.close()
    again = rg.Engine(300, 3)  # the device is as usable as before
    enable_prefix(again, 3)
    assert again.follow_clock(None, 0) == 0
    again.close()
