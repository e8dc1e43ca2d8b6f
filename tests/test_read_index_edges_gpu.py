"""GPU: ReadIndex at the edges of its kernels -- every slot count, the full depth-16 ring, the workgroup scan of rg_read_reserve
across wave and workgroup boundaries, a list that grows under one lane, the order contract of the list itself, and the capacity
bookkeeping across rg_restore and elections. As in test_read_index_gpu.py the model (tests/readonly_model.py) is the reference,
word for word; here the drained list is compared RAW: call by call, a group's states contiguous and in queue order."""
import copy

import numpy as np
import pytest

import readonly_model as M
from test_read_index_gpu import G, Rig, cfg_make, random_rounds

pytestmark = pytest.mark.gpu
ALL5 = {M.NOT_READY, M.READY, M.QUEUED, M.DUPLICATE, M.FULL}
U64 = (1 << 64) - 1


def assert_list_order(got, calls):
    """include/raftgroups.h: "A group's states are contiguous inside what one call appended and in queue order" and, between
    calls, call order. got: the drained list as it came; calls: what the model emitted, one list per call."""
    got = [tuple(int(x) for x in s) for s in got]
    assert len(got) == sum(len(c) for c in calls), (len(got), [len(c) for c in calls])
    at = 0
    for k, want in enumerate(calls):
        seg = got[at:at + len(want)]
        at += len(want)
        runs = [s[0] for i, s in enumerate(seg) if i == 0 or seg[i - 1][0] != s[0]]
        assert len(runs) == len(set(runs)), (k, "a group's states are not contiguous", [g for g in set(runs) if runs.count(g) > 1][:5])
        per_group = {}
        for s in want:
            per_group.setdefault(s[0], []).append(s)
        i = 0
        for g in runs:
            w = per_group.pop(g, None)
            assert w is not None and seg[i:i + len(w)] == w, (k, g, seg[i:i + 4], (w or [])[:4])
            i += len(w)
        assert not per_group, (k, sorted(per_group)[:5])


class OrderedRig(Rig):
    """A Rig that remembers what the model emitted per call, and compares the drained list with it unsorted."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.calls = []

    def _cut(self):
        self.calls.append(self.model.drain())

    def requests(self, reqs, lease=False):
        st = super().requests(reqs, lease)
        self._cut()
        return st

    def acks(self, acks):
        super().acks(acks)
        self._cut()

    def acks_dense(self, cols):
        super().acks_dense(cols)
        self._cut()

    def check_states(self):
        got = self.eng.read_states().tolist()
        calls, self.calls = self.calls, []
        assert_list_order(got, calls)
        return len(got)

    def cols_for(self, ctx_of, slots=None):
        """dense ack columns: the slots of `slots(g)` (default: all) answer ctx_of[g]"""
        cols = np.zeros((self.P, self.eng.stride), dtype=np.uint64)
        for g, c in ctx_of.items():
            for s in (range(self.P) if slots is None else slots(g)):
                cols[s, g] = c
        return cols


def majorities(n, P=3):
    """every group a majority over all P slots, the leader's slot rotating"""
    full = (1 << P) - 1
    return [cfg_make(full, 0, g % P, full) for g in range(n)]


def follower(r, g):
    return (M.cfg_self(int(r.cfg[g])) + 1) % r.P


# ---- A: every kernel instance of rg_with_p, depth 1 and 2 ------------------------------------------------------------------
# (seeds: the model alone shows the statuses below and drains > 300 states in 12 rounds for each of them)
SWEEP = [(1, 1, 301), (2, 1, 302), (2, 2, 303), (4, 1, 304), (6, 2, 305), (8, 1, 306), (8, 2, 307)]


@pytest.mark.parametrize("P,depth,seed", SWEEP)
def test_slot_count_and_depth_sweep(rg, P, depth, seed):
    """The random sequences of test_random_sequences, 12 rounds, over the slot counts and depths nothing else runs. Sparse acks
    name slots 0..8: slots the engine does not have (no configuration word may give them a Progress: rg_load_column and
    rg_set_config refuse such words) and slot 8, which no engine has."""
    r = OrderedRig(rg, P, depth=depth, seed=seed)
    seen, drained, at_depth = random_rounds(r, 12, slot_hi=8)
    assert seen == (ALL5 if P >= 2 else {M.NOT_READY, M.READY}), (P, depth, seen)
    assert drained > 300 and (P == 1 or at_depth > 30), (drained, at_depth)
    r.close()


# ---- B: the whole ring of RG_READ_MAX_DEPTH entries ----------------------------------------------------------------------------
_HANDLES = [U64, 1 << 63, (1 << 63) + 1, (1 << 63) - 1, 1, 2, 1 << 32, (1 << 32) - 1, (1 << 53) + 1, U64 - 1]


def handle(g, j):
    """the j-th context of group g: handles from both ends and the middle of the 64-bit range"""
    return _HANDLES[j] if j < len(_HANDLES) else ((j + 1) * 0x9E3779B97F4A7C15 + g * 0x1000003) & U64


def test_depth_16_ring_fills_wraps_and_drains_in_order(rg):
    P, D = 5, 16
    r = OrderedRig(rg, P, depth=D, seed=16)
    everyone = list(range(G))
    r.tick_advance(everyone)  # every group has committed in its term
    ns = [g for g in everyone if not M.is_singleton(int(r.cfg[g]))]
    even, odd = [g for g in ns if g % 2 == 0], [g for g in ns if g % 2]
    assert len(ns) > 100 and all(len({handle(g, j) for j in range(22)} - {0}) == 22 for g in ns)

    def ask(j, want):
        st = r.requests([(g, handle(g, j)) for g in everyone])
        assert all(st[g] == (want if g in in_ns else M.READY) for g in everyone), (j, want)
        r.check_queues()

    def answer(j, dense, sparse):
        """every slot answers ctx j: the groups of `dense` through rg_read_acks_device, those of `sparse` through rg_read_acks"""
        r.acks_dense(r.cols_for({g: handle(g, j) for g in dense}))
        r.acks([(g, s, handle(g, j), 0) for g in sparse for s in range(P)])
        r.check_queues()

    in_ns = set(ns)
    queued_at = {}
    for j in range(D):
        if j == 8:
            r.tick_advance(everyone)  # (the first fill carries two different indices)
        ask(j, M.QUEUED)
        queued_at[j] = [r.model.groups[g].commit for g in everyone]
    assert r.model.counts() == [D if g in in_ns else 0 for g in everyone]
    ask(16, M.FULL)
    r.check_states()  # (the singletons' states)
    # the 5th-oldest from a quorum: five states per group, oldest first
    answer(4, even, odd)
    assert r.model.counts() == [D - 5 if g in in_ns else 0 for g in everyone]
    want = [(g, handle(g, j), queued_at[j][g]) for g in even for j in range(5)]
    assert r.calls[-2] == want and len(r.calls[-1]) == 5 * len(odd)
    assert r.check_states() == 5 * len(ns)
    # five more: the ring wraps, head is 5 and the queue full again
    r.tick_advance(everyone)
    for j in range(16, 21):
        ask(j, M.QUEUED)
        queued_at[j] = [r.model.groups[g].commit for g in everyone]
    ask(21, M.FULL)
    ask(20, M.DUPLICATE)
    r.check_states()
    # the newest from a quorum: all sixteen, in order, each with the index it was queued with (the halves swap their roads)
    answer(20, odd, even)
    assert r.model.counts() == [0] * G
    want = [(g, handle(g, j), queued_at[j][g]) for g in odd for j in range(5, 21)]
    assert r.calls[-2] == want and len({i for _, _, i in want[:16]}) >= 2
    assert r.check_states() == D * len(ns)
    r.close()


# ---- C: the scan of rg_read_reserve at wave and workgroup boundaries; a list that grows under one lane -------------------------
@pytest.mark.parametrize("n", [1, 64, 65, 255, 256, 257, 513])
def test_scan_edges(rg, n):
    """Group g holds g % 5 pending reads; a follower acks the last of them -- a quorum of the three voters, so all g % 5 come out
    -- in all groups, in the last lane of every wave only, in the first lane of every workgroup only, in the last group only:
    dense (lane = group) and sparse (one record per group, so run i = lane i = group i; the others' records carry no context),
    the sparse records in DESCENDING group order. Then 1 000 LeaseBased requests of one group in one call."""
    r = OrderedRig(rg, 3, depth=4, seed=n, n=n, cfgs=majorities(n))
    everyone = list(range(n))
    r.tick_advance(everyone)
    subsets = {"all": everyone, "last lane of a wave": [g for g in everyone if g % 64 == 63],
               "first lane of a workgroup": [g for g in everyone if g % 256 == 0], "last group": [n - 1]}
    for name, subset in subsets.items():
        for dense in (True, False):
            # top the queues up to g % 5, round-robin over the groups (the library sorts the records by group)
            have = r.model.counts()
            missing = {g: g % 5 - have[g] for g in everyone}
            reqs = [(g, r.fresh_ctx()) for k in range(4) for g in everyone if k < missing[g]]
            assert set(r.requests(reqs)) <= {M.QUEUED}
            assert r.model.counts() == [g % 5 for g in everyone]
            ctx_of = {g: r.model.groups[g].last_pending() for g in subset}
            if dense:
                r.acks_dense(r.cols_for(ctx_of, lambda g: [follower(r, g)]))
            else:
                r.acks([(g, follower(r, g), ctx_of.get(g, 0), 0) for g in reversed(everyone)])
            assert len(r.calls[-1]) == sum(g % 5 for g in subset), (name, dense)
            assert r.model.counts() == [0 if g in ctx_of else g % 5 for g in everyone], (name, dense)
            r.check_queues()
            items, cnt = r.eng.read_states(cap=0)
            assert cnt == sum(g % 5 for g in subset) and not len(items)
            assert r.check_states() == cnt, (name, dense)
    # one lane emits more states than the list holds: 1 000 requests of one group among one request of every other group
    hot = (2 * n) // 3
    others = [g for g in everyone if g != hot]
    reqs = [(hot, r.fresh_ctx()) for _ in range(1000)]
    for k, g in enumerate(others):
        reqs.insert(1 + k * 1000 // len(others) + k, (g, r.fresh_ctx()))
    assert set(r.requests(reqs, lease=True)) == {M.READY}
    got = r.eng.read_states().tolist()
    assert len(got) == 1000 + len(others)
    first = next(i for i, s in enumerate(got) if s[0] == hot)
    commit = r.model.groups[hot].commit
    assert [tuple(s) for s in got[first:first + 1000]] == [(hot, c, commit) for g, c in reqs if g == hot]
    assert_list_order(got, r.calls)
    r.calls = []
    r.check_queues()
    r.close()


# ---- D: the order the header promises, on the raw list ---------------------------------------------------------------------------
def test_list_order_contract(rg):
    """Two calls without a drain between them -- requests (the singletons answer at once), then acks that pop the others:
    every state of the first call precedes every state of the second, and inside each call's part of the list a group's states
    are contiguous and in queue order. Once with dense acks, once with sparse ones given in a shuffled order."""
    P = 5
    r = OrderedRig(rg, P, depth=4, seed=44)
    r.tick_advance(list(range(G)))
    for dense in (True, False):
        reqs = [(g, r.fresh_ctx()) for k in range(4) for g in range(G) if (g + k) % 3]  # two or three per group, interleaved
        st = r.requests(reqs)
        assert set(st) == {M.READY, M.QUEUED}
        call1 = r.calls[-1]
        ctx_of = {g: c for g, c in enumerate(r.model.last_pending()) if c}
        if dense:
            r.acks_dense(r.cols_for(ctx_of))
        else:
            recs = [(g, s, c, 0) for g, c in ctx_of.items() for s in range(P)]
            order = r.rng.permutation(len(recs))
            recs = sorted((recs[i] for i in order), key=lambda a: a[1])  # groups shuffled, a group's slots ascending
            r.acks(recs)
        call2 = r.calls[-1]
        assert len(call1) > 100 and len(call2) > 300 and not (set(call1) & set(call2))
        got = [tuple(int(x) for x in s) for s in r.eng.read_states().tolist()]
        where = {s: i for i, s in enumerate(got)}
        assert len(where) == len(got) == len(call1) + len(call2)
        assert max(where[s] for s in call1) < min(where[s] for s in call2)
        for call in (call1, call2):
            for g in {s[0] for s in call}:
                mine = [s for s in call if s[0] == g]
                assert [where[s] for s in mine] == list(range(where[mine[0]], where[mine[0]] + len(mine))), (dense, g)
        assert_list_order(got, r.calls)
        r.calls = []
        r.check_queues()
    r.close()


# ---- E: the bound that sizes the list --------------------------------------------------------------------------------------------
def test_restore_with_an_undrained_list(rg):
    """rg_restore keeps the undrained list and makes the checkpoint's pending reads pending AGAIN: 600 states sit in the list,
    600 more can follow, and rg_read_states has to deliver all 1 200 (a list sized for fewer would lose states: RG_ERR_STATE)."""
    r = OrderedRig(rg, 3, depth=2, seed=21, cfgs=majorities(G))
    everyone = list(range(G))
    r.tick_advance(everyone)
    reqs = [(g, r.fresh_ctx()) for _ in range(2) for g in everyone]
    assert r.requests(reqs) == [M.QUEUED] * 600
    r.eng.checkpoint()
    saved = copy.deepcopy(r.model.groups)
    r.acks_dense(r.cols_for({g: r.model.groups[g].last_pending() for g in everyone}, lambda g: [follower(r, g)]))
    r.check_queues()
    assert r.model.counts() == [0] * G and len(r.calls[-1]) == 600
    r.eng.restore()
    r.model.groups = saved
    r.sync_log()
    r.check_queues()
    assert r.model.counts() == [2] * G
    r.acks([(g, follower(r, g), r.model.groups[g].last_pending(), 0) for g in everyone])
    r.check_queues()
    items, n = r.eng.read_states(cap=0)
    assert n == 1200
    got = [tuple(int(x) for x in s) for s in r.eng.read_states().tolist()]
    assert len(got) == 1200 and sorted(got) == sorted(r.calls[-1] * 2) and len(set(got)) == 600
    assert_list_order(got, r.calls[-2:])
    r.calls = []
    assert len(r.eng.read_states()) == 0
    r.close()


def test_elections_drop_full_queues_and_free_their_room(rg):
    """Four times: fill every queue, elect every group (RG_MF_BECOME_LEADER: the pending reads are gone, nothing is emitted),
    let the new term's entry commit, and find both places of every queue free again -- answered in order."""
    r = OrderedRig(rg, 3, depth=2, seed=22, cfgs=majorities(G))
    everyone = list(range(G))
    r.tick_advance(everyone)
    for cycle in range(4):
        reqs = [(g, r.fresh_ctx()) for _ in range(2) for g in everyone]
        assert r.requests(reqs) == [M.QUEUED] * 600
        assert r.requests([(g, r.fresh_ctx()) for g in everyone]) == [M.FULL] * G
        r.check_queues()
        if cycle % 2:  # (a half-answered queue: one ack short of a quorum everywhere)
            r.acks([(g, M.cfg_self(int(r.cfg[g])), r.model.groups[g].last_pending(), 0) for g in everyone])
        r.tick_elect(everyone)
        assert r.model.counts() == [0] * G and r.model.last_pending() == [0] * G
        r.check_queues()
        r.check_queues()  # (the reset is stored: the second look finds what the first one left)
        assert r.check_states() == 0
        assert r.requests([(g, r.fresh_ctx()) for g in everyone]) == [M.NOT_READY] * G
        r.tick_advance(everyone)  # the new term's entry commits
        reqs = [(g, r.fresh_ctx()) for _ in range(2) for g in everyone]
        assert r.requests(reqs) == [M.QUEUED] * 600
        r.check_queues()
        if cycle % 2:
            r.acks_dense(r.cols_for({g: r.model.groups[g].last_pending() for g in everyone}, lambda g: [follower(r, g)]))
        else:
            r.acks([(g, follower(r, g), r.model.groups[g].last_pending(), 0) for g in reversed(everyone)])
        assert M.by_group(r.calls[-1]) == [(g, c, r.model.groups[g].commit) for g in everyone for c in (reqs[g][1], reqs[G + g][1])]
        r.check_queues()
        assert r.check_states() == 600
    r.close()
