"""GPU: ReadIndex on the device (rg_read_index / rg_read_acks / rg_read_acks_device / rg_read_states ...) against
tests/readonly_model.py, word for word: request statuses, the stably sorted list of read states, last_pending_request_ctx and
pending_read_count of every group. The model owns the queues; commit / term_lo / the term are read back from the engine's own
columns after every tick (the ticks are not what is under test here)."""
import numpy as np
import pytest

import readonly_model as M

pytestmark = pytest.mark.gpu

G = 300  # past one 256-lane workgroup; stride 512
MF_VALID, MF_BECOME_LEADER, MF_APPEND = 0x01, 0x02, 0x20


def cfg_make(incoming, outgoing, self_slot, present):
    return (incoming & 0xff) | ((outgoing & 0xff) << 8) | ((self_slot & 7) << 16) | ((present & 0xff) << 24)


def mixed_cfgs(rng, n, P):
    """majority, joint, learner-carrying and singleton groups, interleaved (P = 1: singletons, there is nothing else; P = 2: the
    learner-carrying kind is one voter and one learner, a singleton as well)"""
    full = (1 << P) - 1
    out = np.zeros(n, dtype=np.uint32)
    if P == 1:
        out[:] = cfg_make(1, 0, 0, 1)
        return out
    for g in range(n):
        k = g % 4
        if k == 0:  # majority over every slot
            out[g] = cfg_make(full, 0, int(rng.integers(0, P)), full)
        elif k == 1:  # joint: two overlapping majorities
            inc = int(rng.integers(1, full + 1))
            og = int(rng.integers(1, full + 1))
            voters = [s for s in range(P) if ((inc | og) >> s) & 1]
            out[g] = cfg_make(inc, og, int(rng.choice(voters)), full)
        elif k == 2:  # voters + learners (slot P-1 is always a learner)
            inc = int(rng.integers(1, 1 << (P - 1)))
            voters = [s for s in range(P - 1) if (inc >> s) & 1]
            out[g] = cfg_make(inc, 0, int(rng.choice(voters)), full)
        else:  # one voter, the rest learners or absent
            v = int(rng.integers(0, P))
            out[g] = cfg_make(1 << v, 0, v, (1 << v) | int(rng.integers(0, full + 1)))
    return out


class ReadChecker:
    """The read calls of an engine and the model's side by side. Whoever drives the engine keeps the model's groups current
    (cfg / commit / term_lo / set_term) with the state under the queues."""

    def __init__(self, eng, model, rng, P, depth, n):
        self.eng, self.model, self.rng, self.P, self.depth, self.n = eng, model, rng, P, depth, n
        self.next_ctx = 1

    # ---- the calls under test, engine and model side by side ----
    def fresh_ctx(self):
        self.next_ctx += 1
        return self.next_ctx - 1 + (1 << 40)  # (handles are 64-bit: keep some high bits in play)

    def requests(self, reqs, lease=False):
        got = self.eng.read_index(reqs, lease=lease)
        want = self.model.read_index(reqs, lease)
        assert [int(x) for x in got] == want, [(r, int(a), b) for r, a, b in zip(reqs, got, want) if int(a) != b][:5]
        return want

    def acks(self, acks):
        """acks: [(group, slot, ctx, flags)]"""
        self.eng.read_acks([(g, ctx, slot, flags) for g, slot, ctx, flags in acks])
        self.model.read_acks(acks)

    def acks_dense(self, cols):
        import torch
        d = torch.from_numpy(cols.view(np.int64).copy()).cuda()
        torch.cuda.synchronize()
        self.eng.read_acks_device(d.data_ptr())
        self.eng.sync()
        self.model.read_acks_dense(cols)

    def check_queues(self):
        assert [int(x) for x in self.eng.read_last_pending()] == self.model.last_pending()
        assert [int(x) for x in self.eng.read_pending_counts()] == self.model.counts()

    def check_states(self):
        got = self.eng.read_states()
        assert M.by_group(got.tolist()) == M.by_group(self.model.drain())
        return len(got)

    # ---- random traffic ----
    def random_requests(self, n):
        reqs = []
        while len(reqs) < n:
            g = int(self.rng.integers(0, self.n))
            if self.rng.random() < 0.25:  # several records of one group in one batch: [ctx a, ctx a, ctx b]
                a, b = self.fresh_ctx(), self.fresh_ctx()
                reqs += [(g, a), (g, a), (g, b)]
            else:
                pend = [c for c, _, _ in self.model.groups[g].queue()]
                reqs.append((g, int(self.rng.choice(pend)) if pend and self.rng.random() < 0.2 else self.fresh_ctx()))
        return reqs

    def random_ack_ctx(self, g):
        pend = [c for c, _, _ in self.model.groups[g].queue()]
        r = self.rng.random()
        if pend and r < 0.6:
            return pend[-1]  # what a follower answers: the last pending ctx its heartbeat carried
        if pend and r < 0.8:
            return int(self.rng.choice(pend))
        return 0 if r < 0.9 else self.fresh_ctx()  # no context / one that is not pending

    def random_sparse_acks(self, n, slot_hi=None):
        """slots 0 .. slot_hi (default P: not a slot of the engine; up to 8: not a slot of any engine)"""
        out = []
        for _ in range(n):
            g = int(self.rng.integers(0, self.n))
            out.append((g, int(self.rng.integers(0, (self.P if slot_hi is None else slot_hi) + 1)), self.random_ack_ctx(g), 0))
        return out

    def random_dense_cols(self, fill):
        cols = np.zeros((self.P, self.eng.stride), dtype=np.uint64)
        for g in range(self.n):
            for s in range(self.P):
                if self.rng.random() < fill:
                    cols[s, g] = self.random_ack_ctx(g)
        return cols


class Rig(ReadChecker):
    """An engine with clean leaders (every Progress caught up, Replicate) and the model next to it."""

    def __init__(self, rg, P, depth, seed, n=G, enable=True, cfgs=None, flags=None):
        self.rg, self.P, self.depth, self.n = rg, P, depth, n
        self.rng = np.random.default_rng(seed)
        self.eng = eng = rg.Engine(n, P, flags=flags)
        stride = eng.stride
        self.cfg = mixed_cfgs(self.rng, n, P) if cfgs is None else np.array(cfgs, dtype=np.uint32)
        last = self.rng.integers(5, 50, size=n).astype(np.uint64)
        cols = np.zeros((P, stride), dtype=np.uint64)
        cols[:, :n] = last
        eng.load_column(rg.COL.MATCH, cols)
        eng.load_column(rg.COL.PR_COMMIT, cols)
        cols[:, :n] = last + 1
        eng.load_column(rg.COL.NEXT, cols)
        zero = np.zeros((P, stride), dtype=np.uint64)
        for c in (rg.COL.PEND_SNAP, rg.COL.PEND_RS, rg.COL.GID):
            eng.load_column(c, zero)
        pf = np.zeros((n, 8), dtype=np.uint8)
        pf[:, :P] = 1 | 8  # Replicate, recent_active
        eng.load_column(rg.COL.PFLAGS, pf)
        eng.load_column(rg.COL.COMMIT, last)
        lo = (last - np.minimum(self.rng.integers(0, 4, size=n).astype(np.uint64), last - 1)).astype(np.uint64)
        lo = np.where(self.rng.random(n) < 0.15, last + 1, lo).astype(np.uint64)  # nothing of the leader's term committed yet
        eng.load_column(rg.COL.TERM_LO, lo)
        eng.load_column(rg.COL.TERM_HI, last)
        eng.load_column(rg.COL.CFG, self.cfg)
        eng.load_column(rg.COL.CUR_TERM, np.full(n, 2, dtype=np.uint64))
        eng.load_column(rg.COL.DUMMY_INDEX, np.zeros(n, dtype=np.uint64))
        eng.load_column(rg.COL.DUMMY_TERM, np.zeros(n, dtype=np.uint64))
        self.model = M.Shard(self.cfg, depth)
        for g in self.model.groups:
            g.term = 2
        self.next_ctx = 1
        self.msgs = rg.MsgBuffers(n, P, stride)
        self.keep = []
        if enable:
            eng.read_index_enable(depth)
        self.sync_log()

    def close(self):
        self.eng.sync()
        self.eng.close()

    # ---- the state under the queues: read back from the engine's columns ----
    def sync_log(self):
        rg = self.rg
        commit, lo, term = (self.eng.read_column(c) for c in (rg.COL.COMMIT, rg.COL.TERM_LO, rg.COL.CUR_TERM))
        for g, grp in enumerate(self.model.groups):
            grp.commit, grp.term_lo = int(commit[g]), int(lo[g])
            grp.set_term(int(term[g]))

    def tick_advance(self, groups):
        """the leaders of `groups` append 1..3 entries and persist them; then every peer acks the new last index"""
        m, rg = self.msgs, self.rg
        hi = self.eng.read_column(rg.COL.TERM_HI)
        new_last = hi.copy()
        m.clear()
        for g in groups:
            s = M.cfg_self(int(self.cfg[g]))
            new_last[g] = hi[g] + np.uint64(self.rng.integers(1, 4))
            m.m_flags[g, s] = MF_VALID | MF_APPEND
            m.m_index[s, g] = new_last[g]
            m.m_commit[s, g] = new_last[g]
        self.eng.tick(m)
        m.clear()
        for g in groups:
            for s in M.cfg_present(int(self.cfg[g])):
                if s != M.cfg_self(int(self.cfg[g])) and s < self.P:
                    m.m_flags[g, s] = MF_VALID
                    m.m_index[s, g] = new_last[g]
        self.eng.tick(m)
        self.sync_log()

    def tick_elect(self, groups):
        """RG_MF_BECOME_LEADER at the next term: Raft::reset drops the pending reads -- lazily, on the device"""
        m, rg = self.msgs, self.rg
        term, hi, match = (self.eng.read_column(c) for c in (rg.COL.CUR_TERM, rg.COL.TERM_HI, rg.COL.MATCH))
        # (become_leader asserts persisted == last_index, raft.rs:1170: a leader elected twice has to persist its empty entry between)
        groups = [g for g in groups if match[M.cfg_self(int(self.cfg[g])), g] == hi[g]]
        assert groups
        m.clear()
        for g in groups:
            s = M.cfg_self(int(self.cfg[g]))
            m.m_flags[g, s] = MF_BECOME_LEADER
            m.m_hint[s, g] = term[g] + np.uint64(1)
        self.eng.tick(m)
        out = self.eng.read_column(rg.COL.OUT)
        assert all(out[g] & 0x10 for g in groups), "the elections of the scenario are well-formed"
        self.sync_log()

    def set_config(self, g, word, recheck=True):
        self.eng.set_config(g, int(word))
        self.cfg[g] = word
        self.model.groups[g].cfg = int(word)
        if recheck:  # post_conf_change
            self.acks([(g, 0, 0, M.ACK_LAST_SELF)])


def random_rounds(r, rounds, slot_hi=None):
    """Rounds of request batches, sparse and dense acks, ticks that move commit, rg_set_config + re-check and elections, every
    call checked against the model -> (statuses seen, states drained, queues found at their depth after a round)."""
    rng, P, n = r.rng, r.P, r.n
    seen, drained, at_depth = set(), 0, 0
    for rnd in range(rounds):
        seen |= set(r.requests(r.random_requests(120), lease=(rnd % 10 == 9)))
        r.check_queues()
        if rnd % 3 != 2:
            r.acks(r.random_sparse_acks(200, slot_hi))
        else:
            r.acks_dense(r.random_dense_cols(0.5))
        r.check_queues()
        if rnd % 2 == 0:
            r.tick_advance([int(g) for g in rng.choice(n, size=60, replace=False)])
        if rnd % 4 == 1:
            for g in rng.choice(n, size=6, replace=False):
                g = int(g)
                full = (1 << P) - 1
                c = int(r.cfg[g])
                s = M.cfg_self(c)
                # the quorum shrinks (leave joint, drop voters down to the leader) or the membership is redrawn
                word = cfg_make(1 << s, 0, s, (c >> 24) & 0xff) if rng.random() < 0.5 else \
                    cfg_make(int(rng.integers(0, full + 1)) | (1 << s), int(rng.integers(0, full + 1)) if rng.random() < 0.4 else 0, s, full)
                if P == 1:
                    word &= ~0xff00  # (one slot: every group stays a singleton, never a joint configuration of that one voter)
                r.set_config(g, word)
        if rnd % 5 == 3:
            r.tick_elect([int(g) for g in rng.choice(n, size=25, replace=False)])
        r.check_queues()
        at_depth += sum(1 for grp in r.model.groups if grp.read_only.pending_read_count() == r.depth)
        if rnd % 4 == 3 or rnd == rounds - 1:
            drained += r.check_states()
    return seen, drained, at_depth


@pytest.mark.parametrize("P", [3, 5, 7])
def test_random_sequences(rg, P):
    """40 rounds of request batches, sparse and dense acks, ticks that move commit, rg_set_config + re-check and elections, at
    depth 2 (FULL and ring wrap-around both occur)."""
    r = Rig(rg, P, depth=2, seed=100 + P)
    seen, drained, at_depth = random_rounds(r, 40)
    assert seen == {M.NOT_READY, M.READY, M.QUEUED, M.DUPLICATE, M.FULL}
    assert drained > 1000 and at_depth > 100  # (queues that stay full while their head moves: the ring wraps)
    r.close()


def test_dense_acks_equal_sparse_acks(rg):
    """The same acks through rg_read_acks_device and through rg_read_acks (slot-ascending per group) leave identical queues
    and identical state lists."""
    P = 5
    a, b = Rig(rg, P, depth=4, seed=7), Rig(rg, P, depth=4, seed=7)
    for rnd in range(6):
        reqs = a.random_requests(250)  # (rig a draws the traffic, rig b replays it)
        assert a.requests(reqs) == b.requests(reqs)
        cols = a.random_dense_cols(0.4)
        a.acks_dense(cols)
        b.acks([(g, s, int(cols[s, g]), 0) for g in range(G) for s in range(P) if cols[s, g]])
        for x in (a, b):
            x.check_queues()
        assert (a.eng.read_last_pending() == b.eng.read_last_pending()).all()
        assert (a.eng.read_pending_counts() == b.eng.read_pending_counts()).all()
        sa, sb = a.eng.read_states(), b.eng.read_states()
        assert len(sa) > 50 and M.by_group(sa.tolist()) == M.by_group(sb.tolist()) == M.by_group(a.model.drain())
        b.model.drain()
    a.close()
    b.close()


def test_drain_semantics_and_list_growth(rg):
    """States accumulate across calls; a drain with cap < n writes cap items, reports n and empties the list; the list grows
    past its initial capacity (256 states) when 3 x G requests are answered before any drain, and every one is reported."""
    r = Rig(rg, 3, depth=2, seed=5)
    r.tick_advance(list(range(G)))  # every group has committed in its term: nothing is NOT_READY
    want = []
    for k in range(3):  # LeaseBased answers every request at once: 3 x G = 900 states before any drain
        reqs = [(g, r.fresh_ctx()) for g in range(G)]
        assert set(r.requests(reqs, lease=True)) == {M.READY}
        want += [(g, c, r.model.groups[g].commit) for g, c in reqs]
    items, n = r.eng.read_states(cap=0)
    assert n == 3 * G and len(items) == 0  # cap = 0 only counts
    got = r.eng.read_states()
    assert len(got) == 3 * G and M.by_group(got.tolist()) == M.by_group(want) == M.by_group(r.model.drain())
    assert len(r.eng.read_states()) == 0
    # a short array: cap items written, n reported, everything drained
    reqs = [(g, r.fresh_ctx()) for g in range(40)]
    r.requests(reqs, lease=True)
    r.requests([(g, r.fresh_ctx()) for g in range(40, 50)], lease=True)
    items, n = r.eng.read_states(cap=16)
    assert n == 50 and len(items) == 16
    first = {tuple(int(x) for x in it) for it in items.tolist()}
    assert len(first) == 16 and first <= set(r.model.drain())
    items, n = r.eng.read_states(cap=16)
    assert n == 0 and len(items) == 0
    # queued reads answered later land behind what is already in the list
    safe = [g for g in range(G) if not M.is_singleton(int(r.cfg[g]))][:30]
    assert set(r.requests([(g, r.fresh_ctx()) for g in safe])) == {M.QUEUED}
    r.requests([(g, r.fresh_ctx()) for g in range(5)], lease=True)
    cols = np.zeros((3, r.eng.stride), dtype=np.uint64)
    for g in safe:
        cols[:, g] = r.model.groups[g].last_pending()
    r.acks_dense(cols)
    r.check_queues()
    assert r.check_states() >= 5 + len([g for g in safe if r.model.groups[g].read_only.pending_read_count() == 0])
    r.close()


def test_queues_travel_with_checkpoint_restore_and_permute(rg):
    P = 5
    r = Rig(rg, P, depth=4, seed=9)
    r.tick_advance(list(range(G)))
    r.requests(r.random_requests(400))
    r.acks(r.random_sparse_acks(150))
    r.check_queues()
    r.check_states()
    r.eng.checkpoint()
    import copy
    saved = copy.deepcopy(r.model.groups)
    # diverge: more requests, acks that empty queues, an election
    r.requests(r.random_requests(200))
    r.acks_dense(r.random_dense_cols(0.9))
    r.tick_elect(list(range(0, G, 7)))
    r.check_queues()
    r.check_states()
    r.eng.restore()
    r.model.groups = saved
    r.sync_log()
    r.check_queues()
    assert sum(r.model.counts()) > 100
    # a non-trivial permutation: the queues follow their groups (and their logs, which the tick needs)
    perm = r.rng.permutation(G).astype(np.uint64)
    r.eng.permute_groups(perm)
    r.model.groups = [r.model.groups[int(perm[i])] for i in range(G)]
    r.cfg = r.cfg[perm.astype(np.int64)]
    r.check_queues()
    cols = np.zeros((P, r.eng.stride), dtype=np.uint64)
    for g in range(G):
        cols[:, g] = r.model.groups[g].last_pending()
    r.acks_dense(cols)  # every follower answers the last pending ctx: whatever has a quorum at all drains
    r.check_queues()
    assert r.check_states() > 100
    # ... and a restore WITHOUT a checkpoint of the new placement is refused by the engine (the old image was dropped)
    with pytest.raises(rg.EngineError):
        r.eng.restore()
    r.close()


def test_not_enabled_is_a_state_error(rg):
    import ctypes as C
    r = Rig(rg, 3, depth=2, seed=1, n=64, enable=False)
    eng, L = r.eng, r.eng.L
    buf = np.zeros(3 * eng.stride, dtype=np.uint64)
    req = np.array([(0, 1)], dtype=rg.engine.READ_REQ_DTYPE)
    ack = np.array([(0, 1, 0, 0)], dtype=rg.engine.READ_ACK_DTYPE)
    n = C.c_uint64(0)
    calls = {
        "rg_read_index": lambda: L.rg_read_index(eng.h, req.ctypes.data, 1, 0, buf.ctypes.data),
        "rg_read_acks": lambda: L.rg_read_acks(eng.h, ack.ctypes.data, 1),
        "rg_read_acks_device": lambda: L.rg_read_acks_device(eng.h, buf.ctypes.data),  # (refused before the pointer is looked at)
        "rg_read_states": lambda: L.rg_read_states(eng.h, buf.ctypes.data, 1, C.byref(n)),
        "rg_read_last_pending": lambda: L.rg_read_last_pending(eng.h, None, buf.ctypes.data),
        "rg_read_pending_counts": lambda: L.rg_read_pending_counts(eng.h, buf.ctypes.data),
    }
    for name, call in calls.items():
        assert call() == -8, name  # RG_ERR_STATE
        assert name in L.rg_last_error().decode() and "rg_read_index_enable" in L.rg_last_error().decode()
    with pytest.raises(rg.EngineError) as ei:
        eng.read_index_enable(17)
    assert ei.value.code == -1
    eng.read_index_enable(2)
    with pytest.raises(rg.EngineError) as ei:
        eng.read_index_enable(2)
    assert ei.value.code == -8
    with pytest.raises(rg.EngineError) as ei:
        eng.read_index([(0, 0)])  # ctx 0 is the empty context
    assert ei.value.code == -1
    with pytest.raises(rg.EngineError) as ei:
        eng.read_index([(64, 5)])
    assert ei.value.code == -1
    r.close()
