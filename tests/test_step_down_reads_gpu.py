"""GPU: a group's pending reads across the check-quorum step-down. become_follower(term, INVALID_ID) runs Raft::reset at the
UNCHANGED term, and reset replaces the ReadOnly unconditionally (raft.rs:957): once the rgx_lead_clock call that reports
STEPPED_DOWN has run, in stream order, every ReadIndex entry point finds that group's queue empty and emits nothing for it, while
the groups that stayed leaders -- in the same waves -- keep theirs. Against tests/readonly_model.py composed with
tests/lead_clock_model.py (tick(c, g, read_only)): every group's event byte, clock cells, cfg word and flag row, pending count,
last pending context, and the raw drained list, with sentinels around every output buffer. No test provokes a device fault: every
bad argument used is one the host refuses."""
import copy
import ctypes as C
import random

import numpy as np
import pytest

import lead_clock_model as L
import readonly_model as M
from test_read_index_edges_gpu import OrderedRig, assert_list_order

pytestmark = pytest.mark.gpu

CLOCK = L.Config(2, 1, L.CHECK_QUORUM)  # the first call beats, the second is the election timeout
SHAPES = {3: 300, 8: 70}                # a full block plus a partial one; one partial block
EDGE_LANES = {300: (0, 63, 64, 255, 256, 299), 70: (0, 63, 64, 69)}  # steppers at the ends of waves and blocks, quorate neighbours
EV_SENT, U64_SENT = 0xEE, 0xA5A5A5A5A5A5A5A5
DOWN = L.EV_CHECK_QUORUM | L.EV_STEPPED_DOWN


def layout(P, seed):
    """-> [(cfg word, flag row)] per group: the model's edge shapes in every third lane, all-voter groups with a random leader
    slot and random flag bytes between them; the lanes of EDGE_LANES lose their quorum (nobody recent_active, the leader in slot
    0, a clean Replicate row a later election can run on), the lanes next to them keep it."""
    G, rng = SHAPES[P], random.Random(seed)
    edges = list(L.edge_groups(P).values())
    out = []
    for g in range(G):
        if g % 3 == 2:
            cfg, pf = edges[(g // 3) % len(edges)]
        else:
            cfg, pf = L.cfg_word(range(P), self_slot=rng.randrange(P)), [rng.randrange(256) if s < P else 0 for s in range(8)]
        out.append((cfg, [b if s < P else 0 for s, b in enumerate(pf)]))
    for g in EDGE_LANES[G]:
        out[g] = (L.cfg_word(range(P), self_slot=0), [1 if s < P else 0 for s in range(8)])
        for n in (g - 1, g + 1):
            if 0 <= n < G and n not in EDGE_LANES[G]:
                out[n] = (L.cfg_word(range(P), self_slot=0), [1 | L.PF_RECENT_ACTIVE if s < P else 0 for s in range(8)])
    return out


class StepRig(OrderedRig):
    """The ReadIndex rig (clean leaders of term 2, the model's queues next to them) with the leader's clock on top: every group
    led, both counters 0. order: which layer is enabled first; "clock_only": no ReadIndex layer at all."""

    def __init__(self, rg, P, depth, ix64=False, order="read_first", seed=11):
        lay = layout(P, seed)
        E = rg.engine
        super().__init__(rg, P, depth=depth, seed=seed, n=SHAPES[P], enable=False, cfgs=[c for c, _ in lay], flags=E.CFGF.IX64 if ix64 else None)
        eng, n = self.eng, self.n
        assert eng.device_info()["last_tick_offset_bits"] in (0, 64 if ix64 else 32)
        eng.load_column(rg.COL.PFLAGS, np.array([p for _, p in lay], dtype=np.uint8))
        eng.load_column(rg.COL.TERM_LO, np.ones(n, dtype=np.uint64))  # every group has committed in its term: nothing is NOT_READY
        if order == "read_first":
            eng.read_index_enable(depth)
        eng.lead_clock_enable(CLOCK.election_tick, CLOCK.heartbeat_tick, CLOCK.flags | L.START_LED)
        if order == "clock_first":
            eng.read_index_enable(depth)
        self.reads = order != "clock_only"
        self.sync_log()
        cfg, pf = eng.read_column(rg.COL.CFG), eng.read_column(rg.COL.PFLAGS)  # (the engine keeps its own bits of a loaded flag row exact)
        self.clock = [L.new_group(P, int(cfg[g]), cur_term=2, pflags=[int(b) for b in pf[g]]) for g in range(n)]
        self.forced = EDGE_LANES[n]

    # ---- the read calls, with sentinels around every output buffer ----
    def requests(self, reqs, lease=False):
        eng = self.eng
        a = np.ascontiguousarray(np.array(reqs, dtype=self.rg.engine.READ_REQ_DTYPE))
        st = np.full(len(a) + 16, EV_SENT, dtype=np.uint8)
        eng._check(eng.L.rg_read_index(eng.h, a.ctypes.data, len(a), 0, st[8:].ctypes.data))
        assert (st[:8] == EV_SENT).all() and (st[8 + len(a):] == EV_SENT).all()
        want = self.model.read_index(reqs, lease)
        assert [int(x) for x in st[8:8 + len(a)]] == want, [(r, int(x), w) for r, x, w in zip(reqs, st[8:], want) if int(x) != w][:5]
        self._cut()
        return want

    def pending(self):
        """(last pending ctx, pending count) of every group, as the engine reports them"""
        eng, n = self.eng, self.n
        ctx, cnt = np.full(n + 8, U64_SENT, dtype=np.uint64), np.full(n + 16, EV_SENT, dtype=np.uint8)
        eng._check(eng.L.rg_read_last_pending(eng.h, None, ctx[4:].ctypes.data))
        eng._check(eng.L.rg_read_pending_counts(eng.h, cnt[8:].ctypes.data))
        assert (ctx[:4] == U64_SENT).all() and (ctx[4 + n:] == U64_SENT).all() and (cnt[:8] == EV_SENT).all() and (cnt[8 + n:] == EV_SENT).all()
        return [int(x) for x in ctx[4:4 + n]], [int(x) for x in cnt[8:8 + n]]

    def check_queues(self):
        last, counts = self.pending()
        assert last == self.model.last_pending(), [(g, a, b) for g, (a, b) in enumerate(zip(last, self.model.last_pending())) if a != b][:5]
        assert counts == self.model.counts(), [(g, a, b) for g, (a, b) in enumerate(zip(counts, self.model.counts())) if a != b][:5]

    def check_states(self):
        """Drain the list into an array of exactly its size between two sentinel items; compare it RAW with what the model emitted,
        call by call. -> the states"""
        eng = self.eng
        n, m = C.c_uint64(0), C.c_uint64(0)
        eng._check(eng.L.rg_read_states(eng.h, None, 0, C.byref(n)))
        items = np.zeros(n.value + 2, dtype=self.rg.engine.READ_STATE_DTYPE)
        items.view(np.uint8)[:] = 0xA5
        if n.value:
            eng._check(eng.L.rg_read_states(eng.h, items[1:].ctypes.data, n.value, C.byref(m)))
            assert m.value == n.value
        assert (items[:1].view(np.uint8) == 0xA5).all() and (items[-1:].view(np.uint8) == 0xA5).all()
        got = [tuple(int(x) for x in s) for s in items[1:1 + n.value].tolist()]
        calls, self.calls = self.calls, []
        assert_list_order(got, calls)
        return got

    # ---- the clock ----
    def clock_call(self, sync=True):
        """One rgx_lead_clock, the model's tick next to it (a step-down resets the group's read-only model). -> what verify() needs"""
        import torch
        want = [L.tick(CLOCK, g, ro if self.reads else None) for g, ro in zip(self.clock, self.model.groups)]
        events = torch.full((self.eng.stride,), EV_SENT, dtype=torch.uint8, device="cuda")
        down = torch.full((self.n + 3,), U64_SENT - (1 << 64), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        counts = self.eng.lead_clock(events, None, 0, down, self.n, None, sync=sync)
        return events, down, want, counts

    def verify(self, call):
        """(after a synchronisation) the event column, the step-down list and the counts of one call"""
        events, down, want, counts = call
        ev = events.cpu().numpy()
        assert [int(x) for x in ev[:self.n]] == want, [(i, int(ev[i]), w) for i, w in enumerate(want) if int(ev[i]) != w][:5]
        assert (ev[self.n:] == EV_SENT).all()
        downs = [i for i, e in enumerate(want) if e & L.EV_STEPPED_DOWN]
        lst = down.cpu().numpy().view(np.uint64)
        assert sorted(int(x) for x in lst[:len(downs)]) == downs and (lst[len(downs):] == U64_SENT).all()
        if counts is not None:
            assert counts == (sum(1 for e in want if e & L.EV_BEAT), sum(1 for e in want if e & L.EV_CHECK_QUORUM), len(downs),
                              sum(1 for e in want if e & L.EV_TRANSFER_ABORTED))
        return want

    def check_cells(self):
        """The clock cells, RG_COL_CFG and RG_COL_PFLAGS against the clock model; the read model takes the cfg words over (a
        step-down clears the TRANSFEREE bits)."""
        got = self.eng.lead_clock_read(np.arange(self.n, dtype=np.uint64))
        for i, (r, g) in enumerate(zip(got, self.clock)):
            assert (int(r["term"]), int(r["election_elapsed"]), int(r["heartbeat_elapsed"]), int(r["led"])) == (g["tag"], g["el"], g["hb"], int(g["led"])), (i, r, g)
        cfg, pf = self.eng.read_column(self.rg.COL.CFG), self.eng.read_column(self.rg.COL.PFLAGS)
        assert [int(x) for x in cfg] == [g["cfg"] for g in self.clock]
        assert [[int(b) for b in row] for row in pf] == [g["pflags"] for g in self.clock]
        for i, g in enumerate(self.clock):
            self.cfg[i] = self.model.groups[i].cfg = g["cfg"]

    def to_the_step_down(self):
        """Two synchronous calls: everybody beats, then the election timeout. -> (steppers, stayers)"""
        self.verify(self.clock_call())
        return self.verify_step_down(self.clock_call())

    def verify_step_down(self, call):
        """... and what the layout promises: the lanes of EDGE_LANES stepped down, their neighbours did not, and every wave holds
        both kinds. -> (steppers, stayers)"""
        want = self.verify(call)
        self.check_cells()
        steppers = [g for g, e in enumerate(want) if e & L.EV_STEPPED_DOWN]
        assert all(want[g] == DOWN for g in steppers) and set(self.forced) <= set(steppers)
        assert all(not want[n] & L.EV_STEPPED_DOWN for g in self.forced for n in (g - 1, g + 1) if 0 <= n < self.n and n not in self.forced)
        for w in range(0, self.n, 64):
            kinds = {bool(want[g] & L.EV_STEPPED_DOWN) for g in range(w, min(w + 64, self.n))}
            assert kinds == {True, False}, w
        return steppers, [g for g in range(self.n) if g not in steppers]

    # ---- the scenario's pieces ----
    def fill(self):
        """Queues of 0, 1, depth-1 and depth reads (the lanes of EDGE_LANES: full, empty, depth-1, full, 1, full), asked for round
        robin; then all slots but the last answer the OLDEST read of every other group of four -- a quorum in most of them: states
        emitted BEFORE the step-down, and queues whose head has moved. -> {group: [contexts pending now]}"""
        d = self.depth
        sizes = [(0, 1, d - 1, d)[g % 4] for g in range(self.n)]
        for k, g in enumerate(self.forced):
            sizes[g] = (d, 0, d - 1, d, 1, d)[k]
        st = self.requests([(g, self.fresh_ctx()) for k in range(d) for g in range(self.n) if k < sizes[g]])
        assert set(st) == {M.QUEUED, M.READY}
        heads = [(g, q[0][0]) for g, q in ((g, self.model.groups[g].queue()) for g in range(self.n)) if q and g % 8 >= 4 and g not in self.forced]
        self.acks([(g, s, ctx, 0) for g, ctx in heads for s in range(self.P - 1)])
        assert len(self.calls[-1]) > self.n // 16
        self.check_queues()
        counts = self.model.counts()
        assert {counts[g] for g in self.forced} >= {0, d} and {0, 1, d - 1, d} <= set(counts)
        return {g: [c for c, _, _ in self.model.groups[g].queue()] for g in range(self.n) if counts[g]}

    def adopt(self):
        """What a tick did to the columns the clock reads is the tick's business: the clock model takes them over."""
        cfg, pf, term = (self.eng.read_column(c) for c in (self.rg.COL.CFG, self.rg.COL.PFLAGS, self.rg.COL.CUR_TERM))
        for i, g in enumerate(self.clock):
            g["cfg"], g["pflags"], g["cur_term"] = int(cfg[i]), [int(b) for b in pf[i]], int(term[i])

    def quorum_cols(self, pend):
        """dense ack columns: every slot answers the NEWEST context of `pend` -- a quorum for it releases the whole queue"""
        return self.cols_for({g: ctxs[-1] for g, ctxs in pend.items()})

    def late_acks(self, pend, dense, recheck=()):
        """The acks that would have formed a quorum for everything in `pend`, through rg_read_acks_device (the newest context from
        every slot) or rg_read_acks (every context from every slot, newest first; then post_conf_change's re-check for the groups
        of `recheck`). -> the states drained"""
        if dense:
            self.acks_dense(self.quorum_cols(pend))
        else:
            self.acks([(g, s, ctx, 0) for g, ctxs in pend.items() for ctx in reversed(ctxs) for s in range(self.P)] + [(g, 0, 0, M.ACK_LAST_SELF) for g in recheck])
        self.check_queues()
        return self.check_states()

    def save(self):
        self.eng.checkpoint()
        return copy.deepcopy((self.model.groups, self.clock, self.cfg))

    def load(self, saved):
        self.eng.restore()
        self.model.groups, self.clock, self.cfg = copy.deepcopy(saved)


def no_state_of(states, groups):
    hit = {s[0] for s in states} & set(groups)
    assert not hit, sorted(hit)[:8]


def releasable(r, pend, groups):
    """the groups of `groups` whose pending reads a quorum of acks would release (from a copy of the model)"""
    out = []
    for g in groups:
        if g in pend:
            ro = copy.deepcopy(r.model.groups[g])
            if any(ro.ack(s, pend[g][-1]) for s in range(r.P)):
                out.append(g)
    return out


def stepper_contexts(pend, steppers):
    return {c for g in steppers for c in pend.get(g, ())}


@pytest.mark.parametrize("depth", [1, 2, 16])
@pytest.mark.parametrize("P,ix64", [(3, False), (8, True)])
def test_a_step_down_drops_the_pending_reads(rg, P, ix64, depth):
    """Queue reads, tick to the step-down. After the call that reports STEPPED_DOWN every stepper has pending count 0 and last
    pending context 0, rg_read_states drains exactly what was emitted before, and the late acks of a quorum -- sparse, then dense
    from the same checkpoint -- release nothing for a stepper and exactly the model's states, in the model's order, for everybody
    else. Restored WITHOUT the step-down the queue and the led cell are back, and the same acks release the steppers' reads too."""
    r = StepRig(rg, P, depth, ix64)
    pend = r.fill()
    saved = r.save()
    would = set(releasable(r, pend, range(r.n)))
    emitted_before = [s for c in r.calls for s in c]
    assert emitted_before
    for dense in (False, True):
        steppers, stayers = r.to_the_step_down()
        assert set(steppers) & would and set(stayers) & would and {len(pend.get(g, ())) for g in steppers} >= {0, 1, depth - 1, depth}
        # ---- after the call that reports STEPPED_DOWN ----
        last, counts = r.pending()
        assert all(counts[g] == 0 for g in steppers), [(g, counts[g]) for g in steppers if counts[g]][:8]
        assert all(last[g] == 0 for g in steppers), [(g, last[g]) for g in steppers if last[g]][:8]
        r.check_queues()
        r.check_queues()  # (the reset is stored: the second look finds what the first one left)
        assert sorted(r.check_states()) == sorted(emitted_before)  # exactly what was emitted before the step-down (the list survives a restore)
        emitted_before = []
        # ---- late acks ----
        states = r.late_acks(pend, dense, recheck=steppers)
        no_state_of(states, steppers)
        assert {s[0] for s in states} == would - set(steppers)
        assert not any(r.model.counts()[g] for g in steppers)
        r.check_cells()  # (no read call moved a clock cell, a cfg word or a flag byte)
        # ---- back to the checkpoint: the queue and the led cell are back ----
        r.load(saved)
        r.check_cells()
        assert all(g["led"] for g in r.clock)
        r.check_queues()
        assert {g: [c for c, _, _ in r.model.groups[g].queue()] for g in pend} == pend
        assert r.check_states() == []
    states = r.late_acks(pend, True)  # ... and without the step-down the acks release the model's states, the steppers' included
    assert {s[0] for s in states} == would and {s[1] for s in states} & stepper_contexts(pend, steppers)
    r.close()


@pytest.mark.parametrize("P,ix64,depth", [(3, False, 2), (8, True, 16)])
def test_the_asynchronous_form_drops_them_in_stream_order(rg, P, ix64, depth):
    """rgx_lead_clock(..., host_counts = NULL) twice, rg_read_acks_device behind them, ONE synchronisation at the end: the acks find
    the steppers' queues empty although no host call stood between the step-down and them."""
    import torch
    r = StepRig(rg, P, depth, ix64)
    pend = r.fill()
    would = set(releasable(r, pend, range(r.n)))
    cols = r.quorum_cols(pend)
    d_cols = torch.from_numpy(cols.view(np.int64).copy()).cuda()
    first, second = r.clock_call(sync=False), r.clock_call(sync=False)
    assert first[3] is None and second[3] is None
    r.eng.read_acks_device(d_cols.data_ptr())
    r.eng.sync()
    r.model.read_acks_dense(cols)
    r._cut()
    r.verify(first)
    steppers, stayers = r.verify_step_down(second)
    last, counts = r.pending()
    assert not any(counts[g] or last[g] for g in steppers)
    r.check_queues()
    states = r.check_states()
    assert not {s[1] for s in states} & stepper_contexts(pend, steppers)
    assert {s[0] for s in states if s[1] in stepper_contexts(pend, stayers)} == would - set(steppers)
    r.close()


@pytest.mark.parametrize("depth", [1, 2, 16])
def test_a_stepper_with_a_full_queue_has_its_room_back(rg, depth):
    """Twice: the steppers of EDGE_LANES fill their queues and step down, then take RG_MF_BECOME_LEADER at the next term in a tick
    (an engine without the arena): nothing is emitted, the clock reports NEW_TERM with counters (1, 1) (the heartbeat counter
    wraps at once under heartbeat_tick 1), and once the new term's entry has committed each of them accepts `depth` new reads and
    refuses one more; a quorum's acks release all of them, in order. The second time the queue's term stamp is the new term's, and
    the step-down has to be stamped over it. The list's capacity bookkeeping holds through it: every drain is exact."""
    r = StepRig(rg, 3, depth)
    chosen = list(r.forced)
    pend = r.fill()
    for cycle in range(2):
        for _ in range(4):  # (the second leadership: the peers acked once, so the first check passes and the next one fails)
            r.verify(r.clock_call())
            r.check_cells()
            if not any(r.clock[g]["led"] for g in chosen):
                break
        assert not any(r.clock[g]["led"] for g in chosen)
        if cycle:  # (the first time nobody looks at the queues between the step-down and the election)
            last, counts = r.pending()
            assert not any(counts[g] or last[g] for g in chosen)
            r.check_queues()
        term = r.eng.read_column(rg.COL.CUR_TERM)
        r.tick_elect(chosen)
        assert all(int(t) == int(term[g]) + 1 for g, t in ((g, r.eng.read_column(rg.COL.CUR_TERM)[g]) for g in chosen))
        r.adopt()
        want = r.verify(r.clock_call())
        r.check_cells()
        assert all(want[g] == L.EV_NEW_TERM | L.EV_BEAT and r.clock[g]["led"] and (r.clock[g]["hb"], r.clock[g]["el"]) == (0, 1) for g in chosen)
        r.check_queues()
        assert not any(r.model.counts()[g] for g in chosen)
        r.check_states()
        assert r.requests([(g, r.fresh_ctx()) for g in chosen]) == [M.NOT_READY] * len(chosen)
        r.tick_advance(chosen)  # the new term's entry commits
        r.adopt()
        reqs = [(g, r.fresh_ctx()) for _ in range(depth) for g in chosen]
        assert r.requests(reqs) == [M.QUEUED] * len(reqs)
        assert r.requests([(g, r.fresh_ctx()) for g in chosen]) == [M.FULL] * len(chosen)
        r.check_queues()
        assert r.eng.read_states(cap=0)[1] == 0
        if cycle == 0:
            continue  # ... the full queues of the second leadership are the ones the second step-down drops
        fresh = {g: [c for c, _, _ in r.model.groups[g].queue()] for g in chosen}
        states = r.late_acks(fresh, dense=False)
        assert M.by_group(states) == [(g, c, r.model.groups[g].commit) for g in sorted(chosen) for c in fresh[g]]
    states = r.late_acks(pend, dense=True)  # the first fill's reads: what a group that is still a leader holds of them comes out, exactly
    no_state_of(states, chosen)
    r.close()


def test_the_reset_travels_with_the_group(rg):
    """Nobody looks at the queues between the step-down and rg_checkpoint / rg_permute_groups: what has to travel is what the
    clock call left in the queue's own cells. Acks after a restore of that checkpoint, and acks at the groups' new positions,
    release nothing for a stepper and the model's states for the others."""
    r = StepRig(rg, 3, 2)
    pend = r.fill()
    r.check_states()
    steppers, stayers = r.to_the_step_down()
    saved = r.save()  # (a checkpoint AFTER the step-down)
    states = r.late_acks(pend, dense=True)
    no_state_of(states, steppers)
    assert states
    r.load(saved)
    perm = np.random.default_rng(3).permutation(r.n).astype(np.uint64)
    assert any(int(perm[i]) != i for i in range(r.n))
    r.eng.permute_groups(perm)
    r.model.groups = [r.model.groups[int(o)] for o in perm]
    r.clock = [r.clock[int(o)] for o in perm]
    r.cfg = r.cfg[perm.astype(np.int64)]
    moved = {i: pend[int(o)] for i, o in enumerate(perm) if int(o) in pend}
    now_steppers = [i for i, o in enumerate(perm) if int(o) in set(steppers)]
    r.check_cells()
    again = r.late_acks(moved, dense=False, recheck=now_steppers)
    no_state_of(again, now_steppers)
    assert sorted((int(perm[g]), c, i) for g, c, i in again) == sorted(states)
    last, counts = r.pending()
    assert not any(counts[g] or last[g] for g in now_steppers)
    r.close()


@pytest.mark.parametrize("order", ["read_first", "clock_first"])
def test_either_enable_order(rg, order):
    """rg_read_index_enable before rgx_lead_clock_enable and after it: the clock finds the queues either way."""
    r = StepRig(rg, 3, 2, order=order)
    pend = r.fill()
    r.check_states()
    steppers, _ = r.to_the_step_down()
    states = r.late_acks(pend, dense=True)
    no_state_of(states, steppers)
    assert states and stepper_contexts(pend, steppers)
    last, counts = r.pending()
    assert not any(counts[g] or last[g] for g in steppers)
    r.close()


def test_a_clock_without_read_index_behaves_as_before(rg):
    """No ReadIndex layer: the clock's events, cells, cfg words and flag rows are the model's through two election timeouts, and
    the read calls are still refused on the host."""
    r = StepRig(rg, 3, 2, order="clock_only")
    seen = set()
    for _ in range(4):
        seen |= set(r.verify(r.clock_call()))
        r.check_cells()
    assert DOWN in seen and L.EV_BEAT in seen and L.EV_BEAT | L.EV_CHECK_QUORUM in seen
    for call in (r.eng.read_pending_counts, r.eng.read_last_pending, r.eng.read_states, lambda: r.eng.read_index([(0, 5)])):
        with pytest.raises(rg.EngineError) as ei:
            call()
        assert ei.value.code == -8
    r.close()
