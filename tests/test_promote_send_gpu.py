"""GPU: the promotion into an engine with device Inflights (rgh_follow_promote / rgh_follow_promote_device) against the reference's
route through the oracle, all on the CPU -- handoff_rig.route_state, the RG_MF_BECOME_LEADER tick, Cluster.send_stage_soa with the
oracle's own Inflights (promote_send_model.oracle_route) -- and against tests/promote_send_model.py: every leader column of every
group, every window, the item set, exactly. 130 lead groups behind an arena of 300 followed groups (one full block plus a 44-lane
tail). No test provokes a device fault: every bad argument is refused on the host, every bad dense cell is an ANSWER."""
import ctypes

import numpy as np
import pytest

import elect_model as EM
import gate_model as G
import handoff_model as H
import handoff_rig as R
import promote_send_model as M
import sendstage
from test_follow_gate_gpu import soft_array, states_array
from test_handoff_gpu import GATE, U64_SENT, Rig, dev, same_but_out

pytestmark = pytest.mark.gpu

U64_MAX = (1 << 64) - 1
CANARY = 0x7E
MF_VALID, MF_APPEND = 0x01, 0x20
SEND_BYTES = 0x2


class SendRig(Rig):
    """A leader engine of 130 x P with device Inflights behind a follower arena of 300 groups, gate and election cells enabled."""

    def __init__(self, rg, P, ix64=False, max_inflight=8, elect=True, n_lead=M.N_LEAD):
        self.rg, self.E, self.P, self.G, self.n, self.cap = rg, rg.engine, P, n_lead, M.N_FOLLOW, max_inflight
        self.eng = rg.Engine(self.G, P, flags=self.E.CFGF.IX64 if ix64 else None, max_inflight=max_inflight)
        self.all = np.arange(self.n, dtype=np.uint64)
        self.eng.follow_enable(self.n)
        self.stride = self.eng.follow_stride()
        assert self.stride >= self.n
        if elect:
            self.eng.follow_gate_enable(GATE.election_tick, GATE.min_timeout, GATE.max_timeout, GATE.flags, GATE.seed)
            self.eng.follow_elect_enable()

    def windows(self):
        """every window of the engine, logically: (meta as rg_read_inflights reports it, {(group, slot): entries oldest first})"""
        meta, ring = self.eng.read_inflights()
        return meta, {(g, s): self.eng.inflights(g, s, meta, ring) for g in range(self.G) for s in range(self.P)}

    def everything(self):
        return self.read_lead(), self.arena(), self.windows()

    def unchanged(self, before, what):
        lead, arena, (meta, win) = self.everything()
        same_but_out(before[0], lead, what)
        assert (lead["out"] == before[0]["out"]).all() and (lead["host_hint"] == before[0]["host_hint"]).all(), what
        assert arena == before[1], what
        assert (meta == before[2][0]).all() and win == before[2][1], what

    def promote_send(self, cases, dense, answers, item_cap=None, max_entries=0, flags=0, extra=()):
        """promote `cases` with the new call, compare every answer field with `answers` -> (items written, total). `extra`: dense
        only, further (follow group, lead cell) pairs selected as WON (their answers are the caller's to check: -> status column)."""
        import torch
        room = len(cases) * self.P if item_cap is None else item_cap
        if not dense:
            resp, items, total = self.eng.follow_promote_send(self.recs(cases), max_entries, flags, item_cap)
            assert [tuple(int(r[k]) for k in ("status", "term", "last_index", "commit", "out")) for r in resp] == answers
            return items, total
        result, lead, persisted = np.zeros(self.stride, np.uint8), np.full(self.stride, U64_SENT, np.uint64), np.full(self.stride, U64_SENT, np.uint64)
        result[:self.n] = np.arange(self.n) % EM.WON  # every value but WON selects nothing, whatever the lead column holds
        for c, r in zip(cases, self.recs(cases)):
            result[c.g], lead[c.g], persisted[c.g] = EM.WON, c.L, r["persisted"]
        for g, cell in extra:
            result[g], lead[g] = EM.WON, cell
        out = self.out_columns()
        buf = torch.full(((room + 2) * 32,), CANARY, dtype=torch.uint8, device="cuda")  # two items of canary behind item_cap
        count = torch.full((2,), 0x55555555, dtype=torch.int32, device="cuda")
        cols = (dev(result), dev(lead), dev(persisted))
        self.eng.follow_promote_send_device(cols[0], cols[1], out, buf if room else None, room, count, cols[2], max_entries, flags)
        self.eng.sync()
        if not extra:
            self.dense_answers(out, cases, answers)
        self.status = out["status"].cpu().numpy()
        total = int(count.cpu().numpy().view(np.uint32)[0])
        assert int(count.cpu().numpy().view(np.uint32)[1]) == 0x55555555
        raw = buf.cpu().numpy()
        assert (raw[room * 32:] == CANARY).all(), "nothing is written beyond item_cap"
        k = min(total, room)
        assert (raw[k * 32:room * 32] == CANARY).all()
        return raw[:k * 32].view(self.E.SEND_ITEM_DTYPE).copy(), total


def loaded_rig(rg, P, cases, ix64=False, cap=8, window_groups=None):
    """The rig with `cases` in place: the lead state, the arena, the windows of the cases' lead groups (and of window_groups) in the
    five starting shapes -> (rig, the python state loaded, what the engine holds before the call)"""
    rig = SendRig(rg, P, ix64, cap)
    st = R.state_with(rig.G, P, rig.eng.stride, cases)
    rig.load_lead(st)
    rig.load_arena(cases)
    meta, ring, shapes = M.window_arrays(rig.G, P, rig.eng.stride, cap, sorted({c.L for c in cases} | set(window_groups or ())))
    rig.eng.load_inflights(meta, ring)
    rig.shapes = shapes
    return rig, st, rig.everything()


def expect_after(rig, before, cases):
    """The model over what the engine held before the call -> (state, meta, answers, items)"""
    lead, _, (meta, win) = before
    ring = np.zeros((rig.G, rig.P, rig.cap), dtype=np.uint64)
    for (g, s), entries in win.items():  # (the model reads a window as its entries: written out at the start rg_read_inflights reports)
        start = int(meta[s, g]) & 0xFFFF
        for i, e in enumerate(entries):
            ring[g, s, (start + i) % rig.cap] = e
    return M.promote_state(lead, meta, ring, cases, rig.cap)


def check_after(rig, st, before, cases, items, total, want_items=None):
    """Every column, every window and the items against the model over the state before and against the oracle's route"""
    want, want_meta, answers, model_items = expect_after(rig, before, cases)
    got, arena, (meta, win) = rig.everything()
    same_but_out(want, got, "promotion against the model")
    assert (got["out"] == before[0]["out"]).all() and (got["host_hint"] == before[0]["host_hint"]).all()
    assert arena == before[1], "a promotion leaves all three layers of the arena alone"
    assert (meta == want_meta).all(), np.argwhere(meta != want_meta)[:4]
    done = {c.L for c in cases if c.expect == H.DONE}
    for (g, s), entries in win.items():
        present = H.cfg_fields(int(got["cfg"][g]))[4]
        assert entries == ([] if g in done and present >> s & 1 else before[2][1][(g, s)]), (g, s, entries)
    assert total == len(model_items) and sendstage.items_dict(items) == (model_items if want_items is None else want_items)
    # the reference's route: the tick, then the stage with the oracle's own Inflights
    after, gout, sent, cl = M.oracle_route(st, cases, rig.cap)
    if want_items is None:
        sendstage.compare_items(items, sent)
    for c in cases:
        if c.expect == H.DONE:
            assert R.get_lead(after, c.L) == R.get_lead(got, c.L), c.name
            for s in range(rig.P):
                assert cl.ins_contents(c.L, s + 1) == [] == (win[(c.L, s)] if H.cfg_fields(c.lead["cfg"])[4] >> s & 1 else [])
        else:
            assert R.get_lead(got, c.L) == R.get_lead(before[0], c.L), c.name
    return want, model_items


# ---------------------------------------------------------------------------------------------------------------------
# 1. equality with the route
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [1, 4, 8])
@pytest.mark.parametrize("ix64", [False, True])
@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("P", [3, 5])
def test_promotion_with_windows_equals_the_route(rg, P, dense, ix64, cap):
    """Promoted groups in neighbouring lanes of one wave, across a wave boundary and in both blocks (max_inflight 1: in the tail
    block only -- the first block promotes nobody), a FAULT among them; the windows of every case in the five starting shapes
    (cap 8: six entries are a ring window, a start of 7 wraps; cap 4: full and compact)."""
    cases = M.edge_cases(P, blocks="tail" if cap == 1 else "both")
    rig, st, before = loaded_rig(rg, P, cases, ix64, cap, window_groups=(2, 3))
    assert set(rig.shapes.values()) == set(M.WINDOW_SHAPES)
    if cap == 8:
        assert any(len(w) > 4 for w in before[2][1].values()) and any(int(before[2][0][s, g]) & 0xFFFF == 7 for (g, s) in before[2][1])
    answers = [a for a in expect_after(rig, before, cases)[2]]
    assert {a[0] for a in answers} == {H.DONE, H.FAULT}
    items, total = rig.promote_send(cases, dense, answers)
    want, model_items = check_after(rig, st, before, cases, items, total)
    if P == 5:  # a learner gets an item, an absent slot keeps its window cells
        c = next(c for c in cases if c.expect == H.DONE and H.cfg_fields(c.lead["cfg"])[4] == H.mask((0, 1, 2, 4)))
        assert (c.L, 4) in model_items and (c.L, 3) not in model_items and (c.L, 2) not in model_items
        assert rig.windows()[0][3, c.L] == before[2][0][3, c.L] and (before[2][0][3, c.L] != 0 or rig.shapes[(c.L, 3)] == "empty")
    rig.close()


@pytest.mark.parametrize("dense", [False, True])
def test_one_slot_is_done_with_no_item(rg, dense):
    cases = M.edge_cases(1)
    rig, st, before = loaded_rig(rg, 1, cases, cap=4)
    answers = expect_after(rig, before, cases)[2]
    items, total = rig.promote_send(cases, dense, answers)
    assert total == 0 and len(items) == 0 and sum(a[0] == H.DONE for a in answers) == len(cases) - 1
    check_after(rig, st, before, cases, items, total)
    rig.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. refused records
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dense", [False, True])
def test_refused_records_change_nothing(rg, dense):
    """NOT_WON, CONF, NOT_PERSISTED and FAULT beside promoted groups (the dense form: also a lead cell beyond the engine): every
    cell of both sides, every window and the item count equal those of a run without the refused records."""
    good = M.edge_cases(3)
    bad = H.refusal_cases()
    runs = []
    for with_bad in (False, True):
        rig, st, before = loaded_rig(rg, 3, good + bad, cap=4)  # (both runs load the refused groups and their windows)
        cases = good + bad if with_bad else good
        answers = expect_after(rig, before, cases)[2]
        extra = [(200, rig.G)] if dense and with_bad else ()
        items, total = rig.promote_send(cases, dense, answers, extra=extra)
        if extra:
            want = {c.g: a[0] for c, a in zip(cases, answers)}
            want[200] = H.FAULT
            assert [int(x) for x in rig.status[:rig.n]] == [want.get(g, H.NONE) for g in range(rig.n)]
        if with_bad:
            assert sorted({a[0] for a in answers}) == [H.DONE, H.NOT_WON, H.CONF, H.NOT_PERSISTED, H.FAULT]
            for c in bad:
                assert R.get_lead(rig.read_lead(), c.L) == R.get_lead(before[0], c.L), c.name
        runs.append((rig.everything(), sendstage.items_dict(items), total))
        rig.close()
    (lead_a, arena_a, (meta_a, win_a)), items_a, total_a = runs[0]
    (lead_b, arena_b, (meta_b, win_b)), items_b, total_b = runs[1]
    same_but_out(lead_a, lead_b, "refused records")
    assert arena_a == arena_b and (meta_a == meta_b).all() and win_a == win_b and items_a == items_b and total_a == total_b > 0


# ---------------------------------------------------------------------------------------------------------------------
# 3. item_cap
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dense", [False, True])
def test_item_cap(rg, dense):
    """item_cap 0, the total minus one and the total: the count is the total each time, the items written are a subset of the
    model's, and (dense) two items' worth of canary behind item_cap survives."""
    cases = M.edge_cases(5)
    full = None
    for k, cap_of in enumerate((lambda t: t, lambda t: t - 1, lambda t: 0)):
        rig, st, before = loaded_rig(rg, 5, cases, cap=4)
        want, want_meta, answers, model_items = expect_after(rig, before, cases)
        item_cap = cap_of(len(model_items))
        items, total = rig.promote_send(cases, dense, answers, item_cap=item_cap)
        got = sendstage.items_dict(items)
        assert total == len(model_items) > 2 and len(got) == item_cap and all(model_items[key] == v for key, v in got.items())
        same_but_out(want, rig.read_lead(), "item_cap %d" % item_cap)
        assert (rig.windows()[0] == want_meta).all()
        rig.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. message limits and the empty entry's size record
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("max_entries,flags", [(0, 0), (1, 0), (0, 1), (0, SEND_BYTES), (U64_MAX, SEND_BYTES)])
def test_message_limits_change_nothing(rg, dense, max_entries, flags):
    """max_entries_per_msg 0 and 1, RG_SEND_SKIP_BCAST_COMMIT, RG_SEND_BYTES with limits 0 and UINT64_MAX (after
    rg_log_sizes_enable(8)): the one entry goes out whole -- the route's items (the host tests hold the oracle's stage under these
    limits against the same model)."""
    cases = M.edge_cases(3)
    rig, st, before = loaded_rig(rg, 3, cases, cap=8)
    if flags & SEND_BYTES:
        rig.eng.log_sizes_enable(8)
    answers = expect_after(rig, before, cases)[2]
    items, total = rig.promote_send(cases, dense, answers, max_entries=max_entries, flags=flags)
    check_after(rig, st, before, cases, items, total)
    rig.close()


@pytest.mark.parametrize("dense", [False, True])
def test_the_empty_entrys_size_record(rg, dense):
    """Four promoted groups with the same log (last_index 7, T = 4: the empty entry is index 8, 4 bytes), cumulative record 1000 at
    index 7. The record the call writes for index 8 and the cell before it are read back through a following byte-limited stage
    (limit 30 bytes): the leader appends entries 9 and 10, peer 0 acknowledges 8 (groups X, Y: the stage's sums start at the
    record of 8) or 7 (Z1, Z2: at the record of 7). X and Z1 hold exactly 30 bytes behind the base when the record is right -- one
    message; Y and Z2 31 -- two. One byte more or less in either cell flips one of the four."""
    c, t = H.LOG_EDGES["one_run"]
    cfg = H.mask((0, 1, 2)) | 1 << 16 | 7 << 24
    import random
    rng = random.Random(3)
    groups = {"X": (0, 5), "Y": (1, 64), "Z1": (256, 129), "Z2": (299, 0)}
    cases = [H.Case(k, g, L, H.Follower(c, t, 7, (0, 1, 2), (), 1), H.make_lead(3, cfg, rng)) for k, (g, L) in groups.items()]
    rig, st, before = loaded_rig(rg, 3, cases, cap=8)
    E, eng = rig.E, rig.eng
    eng.log_sizes_enable(8)
    hi, size = 8, M.empty_entry_size(t, 8)
    assert (t, c["last_index"], size) == (4, 7, 4)
    recs = np.zeros(len(cases), dtype=E.LOG_SIZE_DTYPE)
    for k, cs in enumerate(cases):
        recs[k] = (cs.L, hi - 1, 1000)
    eng.log_sizes_write(recs)
    answers = expect_after(rig, before, cases)[2]
    items, total = rig.promote_send(cases, dense, answers, max_entries=30, flags=SEND_BYTES)
    check_after(rig, st, before, cases, items, total)
    later = np.zeros(2 * len(cases), dtype=E.LOG_SIZE_DTYPE)
    mb = rg.MsgBuffers(rig.G, 3, eng.stride)
    for k, cs in enumerate(cases):
        total_bytes = 1000 + size + (30 if cs.name in ("X",) else 31 if cs.name == "Y" else 30 - size if cs.name == "Z1" else 31 - size)
        later[2 * k], later[2 * k + 1] = (cs.L, hi + 1, 1000 + size + 10), (cs.L, hi + 2, total_bytes)
        mb.m_flags[cs.L, 0], mb.m_index[0, cs.L] = MF_VALID, hi if cs.name in ("X", "Y") else hi - 1
        mb.m_flags[cs.L, 1], mb.m_index[1, cs.L], mb.m_commit[1, cs.L] = MF_VALID | MF_APPEND, hi + 2, hi + 2
    eng.log_sizes_write(later)
    eng.tick_send(mb, max_bytes=30)
    got = sendstage.items_dict(eng.send_items())
    n_msgs = {cs.name: got[(cs.L, 0)][3] for cs in cases}
    assert all(got[(cs.L, 0)][2] == hi + 2 and got[(cs.L, 0)][0] == 1 for cs in cases), got
    assert all(got[(cs.L, 0)][1] == (hi if cs.name in ("X", "Y") else hi - 1) for cs in cases), got
    assert n_msgs == {"X": 1, "Y": 2, "Z1": 1, "Z2": 2}, n_msgs
    rig.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the engine's own list survives
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dense", [False, True])
def test_the_engines_own_item_list_survives(rg, dense):
    """rg_tick_device_send over other groups, then the new call: rg_send_items answers what it answers on an engine that never made
    the call -- whether the compact list had been materialised from the stage's columns before the call or not --, and
    rg_send_columns / rg_send_tail_column still serve the stage."""
    cases = M.edge_cases(3)
    lists, cols = [], []
    for when in ("never", "before the first read", "after it"):
        rig, st, before = loaded_rig(rg, 3, cases, cap=4)
        eng = rig.eng
        mb = rg.MsgBuffers(rig.G, 3, eng.stride)
        for g in range(10, 60):  # quiet base groups (entries 1..3, commit 2): an ack of 3 commits it and broadcasts
            mb.m_flags[g, 1], mb.m_index[1, g] = MF_VALID, 3
        d = [dev(getattr(mb, k)) for k in ("m_index", "m_commit", "m_hint", "m_rs", "m_flags")]
        eng.tick_device_send(*[x.data_ptr() for x in d])
        eng.sync()
        if when == "after it":
            first = sendstage.items_dict(eng.send_items())
        if when != "never":
            before = rig.everything()
            answers = expect_after(rig, before, cases)[2]
            items, total = rig.promote_send(cases, dense, answers)
            assert total == len(items) > 0 and not {k[0] for k in sendstage.items_dict(items)} & set(range(10, 60))
        cols.append(eng.send_columns() + (eng.send_tail_column(),))
        lists.append(sendstage.items_dict(eng.send_items()))
        if when == "after it":
            assert first == lists[-1]
        assert all(cols[-1]) and eng.send_columns() == cols[-1][:3]
        rig.close()
    assert lists[0] == lists[1] == lists[2] and len(lists[0]) >= 40 and {k[0] for k in lists[0]} <= set(range(10, 60))


# ---------------------------------------------------------------------------------------------------------------------
# 6. the whole life cycle on an engine with device Inflights
# ---------------------------------------------------------------------------------------------------------------------
def test_life_cycle_with_device_inflights(rg):
    """Election on the device, promotion with the new call, rg_tick_device_send with acks until the windows of peer 0 are ring
    windows (the oracle ticks and sends along, with its own Inflights, from the promoted state), step-down through rgx_lead_clock
    and rgx_follow_step_down_device, a second election in the arena at term + 1, promotion again: the windows are empty, the
    items are those of the new term, the first leadership's entries are filed as a run -- all against the oracle's route."""
    import torch
    import lead_clock_model as LC
    import oracle_lib as O
    from life_cycle_rig import CLOCK, elect_out, vote_round
    from test_follow_elect_gpu import cells_array
    P, cap = 3, 8
    rig = SendRig(rg, P, max_inflight=cap)
    E, eng, S = rig.E, rig.eng, rig.stride
    winners = {0: 129, 63: 5, 64: 77, 299: 64}  # follow group -> lead group
    cfg = H.mask((0, 1, 2)) | 1 << 16 | 7 << 24
    log = H.canon(0, 0, [(1, 1), (4, 2)], 6, 6)
    st = R.base_state(rig.G, P, eng.stride)
    for Lg in winners.values():
        st["cfg"][Lg] = cfg
    rig.load_lead(st)
    gs = sorted(winners)
    nodes = {}
    for g in gs:
        nd = EM.Node(GATE, g, H.log_of(log), self_id=2, incoming=(0, 1, 2), self_slot=1)
        nd.load(2, 0, 1, 0, G.FOLLOWER, 0, 0, True)  # a follower of peer 1 at term 2
        nodes[g] = nd
    eng.follow_write(states_array(E, gs, [nodes[g].log.canonical() for g in gs]))
    eng.follow_elect_write(cells_array(E, gs, [nodes[g].cells() for g in gs]))
    eng.lead_clock_enable(CLOCK.election_tick, CLOCK.heartbeat_tick, CLOCK.flags)
    lead = np.full(S, LC.NO_LEAD, np.uint64)
    for g, Lg in winners.items():
        lead[g] = Lg
    d_lead = dev(lead)
    hup = torch.full((S,), -1, dtype=torch.int64, device="cuda")
    softs = {g: nodes[g].soft() for g in gs}
    hi_of = {}
    for cycle, T in enumerate((3, 4)):
        # ---- the election, on the device: three clock ticks to the timeout, the campaign, both vote rounds ----
        eng.follow_soft_write(soft_array(E, gs, [softs[g][:5] + (softs[g][6] - 3, softs[g][6], softs[g][7]) for g in gs]))
        pre, real = vote_round(S, gs, EM.PREVOTE, T), vote_round(S, gs, EM.VOTE, T)
        o_camp, o_pre, o_real = elect_out(S), elect_out(S), elect_out(S)
        for _ in range(3):
            eng.follow_clock(hup, S, sync=False)
            eng.follow_campaign_device(hup, eng.follow_clock_counts(), S, o_camp)
        eng.follow_vote_resps_device(pre, o_pre)
        eng.follow_vote_resps_device(real, o_real)
        eng.sync()
        assert sorted(int(g) for g in np.nonzero(o_real["result"].cpu().numpy()[:rig.n] == EM.WON)[0]) == gs, cycle
        before = rig.everything()
        arena = before[1]
        assert all(arena[g][1][0] == T and arena[g][1][2] == 2 and arena[g][1][4] == G.FOLLOWER for g in gs), (cycle, arena[0][1])
        cases = [H.Case("w%d" % g, g, winners[g], H.Follower(arena[g][0], T, 2, (0, 1, 2), (), 1), R.get_lead(before[0], winners[g])) for g in gs]
        if cycle == 1:  # what the first leadership left: ring windows at peer 0, its entries in the arena's log
            assert all(len(before[2][1][(Lg, 0)]) > 4 for Lg in winners.values()), [before[2][1][(Lg, 0)] for Lg in winners.values()]
            assert all(arena[g][0]["runs"][-1] == (hi_of[g], 3) and arena[g][0]["last_index"] == hi_of[g] + 6 for g in gs), arena[0][0]
        # ---- the promotion: the new call on the vote round's result column ----
        want, want_meta, answers, model_items = expect_after(rig, before, cases)
        out = rig.out_columns()
        buf = torch.zeros((len(gs) * P * 32,), dtype=torch.uint8, device="cuda")
        count = torch.zeros((1,), dtype=torch.int32, device="cuda")
        eng.follow_promote_send_device(o_real["result"], d_lead, out, buf, len(gs) * P, count, None)
        eng.sync()
        rig.dense_answers(out, cases, answers)
        total = int(count.cpu().numpy()[0])
        items = buf.cpu().numpy()[:total * 32].view(E.SEND_ITEM_DTYPE)
        want, model_items = check_after(rig, before[0], before, cases, items, total)
        for g in gs:
            hi = arena[g][0]["last_index"] + 1
            hi_of[g] = hi
            assert answers[gs.index(g)] == (H.DONE, T, hi, arena[g][0]["committed"], 0x18)
            assert model_items[(winners[g], 0)] == model_items[(winners[g], 2)] == (M.SEND_APPEND, hi - 1, hi, 1)
        if cycle == 1:
            d = R.get_lead(rig.read_lead(), winners[0])
            n = d["run_count"]
            assert (d["run_first"][n - 1], d["run_term"][n - 1]) == (hi_of[0] - 7, 3) and d["cur_term"] == 4 and d["term_lo"] == d["term_hi"] == hi_of[0]
            break
        # ---- the leadership: six ticks with their send stages, the oracle along with its own Inflights ----
        cl = O.Cluster(rig.G)
        state = rig.read_lead()
        cl.load_soa(state, term=2, max_inflight=cap)
        cl.set_own_inflights(True)
        hi = hi_of[gs[0]]
        assert all(hi_of[g] == hi for g in gs)
        for t in range(6):
            mb = rg.MsgBuffers(rig.G, P, eng.stride)
            for Lg in winners.values():  # the leader appends and persists one entry per tick; peer 0 acknowledges the empty entry once
                mb.m_flags[Lg, 1], mb.m_index[1, Lg], mb.m_commit[1, Lg] = MF_VALID | MF_APPEND, hi + t + 1, hi + t + 1
                if t == 0:
                    mb.m_flags[Lg, 0], mb.m_index[0, Lg] = MF_VALID, hi
            d = [dev(getattr(mb, k)) for k in ("m_index", "m_commit", "m_hint", "m_rs", "m_flags")]
            eng.tick_device_send(*[x.data_ptr() for x in d])
            eng.sync()
            gout = np.zeros(rig.G, dtype=np.uint32)
            cl.tick_soa(mb.as_dict(), gout)
            sent = cl.send_stage_soa(gout, 0)
            sendstage.compare_items(eng.send_items(), sent)
            cl.store_soa(state)
            got = rig.read_lead()
            diffs = R.diff(state, got, O.STATE_COLS)
            assert not diffs and (got["out"] == gout).all(), (t, diffs)
            meta, ring = eng.read_inflights()
            sendstage.compare_rings(cl, meta, ring, state, cap)
        assert all(rig.eng.inflights(Lg, 0) == [hi + k for k in range(1, 7)] for Lg in winners.values())
        # ---- the step-down: the clock until the election timeout finds no quorum, rgx_follow_step_down_device behind every call ----
        down = set()
        for _ in range(8):
            events = torch.zeros(eng.stride, dtype=torch.uint8, device="cuda")
            o_down = rig.out_columns()
            eng.lead_clock(events, sync=False)
            eng.follow_step_down_device(events, d_lead, o_down)
            eng.sync()
            status = o_down["status"].cpu().numpy()
            down |= {g for g in gs if int(status[g]) == H.DONE}
            if down == set(gs):
                break
        assert down == set(gs)
        arena = rig.arena()
        for g in gs:  # everything the group holds is committed before it campaigns again (a campaign needs term(committed))
            canon = dict(arena[g][0])
            assert canon["last_index"] == hi + 6 and canon["runs"][-1] == (hi, 3), canon
            canon["committed"] = canon["last_index"]
            nodes[g].log = H.log_of(canon)
            softs[g] = arena[g][1]
            assert softs[g][0] == 3 and softs[g][2] == 0 and softs[g][4] == G.FOLLOWER, softs[g]
        eng.follow_write(states_array(E, gs, [nodes[g].log.canonical() for g in gs]))
    rig.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------------------------------
def code_of(rg, call):
    with pytest.raises(rg.EngineError) as ei:
        call()
    return ei.value.code, str(ei.value)


def test_refusals(rg):
    """Every refusal of the header, each followed by a comparison of the arena, the leader columns and the windows with their state
    before."""
    import torch
    cases = M.edge_cases(3)
    rig, st, before = loaded_rig(rg, 3, cases, cap=4)
    E, eng = rig.E, rig.eng
    STATE, ARG = E.ERR["STATE"], E.ERR["INVALID_ARG"]
    recs = rig.recs(cases)
    S = rig.stride
    result, lead, out = dev(np.full(S, EM.WON, np.uint8)), dev(np.zeros(S, np.uint64)), rig.out_columns()
    buf = torch.zeros((64 * 32,), dtype=torch.uint8, device="cuda")
    count = torch.zeros((1,), dtype=torch.int32, device="cuda")

    def sparse(r=recs, **kw):
        return lambda: eng.follow_promote_send(r, kw.get("max_entries", 0), kw.get("flags", 0))

    def dense_call(res=result, ld=lead, o=out, items=buf, cap=64, cnt=count, flags=0):
        return lambda: eng.follow_promote_send_device(res, ld, o, items, cap, cnt, None, 0, flags)
    refused = [("unknown flags", sparse(flags=4), ARG), ("unknown flags", dense_call(flags=0x80), ARG),
               ("RG_SEND_BYTES without the size table", sparse(flags=SEND_BYTES), STATE), ("RG_SEND_BYTES without the size table", dense_call(flags=SEND_BYTES), STATE),
               ("result NULL", dense_call(res=None), ARG), ("lead NULL", dense_call(ld=None), ARG), ("count NULL", dense_call(cnt=None), ARG),
               ("items NULL with a capacity", dense_call(items=None), ARG), ("an output column NULL", dense_call(o={**out, "term": None}), ARG)]
    for bad in ([(rig.n, 0)], [(0, rig.G)], [(1, 5), (1, 6)], [(1, 5), (2, 5)]):  # the record faults of the shared walk
        a = np.zeros(len(bad), dtype=E.HANDOFF_REC_DTYPE)
        for k, (g, L) in enumerate(bad):
            a[k]["follow_group"], a[k]["lead_group"] = g, L
        refused.append(("record fault %r" % (bad,), sparse(r=a), ARG))
    for what, call, want in refused:
        assert code_of(rg, call)[0] == want, what
        rig.unchanged(before, what)
    n = ctypes.c_uint64(0)
    resp = np.zeros(len(recs), dtype=E.HANDOFF_RESP_DTYPE)
    raw = eng.L.rgh_follow_promote
    assert raw(eng.h, recs.ctypes.data, len(recs), resp.ctypes.data, 0, 0, None, 0, None) == ARG  # n_items NULL
    assert raw(eng.h, recs.ctypes.data, len(recs), resp.ctypes.data, 0, 0, None, 3, ctypes.byref(n)) == ARG  # items NULL with a capacity
    assert raw(eng.h, None, 1, resp.ctypes.data, 0, 0, None, 0, ctypes.byref(n)) == ARG and raw(eng.h, recs.ctypes.data, 1, None, 0, 0, None, 0, ctypes.byref(n)) == ARG
    rig.unchanged(before, "NULL pointers")
    # a tick's stage is still owed
    mb = rg.MsgBuffers(rig.G, 3, eng.stride)
    eng.tick(mb)
    owed = rig.everything()
    for call in (sparse(), dense_call()):
        code, text = code_of(rg, call)
        assert code == STATE and "rg_send_appends" in text
    rig.unchanged(owed, "a stage is owed")
    eng.send_appends(0)
    eng.sync()
    # ... and once it has run the call is served
    settled = rig.everything()
    answers = expect_after(rig, settled, cases)[2]
    items, total = rig.promote_send(cases, False, answers)
    assert total == len(items) > 0
    rig.close()
    # no device Inflights: the older calls are this engine's promotion; no election layer
    plain = Rig(rg, 3)
    for call in (lambda: plain.eng.follow_promote_send(np.zeros(1, dtype=E.HANDOFF_REC_DTYPE)),
                 lambda: plain.eng.follow_promote_send_device(result, lead, out, buf, 64, count)):
        code, text = code_of(rg, call)
        assert code == STATE and "rg_follow_promote" in text
    plain.close()
    bare = SendRig(rg, 3, elect=False)
    bare.load_lead(R.base_state(bare.G, 3, bare.eng.stride))
    for call in (lambda: bare.eng.follow_promote_send(np.zeros(1, dtype=E.HANDOFF_REC_DTYPE)),
                 lambda: bare.eng.follow_promote_send_device(result, lead, out, buf, 64, count)):
        code, text = code_of(rg, call)
        assert code == STATE and "rg_follow_elect_enable" in text
    bare.close()


def test_unresolved_host_hints_refuse_the_call(rg):
    """Groups that still carry RG_OUT_HOST_HINT: RG_ERR_STATE from both forms, nothing changed; served once the hint is answered."""
    import torch
    from test_tick_unit_edges_gpu import M_INDEX, crafted_tick, to_buffers
    rig = SendRig(rg, 3, max_inflight=4)
    E, eng, S = rig.E, rig.eng, rig.stride
    st, host, msgs = crafted_tick(rig.G, 3, {9: 0b010})
    eng.load_state(st)
    eng.tick(to_buffers(rg, eng, msgs))
    eng.send_appends(0)
    eng.sync()
    assert int(eng.read_column(E.COL.OUT)[9]) & 0x20
    before = rig.everything()
    result, lead, out = dev(np.zeros(S, np.uint8)), dev(np.zeros(S, np.uint64)), rig.out_columns()
    count = torch.zeros((1,), dtype=torch.int32, device="cuda")
    for call in (lambda: eng.follow_promote_send(np.zeros(1, dtype=E.HANDOFF_REC_DTYPE)), lambda: eng.follow_promote_send_device(result, lead, out, None, 0, count)):
        code, text = code_of(rg, call)
        assert code == E.ERR["STATE"] and "rg_resolve_host_hints" in text
    rig.unchanged(before, "unresolved host hints")
    assert eng.resolve_host_hints([(9, M_INDEX, 13, 1, 0)]).all()
    eng.follow_promote_send_device(result, lead, out, None, 0, count)  # (selects nobody)
    eng.sync()
    assert int(count.cpu().numpy()[0]) == 0 and not out["status"].cpu().numpy()[:rig.n].any()
    rig.close()


def test_mirrored_engine(rg):
    """rg_set_peers: the dense form is refused; the sparse form keeps rg_follow_promote's rules -- a lead group with queued mirror
    events is RG_ERR_SLOT_BUSY, and after DONE the term is registered in the mirror's gate."""
    import torch
    rig = SendRig(rg, 3, max_inflight=4)
    E, eng = rig.E, rig.eng
    L, g = 9, 33
    st = R.base_state(rig.G, 3, eng.stride)
    st["cfg"][L] = H.mask((0, 1, 2)) | 1 << 16 | 7 << 24
    st["match"][:, L] = (2, 3, 1)
    rig.load_lead(st)
    for grp in range(rig.G):
        eng.set_peers(grp, [101, 102, 103], 2)
    case = H.Case("mirror", g, L, H.Follower(H.canon(0, 0, [(1, 2)], 3, 3), 6, 102, (0, 1, 2), (), 1), R.get_lead(st, L))
    rig.load_arena([case])
    S = rig.stride
    result, lead, out = dev(np.zeros(S, np.uint8)), dev(np.zeros(S, np.uint64)), rig.out_columns()
    count = torch.zeros((1,), dtype=torch.int32, device="cuda")
    code, text = code_of(rg, lambda: eng.follow_promote_send_device(result, lead, out, None, 0, count))
    assert code == E.ERR["STATE"] and "host mirror" in text
    eng.step(L, 101, 2, 3)  # an ack of the old term waits in the mirror's queue
    before = rig.everything()
    assert code_of(rg, lambda: eng.follow_promote_send(rig.recs([case])))[0] == E.ERR["SLOT_BUSY"]
    rig.unchanged(before, "queued events")
    eng.flush_send(0)
    eng.sync()
    before = rig.everything()
    want, want_meta, answers, model_items = expect_after(rig, before, [case])
    items, total = rig.promote_send([case], False, answers)
    assert answers == [(H.DONE, 6, 4, 3, 0x18)] and total == 2 and sendstage.items_dict(items) == model_items
    same_but_out(want, rig.read_lead(), "the mirrored promotion")
    eng.step(L, 103, 2, 3)   # the old term: dropped by the gate
    eng.step(L, 101, 6, 4)   # the new leader's term: applied
    eng.flush_send(0)
    match = eng.read_column(E.COL.MATCH)
    assert [int(match[s, L]) for s in range(3)] == [4, 3, 0]
    with pytest.raises(rg.EngineError) as ei:
        eng.step(L, 103, 7, 4)
    assert ei.value.code == E.ERR["HIGHER_TERM"]
    rig.close()
