"""GPU: the batched leader transfer (rgm_transfer_leader / rgm_transfer_leader_device) against tests/transfer_model.py -- every
column of every group, every window, the clock cells, the answers and the item set, exactly -- on an engine of 300 groups (two
256-thread blocks, the second partial), of 1 and of 65 groups; slot counts 1, 3, 5 and 8, max_inflight 0, 1 and 8, 32- and 64-bit
cell offsets (RG_CFGF_IX64 forces the 64-bit instantiations at this size). No test provokes a device fault: every bad argument is
refused on the host, every bad dense cell is an ANSWER."""
import ctypes

import numpy as np
import pytest

import conf_model as CM
import handoff_rig as R
import oracle_lib as O
import sendstage
import test_conf_change_gpu as CG
import transfer_model as M

pytestmark = pytest.mark.gpu

READ_COLS, CANARY, G_BIG, dev = CG.READ_COLS, CG.CANARY, CG.G_BIG, CG.dev
ALL_STATUSES = {M.STARTED, M.SELF, M.IN_PROGRESS, M.LEARNER, M.NO_PROGRESS, M.NOT_LED, M.FAULT}
EL, HB = 4, 1  # the counters every case group's clock cell is loaded with (election_tick 10, heartbeat_tick 3)


class Rig(CG.Rig):
    """CG.Rig over the transfer's cases ((name, group dict, transferee slot, windows, status): recs = [(group, slot)]), always with
    the leader's clock: every case group's cell holds election_elapsed EL and heartbeat_elapsed HB, a NOT_LED case's is stopped."""

    def __init__(self, rg, P, cap, cases=None, clock=True, **kw):
        super().__init__(rg, P, cap, cases=M.edge_cases(P) if cases is None else cases, clock=clock, **kw)
        self.cells = {}
        if clock:
            w = np.zeros(len(self.groups), dtype=self.E.LEAD_CLOCK_CELL_DTYPE)
            for k, (g, c) in enumerate(zip(self.groups, self.cases)):
                term = int(self.st["cur_term"][g])
                w[k] = (g, term, EL, HB, 0 if c[4] == M.NOT_LED else 1, [0] * 7)
                self.cells[g] = {"tag": term, "hb": HB, "el": EL}
                if c[4] == M.NOT_LED:
                    self.led[g] = False
            self.eng.lead_clock_write(w)

    def clock_cells(self):
        return self.eng.lead_clock_read(np.arange(self.G, dtype=np.uint64)) if self.led is not None else None

    def expect(self, recs=None, **limits):
        """the model over what was loaded -> (state, windows, answers, items, clock cells)"""
        win = None if self.windows is None else {k: list(v) for k, v in self.windows.items()}
        st = R.copy_state(self.st)
        st["host_hint"] = np.zeros(self.G, dtype=np.uint8)
        cells = {g: dict(c) for g, c in self.cells.items()}
        want, answers, items = M.apply_state(st, win, self.recs if recs is None else recs, self.cap, led=self.led, cells=cells, **limits)
        return want, win, answers, items, cells

    def rec_array(self, recs):
        a = np.zeros(len(recs), dtype=self.E.TRANSFER_REC_DTYPE)
        for k, (g, t) in enumerate(recs):
            a[k]["group"], a[k]["slot"] = g, t
        return a

    def apply(self, recs, dense, item_cap=None, max_entries=0, flags=0):
        """-> (answers as dicts: sparse every field, dense status / events; the items written; the total)"""
        import torch
        if not dense:
            resp, items, total = self.eng.transfer_leader(self.rec_array(recs), max_entries, flags, item_cap if self.cap else None)
            assert not resp["reserved"].any() and not resp["reserved2"].any()
            return [{k: int(r[k]) for k in resp.dtype.names if not k.startswith("reserved")} for r in resp], items, total
        to = np.zeros(self.G, np.uint8)
        for g, t in recs:
            to[g] = t + 1
        status = torch.full((self.G + 64,), CANARY, dtype=torch.uint8, device="cuda")
        events = torch.full((self.G + 64,), CANARY, dtype=torch.uint8, device="cuda")
        room = len(recs) if item_cap is None else item_cap
        buf = count = None
        if self.cap:
            buf = torch.full(((room + 2) * 32,), CANARY, dtype=torch.uint8, device="cuda")  # two items of canary behind item_cap
            count = torch.full((2,), 0x55555555, dtype=torch.int32, device="cuda")
        self.eng.transfer_leader_device(dev(to), status, events, buf if room and self.cap else None, room if self.cap else 0, count, max_entries, flags)
        self.eng.sync()
        status, events = status.cpu().numpy(), events.cpu().numpy()
        assert (status[self.G:] == CANARY).all() and (events[self.G:] == CANARY).all()
        picked = {g for g, _ in recs}
        for g in range(self.G):
            if g not in picked:
                assert status[g] == M.NONE and events[g] == CANARY, g
        answers = [{"status": int(status[g]), "events": int(events[g])} for g, _ in recs]
        if not self.cap:
            return answers, np.zeros(0, dtype=self.E.SEND_ITEM_DTYPE), 0
        total = int(count.cpu().numpy().view(np.uint32)[0])
        assert int(count.cpu().numpy().view(np.uint32)[1]) == 0x55555555
        raw = buf.cpu().numpy()
        assert (raw[room * 32:] == CANARY).all(), "nothing is written beyond item_cap"
        k = min(total, room)
        assert (raw[k * 32:room * 32] == CANARY).all()
        return answers, raw[:k * 32].view(self.E.SEND_ITEM_DTYPE).copy(), total

    def check(self, want, win, answers, items, cells, got_answers, got_items, total, clock_before=None):
        for a, b in zip(answers, got_answers):
            assert {k: a[k] for k in b} == b, (a, b)
        got = self.read()
        d = R.diff(want, got, cols=READ_COLS)
        assert not d, d
        if self.cap:
            now = self.read_windows()
            for k, v in now.items():
                assert v == win.get(k, []), (k, v, win.get(k))
        if clock_before is not None:  # every cell but election_elapsed of the model's groups is what it was
            expect = clock_before.copy()
            for g, c in cells.items():
                expect[g]["election_elapsed"] = c["el"]
            assert expect.tobytes() == self.clock_cells().tobytes()
        assert total == len(items), (total, len(items))
        if len(got_items) == total:
            assert sendstage.items_dict(got_items) == items
        else:
            assert all(items[k] == v for k, v in sendstage.items_dict(got_items).items())

    def sparse(self, recs):
        """the records the sparse form takes: a slot at or beyond P is refused on the host"""
        return [(g, t) for g, t in recs if t < self.P]

    def snapshot(self):
        everyone = np.arange(self.G, dtype=np.uint64)
        return (self.eng.read_groups(everyone).tobytes(), [a.tobytes() for a in self.eng.read_inflights()] if self.cap else None, self.read(), self.clock_cells().tobytes())

    def same(self, a, b):
        return a[0] == b[0] and a[1] == b[1] and not R.diff(a[2], b[2], cols=READ_COLS) and a[3] == b[3]


def run_against_model(rig, dense, **kw):
    recs = rig.recs if dense else rig.sparse(rig.recs)
    limits = kw.pop("limits", {})
    want, win, answers, items, cells = rig.expect(recs, **limits)
    before = rig.clock_cells()
    got_answers, got_items, total = rig.apply(recs, dense, **kw)
    rig.check(want, win, answers, items, cells, got_answers, got_items, total, before)
    return answers, items


@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("cap", [0, 1, 8])
@pytest.mark.parametrize("P,ix64", [(1, False), (3, False), (3, True), (5, False), (5, True), (8, False)])
def test_both_forms_against_the_model(rg, P, ix64, cap, dense, tail):
    """The model's edge cases at lanes 0, 63, 64, 255, 256 and 299 -- and, tail, nowhere in the first block, whose workgroup then
    leaves at its barrier: every column, every window, the clock cells, the statuses, the events, the item set."""
    rig = Rig(rg, P, cap, ix64=ix64, tail=tail)
    answers, items = run_against_model(rig, dense)
    if P > 1:
        assert {a["status"] for a in answers} == ALL_STATUSES
        assert (cap == 0) == (not items)
        assert any(a["events"] & M.EV_TIMEOUT_NOW for a in answers) and any(a["events"] & M.EV_ABORTED_PREVIOUS for a in answers)
        if cap:
            assert {v[0] for v in items.values()} == {CM.SEND_APPEND, CM.SEND_SNAPSHOT}
    rig.close()


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("G", [1, 65])
def test_one_group_and_sixty_five(rg, G, dense):
    rig = Rig(rg, 3, 4, G=G)
    run_against_model(rig, dense)
    rig.close()


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("limits,max_entries,flags", [({"max_entries": 1}, 1, 0), ({"max_bytes": 9}, 9, 2), ({"max_bytes": (1 << 64) - 1}, (1 << 64) - 1, 2)])
def test_limits(rg, limits, max_entries, flags, dense):
    """max_entries_per_msg 1, and RG_SEND_BYTES over a size window of 16 entries with a limit that splits and with none"""
    rig = Rig(rg, 5, 8)
    kw = dict(limits)
    if flags & 2:
        rig.eng.log_sizes_enable(16)
        sizes = {i: 3 + i % 5 for i in range(64)}
        cum = np.cumsum([0] + [sizes[i] for i in range(1, 64)])
        lsz = np.zeros(G_BIG * 16, dtype=rig.E.LOG_SIZE_DTYPE)
        k = 0
        for g in range(G_BIG):
            hi = int(rig.st["term_hi"][g])
            for i in range(max(1, hi - 15), hi + 1):
                lsz[k] = (g, i, int(cum[i]))
                k += 1
        rig.eng.log_sizes_write(lsz[:k])
        kw.update(sizes=sizes, esz_w=16)
    whole = rig.expect()[3]
    answers, items = run_against_model(rig, dense, limits=kw, max_entries=max_entries, flags=flags)
    cut = [k for k in items if items[k][0] == CM.SEND_APPEND and items[k][2] < whole[k][2]]
    assert bool(cut) == (limits.get("max_bytes") != (1 << 64) - 1)
    rig.close()


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("short", [None, 0, 1])
def test_item_cap(rg, dense, short):
    """*count with item_cap 0, exact and one short: the total is reported, only item_cap items are written, nothing beyond"""
    rig = Rig(rg, 5, 8)
    items = rig.expect(rig.sparse(rig.recs))[3]
    room = 0 if short == 0 else len(items) - (short or 0)
    assert len(items) >= 2
    want, win, answers, items, cells = rig.expect(rig.recs if dense else rig.sparse(rig.recs))
    got_answers, got_items, total = rig.apply(rig.recs if dense else rig.sparse(rig.recs), dense, item_cap=room)
    assert total == len(items) and len(got_items) == room
    rig.check(want, win, answers, items, cells, got_answers, got_items, total)
    rig.close()


@pytest.mark.parametrize("item_cap", [0, 8])
@pytest.mark.parametrize("cap", [0, 8])
@pytest.mark.parametrize("dense", [False, True])
def test_status_outcomes_leave_a_byte_identical_engine(rg, dense, cap, item_cap):
    """Every status but STARTED, and SELF with a previous transfer: rg_read_groups, the Inflights dump, every column and the clock
    cells before and after are the same bytes -- IN_PROGRESS does not reset the election counter"""
    cases = [c for c in M.edge_cases(5) if c[4] != M.STARTED and c[0] != "to_self_previous"]
    rig = Rig(rg, 5, cap, cases=cases)
    recs = rig.recs if dense else rig.sparse(rig.recs)
    before = rig.snapshot()
    want, win, answers, items, cells = rig.expect(recs)
    assert {a["status"] for a in answers} == ALL_STATUSES - {M.STARTED} and not items
    got_answers, got_items, total = rig.apply(recs, dense, item_cap=item_cap if cap else None)
    for a, b in zip(answers, got_answers):
        assert {k: a[k] for k in b} == b, (a, b)
    assert total == 0 and rig.same(before, rig.snapshot())
    rig.close()


@pytest.mark.parametrize("cap", [0, 8])
def test_dense_and_sparse_agree_and_nothing_selected_writes_status_only(rg, cap):
    a, b = Rig(rg, 5, cap), Rig(rg, 5, cap)
    recs = a.sparse(a.recs)
    ra, ia, ta = a.apply(recs, False)
    rb, ib, tb = b.apply(recs, True)
    assert a.same(a.snapshot(), b.snapshot()) and a.read_windows() == b.read_windows()
    assert ta == tb and sendstage.items_dict(ia) == sendstage.items_dict(ib)
    assert [{k: x[k] for k in y} for x, y in zip(ra, rb)] == rb
    before = b.snapshot()
    _, items, total = b.apply([], True)  # (Rig.apply checks the status bytes, the untouched events cells and the canaries)
    assert total == 0 and b.same(before, b.snapshot())
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------------
# the clock
# ---------------------------------------------------------------------------------------------------------------------
def clock_rig(rg, dense_groups=()):
    """three quiet 3-slot groups with a lagging slot 2, election_tick 10, heartbeat_tick 3"""
    cases = [("lagging", M.make_group(3, 0b111, match=[20, 20, 12]), 2, {}, M.STARTED)] * 3
    return Rig(rg, 3, 0, cases=cases)


def set_elapsed(rig, g, el, hb=0):
    w = np.zeros(1, dtype=rig.E.LEAD_CLOCK_CELL_DTYPE)
    w[0] = (g, int(rig.st["cur_term"][g]), el, hb, 1, [0] * 7)
    rig.eng.lead_clock_write(w)


def clock_events(rig, g, n):
    import torch
    events = torch.zeros(rig.G, dtype=torch.uint8, device="cuda")
    out = []
    for _ in range(n):
        rig.eng.lead_clock(events)
        out.append(int(events.cpu().numpy()[g]))
    return out


@pytest.mark.parametrize("dense", [False, True])
def test_the_clock_with_an_equal_tag(rg, dense):
    """test_leader_transfer_timeout: election_elapsed = 9 of 10, then the transfer: the counter starts again -- one rgx_lead_clock
    reports no TRANSFER_ABORTED and the cell reads 1, nine more report it exactly on the ninth, and the bits are clear"""
    rig = clock_rig(rg)
    E, g = rig.E, rig.groups[0]
    set_elapsed(rig, g, 9)
    got, _, _ = rig.apply([(g, 2)], dense)
    assert got[0]["status"] == M.STARTED and got[0]["events"] == M.EV_APPEND
    first = clock_events(rig, g, 1)
    assert not first[0] & E.LEAD_EV_TRANSFER_ABORTED and int(rig.eng.lead_clock_read([g])[0]["election_elapsed"]) == 1
    assert M.fields(int(rig.read()["cfg"][g]))[3] == 3
    more = clock_events(rig, g, 9)
    assert [bool(e & E.LEAD_EV_TRANSFER_ABORTED) for e in more] == [False] * 8 + [True]
    assert M.fields(int(rig.read()["cfg"][g]))[3] == 0
    rig.close()


@pytest.mark.parametrize("dense", [False, True])
def test_in_progress_does_not_reset_the_counter(rg, dense):
    """the same sequence with a repeated request at election_elapsed = 5: it still aborts at the original time"""
    rig = clock_rig(rg)
    E, g = rig.E, rig.groups[0]
    set_elapsed(rig, g, 9)
    assert rig.apply([(g, 2)], dense)[0][0]["status"] == M.STARTED
    assert not any(e & E.LEAD_EV_TRANSFER_ABORTED for e in clock_events(rig, g, 5))
    assert int(rig.eng.lead_clock_read([g])[0]["election_elapsed"]) == 5
    cell = rig.eng.lead_clock_read([g]).tobytes()
    assert rig.apply([(g, 2)], dense)[0][0]["status"] == M.IN_PROGRESS
    assert rig.eng.lead_clock_read([g]).tobytes() == cell
    more = clock_events(rig, g, 5)
    assert [bool(e & E.LEAD_EV_TRANSFER_ABORTED) for e in more] == [False] * 4 + [True]
    assert M.fields(int(rig.read()["cfg"][g]))[3] == 0
    rig.close()


@pytest.mark.parametrize("dense", [False, True])
def test_the_clock_with_a_different_tag_and_a_stopped_group(rg, dense):
    """RG_COL_CUR_TERM bumped by rg_load_column without a clock call: a leadership the clock has not armed. The transfer leaves the
    cell byte-identical and the next rgx_lead_clock reports NEW_TERM with both counters at 1. A stopped group gets NOT_LED."""
    rig = clock_rig(rg)
    E, (g, s, _) = rig.E, rig.groups
    set_elapsed(rig, g, 7, 2)
    w = np.zeros(1, dtype=E.LEAD_CLOCK_CELL_DTYPE)
    w[0] = (s, int(rig.st["cur_term"][s]), 0, 0, 0, [0] * 7)
    rig.eng.lead_clock_write(w)
    term = rig.st["cur_term"].copy()
    term[g] += 1
    rig.eng.load_column(E.COL.NAMES.index("cur_term"), term)
    cell = rig.eng.lead_clock_read([g, s]).tobytes()
    before = rig.read()
    got, _, _ = rig.apply([(g, 2), (s, 2)], dense)
    assert got[0]["status"] == M.STARTED and got[1]["status"] == M.NOT_LED
    assert rig.eng.lead_clock_read([g, s]).tobytes() == cell
    after = rig.read()
    assert M.fields(int(after["cfg"][g]))[3] == 3
    after["cfg"][g] = before["cfg"][g]
    assert not R.diff(before, after, cols=READ_COLS)
    ev = clock_events(rig, g, 1)[0]
    c = rig.eng.lead_clock_read([g])[0]
    assert ev & E.LEAD_EV_NEW_TERM and (int(c["election_elapsed"]), int(c["heartbeat_elapsed"]), int(c["term"])) == (1, 1, int(term[g]))
    rig.close()


# ---------------------------------------------------------------------------------------------------------------------
# life after the call
# ---------------------------------------------------------------------------------------------------------------------
def test_the_tick_sends_timeout_now_once_the_transferee_catches_up(rg):
    """test_leader_transfer_to_slow_follower: a transfer to a lagging peer, then a tick carrying that peer's ack at last_index, gives
    RG_OUT_TIMEOUT_NOW from the tick; the bits are still set afterwards"""
    rig = clock_rig(rg)
    g = rig.groups[0]
    got, _, _ = rig.apply([(g, 2)], False)
    assert got[0]["status"] == M.STARTED and got[0]["events"] == M.EV_APPEND and got[0]["matched"] == 12 and got[0]["last_index"] == 20
    msgs = rig.rg.MsgBuffers(rig.G, 3, rig.eng.stride)
    msgs.m_flags[g, 2] = 0x01
    msgs.m_index[2, g] = 20
    rig.eng.tick(msgs)
    after = rig.read()
    assert int(after["out"][g]) & rig.E.OUT.TIMEOUT_NOW and M.fields(int(after["cfg"][g]))[3] == 3
    assert not any(int(after["out"][x]) & rig.E.OUT.TIMEOUT_NOW for x in range(rig.G) if x != g)
    rig.close()


def test_removing_the_transferee_aborts_the_transfer(rg):
    """test_leader_transfer_remove_node: rgc_apply_conf removing the transferee reports RGC_CONF_EV_TRANSFER_ABORTED"""
    rig = clock_rig(rg)
    E, g = rig.E, rig.groups[0]
    assert rig.apply([(g, 2)], True)[0][0]["status"] == M.STARTED
    recs = np.zeros(1, dtype=E.CONF_REC_DTYPE)
    recs[0]["group"], recs[0]["cfg"] = g, CM.word(0b011)
    resp, _, _ = rig.eng.apply_conf(recs)
    assert int(resp[0]["status"]) == E.CONF_DONE and int(resp[0]["events"]) & E.CONF_EV_TRANSFER_ABORTED
    assert M.fields(int(rig.read()["cfg"][g]))[3] == 0
    rig.close()


def test_a_tick_with_its_send_stage_after_a_transfer_equals_the_oracle(rg):
    """rg_tick_device_send behind a STARTED call against the oracle loaded with what the call left and stepped the same way: every
    column, every result word, the items"""
    P, cap, G = 5, 8, G_BIG
    rig = Rig(rg, P, cap, cases=[c for c in M.edge_cases(P) if c[4] == M.STARTED])
    quiet = M.make_group(P, (1 << P) - 1, match=[20] * P)  # every other group a quiet leader of the same term
    for g in range(G):
        if g not in rig.groups:
            R.put_lead(rig.st, g, quiet)
    for k in CG.LOAD_COLS:
        rig.eng.load_column(rig.E.COL.NAMES.index(k), rig.st[k])
    answers, items = run_against_model(rig, True)
    assert all(a["status"] == M.STARTED for a in answers)
    msgs = rig.rg.MsgBuffers(G, P, rig.eng.stride)
    m = msgs.as_dict()
    got = rig.read()
    for g in range(G):  # every peer of every group acks everything it was sent so far
        present, self_slot = int(got["cfg"][g]) >> 24, int(got["cfg"][g]) >> 16 & 7
        for s in range(P):
            if present >> s & 1 and s != self_slot and int(got["next"][s, g]) - 1 <= int(got["term_hi"][g]):
                m["m_flags"][g, s] = 0x01
                m["m_index"][s, g] = int(got["next"][s, g]) - 1
    cl = O.Cluster(G)
    ost = R.copy_state(got)
    cl.load_soa(ost, term=3, max_inflight=cap)
    cl.set_own_inflights(True)
    for (g, s), entries in rig.read_windows().items():
        for e in entries:
            cl.L.ro_ins_add(ctypes.byref(cl.L.ro_group_progress(cl.h, g, s + 1).contents.ins), e)
    gout = np.zeros(G, dtype=np.uint32)
    cl.tick_soa(m, gout)
    sent = cl.send_stage_soa(gout, 0)
    cl.store_soa(ost)
    rig.eng.tick_send(msgs)
    after = rig.read()
    d = R.diff(ost, after, cols=O.STATE_COLS)
    assert not d, d
    assert (after["out"] == gout).all() and (gout & rig.E.OUT.TIMEOUT_NOW).any()
    sendstage.compare_items(rig.eng.send_items(), sent)
    rig.close()


@pytest.mark.parametrize("cap", [0, 8])
def test_old_road_and_new_road_leave_identical_columns(rg, cap):
    """The host route -- rg_read_groups, rg_set_config with the transferee field, rgx_lead_clock_write with election_elapsed 0, then
    the transferee's cells and window as the model's single maybe_send_append leaves them (rg_write_cells, rg_load_inflights) --
    against ONE rgm_transfer_leader on a second engine: every column, every window, every clock cell"""
    cases = [c for c in M.edge_cases(5) if c[4] == M.STARTED]
    old, new = Rig(rg, 5, cap, cases=cases), Rig(rg, 5, cap, cases=cases)
    want, win, answers, items, cells = new.expect()
    got_answers, got_items, total = new.apply(new.recs, False)
    new.check(want, win, answers, items, cells, got_answers, got_items, total)
    status = old.eng.read_groups(np.array([g for g, _ in old.recs], dtype=np.uint64))
    clock = old.eng.lead_clock_read([g for g, _ in old.recs])
    meta = ring = None
    if cap:
        meta, ring = old.eng.read_inflights()
    for k, (g, t) in enumerate(old.recs):
        cfg = int(status[k]["cfg"])
        old.eng.set_config(g, (cfg & ~M.TRANSFEREE_BITS) | (t + 1) << 20)
        clock[k]["election_elapsed"] = 0
        if cap:
            old.eng.write_cells([{"group": g, "slot": t, "next": int(want["next"][t, g]), "pflags": int(want["pflags"][g, t])}])
            entries = win.get((g, t), [])
            meta[t, g] = len(entries) << 16
            ring[g, t, :len(entries)] = entries
    old.eng.lead_clock_write(clock)
    if cap:
        old.eng.load_inflights(meta, ring)
    d = R.diff(old.read(), new.read(), cols=READ_COLS)
    assert not d, d
    assert old.read_windows() == new.read_windows() and old.clock_cells().tobytes() == new.clock_cells().tobytes()
    old.close()
    new.close()


# ---------------------------------------------------------------------------------------------------------------------
# API states
# ---------------------------------------------------------------------------------------------------------------------
def test_api_states(rg):
    """What the two calls refuse on a live engine, and that a refused call changes nothing: unknown flags, RG_SEND_BYTES without the
    size table, item arguments on an engine without device Inflights, a NULL count on one with them, bad records (a group beyond the
    shard, a group twice, a slot beyond the slot count, a non-zero reserved), a missing pointer, a send stage that is still owed,
    ingested records, groups that carry RG_OUT_HOST_HINT, a host mirror."""
    E = rg.engine

    def code(call):
        with pytest.raises(rg.EngineError) as ei:
            call()
        return ei.value.code

    for cap in (0, 8):
        d = M.make_group(3, 0b111, match=[20, 8, 12], dummy=2, lo=15)  # (the run table starts at 10: the terms of 3..9 are the host's)
        d["run_first"], d["pflags"][1], d["next"][1] = [10] + [0] * 7, CM.PROBE | CM.PF_RECENT_ACTIVE, 12
        rig = Rig(rg, 3, cap, cases=[("lagging", d, 2, {}, M.STARTED)] * 3)
        g = rig.groups[0]
        good = rig.rec_array([(g, 2)])
        before = rig.snapshot()
        to, status = dev(np.zeros(rig.G, np.uint8)), dev(np.zeros(rig.G, np.uint8))
        count = dev(np.zeros(2, np.uint32)) if cap else None
        both = (lambda: rig.eng.transfer_leader(good), lambda: rig.eng.transfer_leader_device(to, status, count=count))
        assert code(lambda: rig.eng.transfer_leader(good, flags=1)) == E.ERR["INVALID_ARG"]  # RG_SEND_SKIP_BCAST_COMMIT is not this call's
        assert code(lambda: rig.eng.transfer_leader_device(to, status, count=count, flags=8)) == E.ERR["INVALID_ARG"]
        assert code(lambda: rig.eng.transfer_leader(good, flags=2)) == E.ERR["STATE"]  # RG_SEND_BYTES without rg_log_sizes_enable
        assert code(lambda: rig.eng.transfer_leader_device(to, status, count=count, flags=2)) == E.ERR["STATE"]
        assert code(lambda: rig.eng.transfer_leader_device(to, None, count=count)) == E.ERR["INVALID_ARG"]
        assert code(lambda: rig.eng.transfer_leader_device(None, status, count=count)) == E.ERR["INVALID_ARG"]
        for bad in ([(rig.G, 1)], [(g, 1), (g, 2)], [(g, 3)], [(g, 254)]):
            assert code(lambda: rig.eng.transfer_leader(rig.rec_array(bad))) == E.ERR["INVALID_ARG"], bad
        reserved = good.copy()
        reserved["reserved"] = 1
        assert code(lambda: rig.eng.transfer_leader(reserved)) == E.ERR["INVALID_ARG"]
        if not cap:  # item arguments on an engine without device Inflights
            n = ctypes.c_uint64(0)
            items = np.zeros(4, dtype=E.SEND_ITEM_DTYPE)
            resp = np.zeros(1, dtype=E.TRANSFER_RESP_DTYPE)
            assert rig.eng.L.rgm_transfer_leader(rig.eng.h, good.ctypes.data, 1, resp.ctypes.data, 0, 0, items.ctypes.data, 4, ctypes.byref(n)) == E.ERR["INVALID_ARG"]
            assert code(lambda: rig.eng.transfer_leader_device(to, status, count=dev(np.zeros(2, np.uint32)))) == E.ERR["INVALID_ARG"]
        else:
            assert code(lambda: rig.eng.transfer_leader_device(to, status, items=None, item_cap=4, count=count)) == E.ERR["INVALID_ARG"]
            assert code(lambda: rig.eng.transfer_leader_device(to, status)) == E.ERR["INVALID_ARG"]  # (no count word)
            resp = np.zeros(1, dtype=E.TRANSFER_RESP_DTYPE)
            assert rig.eng.L.rgm_transfer_leader(rig.eng.h, good.ctypes.data, 1, resp.ctypes.data, 0, 0, None, 0, None) == E.ERR["INVALID_ARG"]  # (no n_items)
        rig.eng.sync()
        assert rig.same(before, rig.snapshot())
        # ingested records that are not ticked yet
        rec = np.zeros(1, dtype=E.WIRE_DTYPE)
        rec[0]["group"], rec[0]["index"], rec[0]["slot"], rec[0]["flags"] = rig.groups[1], 12, 2, 0x01
        assert rig.eng.ingest(rec) == 0
        assert all(code(c) == E.ERR["STATE"] for c in both)
        assert rig.eng.tick_ingested() == 1
        if cap:
            rig.eng.send_appends()
        # a tick whose send stage is still owed (device Inflights), and a group that carries RG_OUT_HOST_HINT (both engines): a reject
        # whose find_conflict_by_term walk needs terms below the device's run table
        msgs = rig.rg.MsgBuffers(rig.G, 3, rig.eng.stride)
        h = rig.groups[2]
        msgs.m_flags[h, 1], msgs.m_index[1, h], msgs.m_hint[1, h], msgs.m_logterm[1, h] = 0x83, 11, 5, 1
        rig.eng.tick(msgs)
        after_tick = rig.snapshot()
        assert int(after_tick[2]["out"][h]) & E.OUT.HOST_HINT
        if cap:  # (an engine without device Inflights has no send requests to hold back: a hint does not stop its next step)
            assert all(code(c) == E.ERR["STATE"] for c in both)  # the stage is owed
            rig.eng.send_appends()
            after_tick = rig.snapshot()
            for c in both:  # the hint is not answered
                with pytest.raises(rg.EngineError) as ei:
                    c()
                assert ei.value.code == E.ERR["STATE"] and "rg_resolve_host_hints" in str(ei.value)
            assert rig.same(after_tick, rig.snapshot())
            assert rig.eng.resolve_host_hints([(h, 11, 2, 1, 0)]).all()
        resp, items, total = rig.eng.transfer_leader(good[:0])  # no record: nothing to do
        assert len(resp) == 0 and total == 0
        # ... and the engine is still usable: the good record goes through
        resp, items, total = rig.eng.transfer_leader(good)
        assert int(resp[0]["status"]) == M.STARTED
        # a host mirror: both forms are refused
        for grp in range(rig.G):
            rig.eng.set_peers(grp, [101, 102, 103], 3)
        assert all(code(c) == E.ERR["STATE"] for c in both)
        rig.close()
