"""GPU: the batched conf change (rgc_apply_conf / rgc_apply_conf_device) against tests/conf_model.py -- every column of every
group, every window, the answers and the item set, exactly -- on an engine of 300 groups (two 256-thread blocks, the second partial;
class blocks of 64, the last partial), of 1 and of 65 groups; slot counts 1, 3, 5 and 8, max_inflight 0, 1 and 8, 32- and 64-bit cell
offsets (RG_CFGF_IX64 forces the 64-bit instantiations at this size). No test provokes a device fault: every bad argument is
refused on the host, every bad dense cell is an ANSWER."""
import ctypes

import numpy as np
import pytest

import conf_model as M
import handoff_rig as R
import oracle_lib as O
import sendstage

pytestmark = pytest.mark.gpu

LOAD_COLS = O.STATE_COLS + O.TERM_TABLE_COLS + ("out",)
READ_COLS = R.ALL_COLS + ("out", "host_hint")
LANES_BOTH = (0, 63, 64, 255, 256, 299)
CANARY = 0x7E
G_BIG = 300


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def lanes_for(n, G, tail):
    """n distinct groups: the edge lanes first (tail: none of the first block, so that its workgroup leaves at its barrier)"""
    if G <= 256:
        first = [g for g in (0, G - 1, 63, 64) if g < G]
        rest = [g for g in range(G) if g not in first]
        return (list(dict.fromkeys(first)) + rest)[:n]
    first = [g for g in LANES_BOTH if not tail or g >= 256]
    rest = [g for g in range(256 if tail else 1, G) if g not in first]
    return (first + rest)[:n]


class Rig:
    def __init__(self, rg, P, cap, G=G_BIG, ix64=False, cases=None, tail=False, clock=False, **kw):
        self.rg, self.E, self.P, self.G, self.cap = rg, rg.engine, P, G, cap
        self.eng = rg.Engine(G, P, flags=self.E.CFGF.IX64 if ix64 else None, max_inflight=cap, **kw)
        self.cases = M.edge_cases(P) if cases is None else cases
        n = min(len(self.cases), G)
        self.cases = self.cases[:n]
        self.groups = lanes_for(n, G, tail)
        self.st = R.base_state(G, P, self.eng.stride)
        self.windows = {} if cap else None
        for g, (name, d, W, win, expect) in zip(self.groups, self.cases):
            R.put_lead(self.st, g, d)
            for s, shape in (win.items() if cap else ()):
                self.windows[(g, s)] = M.window_entries(shape, cap, d["match"][s])
        for k in LOAD_COLS:
            self.eng.load_column(self.E.COL.NAMES.index(k), self.st[k])
        if cap:
            meta, ring = np.zeros((P, self.eng.stride), dtype=np.uint32), np.zeros((G, P, cap), dtype=np.uint64)
            for (g, s), entries in self.windows.items():
                meta[s, g] = len(entries) << 16
                ring[g, s, :len(entries)] = entries
            self.eng.load_inflights(meta, ring)
        self.led = None
        if clock:
            self.eng.lead_clock_enable(10, 3, self.E.LEAD_CLOCK_START_LED)
            self.led = {}
        self.recs = [(g, c[2]) for g, c in zip(self.groups, self.cases)]

    def close(self):
        self.eng.sync()
        self.eng.close()

    def read(self):
        st = {"n_groups": self.G, "n_slots": self.P, "stride": self.eng.stride}
        for k in READ_COLS:
            st[k] = self.eng.read_column(self.E.COL.NAMES.index(k))
        return st

    def read_windows(self):
        if not self.cap:
            return None
        meta, ring = self.eng.read_inflights()
        return {(g, s): self.eng.inflights(g, s, meta, ring) for g in range(self.G) for s in range(self.P)}

    def expect(self, recs=None, **limits):
        """the model over what was loaded -> (state, windows, answers, items)"""
        win = None if self.windows is None else {k: list(v) for k, v in self.windows.items()}
        st = R.copy_state(self.st)
        st["host_hint"] = np.zeros(self.G, dtype=np.uint8)
        want, answers, items = M.apply_state(st, win, self.recs if recs is None else recs, self.cap, led=self.led, **limits)
        return want, win, answers, items

    def rec_array(self, recs):
        a = np.zeros(len(recs), dtype=self.E.CONF_REC_DTYPE)
        for k, (g, W) in enumerate(recs):
            a[k]["group"], a[k]["cfg"] = g, W
        return a

    def apply(self, recs, dense, item_cap=None, max_entries=0, flags=0):
        """-> (answers as dicts: sparse every field, dense status / events / commit; the items written; the total)"""
        import torch
        if not dense:
            resp, items, total = self.eng.apply_conf(self.rec_array(recs), max_entries, flags, item_cap if self.cap else None)
            return [{k: int(r[k]) for k in resp.dtype.names} for r in resp], items, total
        sel, cfg = np.zeros(self.G, np.uint8), np.full(self.G, 0xA5A5A5A5, np.uint32)  # (an unselected word is never read: it is malformed)
        for g, W in recs:
            sel[g], cfg[g] = 1 + g % 255, W
        status = torch.full((self.G + 64,), CANARY, dtype=torch.uint8, device="cuda")
        events = torch.full((self.G + 64,), CANARY, dtype=torch.uint8, device="cuda")
        commit = torch.full((self.G + 64,), -1, dtype=torch.int64, device="cuda")
        room = len(recs) * self.P if item_cap is None else item_cap
        buf = count = None
        if self.cap:
            buf = torch.full(((room + 2) * 32,), CANARY, dtype=torch.uint8, device="cuda")  # two items of canary behind item_cap
            count = torch.full((2,), 0x55555555, dtype=torch.int32, device="cuda")
        cols = (dev(sel), dev(cfg))
        self.eng.apply_conf_device(cols[0], cols[1], status, events, commit, buf if room and self.cap else None, room if self.cap else 0, count, max_entries, flags)
        self.eng.sync()
        status, events, commit = status.cpu().numpy(), events.cpu().numpy(), commit.cpu().numpy().view(np.uint64)
        assert (status[self.G:] == CANARY).all() and (events[self.G:] == CANARY).all()
        picked = {g for g, _ in recs}
        for g in range(self.G):
            if g not in picked:
                assert status[g] == M.NONE and events[g] == CANARY and int(commit[g]) == (1 << 64) - 1, g
        answers = [{"status": int(status[g]), "events": int(events[g]), "commit": int(commit[g])} for g, _ in recs]
        if not self.cap:
            return answers, np.zeros(0, dtype=self.E.SEND_ITEM_DTYPE), 0
        total = int(count.cpu().numpy().view(np.uint32)[0])
        assert int(count.cpu().numpy().view(np.uint32)[1]) == 0x55555555
        raw = buf.cpu().numpy()
        assert (raw[room * 32:] == CANARY).all(), "nothing is written beyond item_cap"
        k = min(total, room)
        assert (raw[k * 32:room * 32] == CANARY).all()
        return answers, raw[:k * 32].view(self.E.SEND_ITEM_DTYPE).copy(), total

    def check(self, want, win, answers, items, got_answers, got_items, total):
        for a, b in zip(answers, got_answers):
            assert {k: a[k] for k in b} == b, (a, b)
        got = self.read()
        d = R.diff(want, got, cols=READ_COLS)
        assert not d, d
        if self.cap:
            now = self.read_windows()
            for k, v in now.items():
                assert v == win.get(k, []), (k, v, win.get(k))
        assert total == len(items), (total, len(items))
        if len(got_items) == total:
            assert sendstage.items_dict(got_items) == items
        else:
            assert all(items[k] == v for k, v in sendstage.items_dict(got_items).items())


@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("cap", [0, 1, 8])
@pytest.mark.parametrize("P,ix64", [(1, False), (3, False), (3, True), (5, False), (5, True), (8, False)])
def test_both_forms_against_the_model(rg, P, ix64, cap, dense, tail):
    """The model's edge cases at lanes 0, 63, 64, 255, 256 and 299 -- and, tail, nowhere in the first block, whose workgroup then
    leaves at its barrier: every column, every window, the statuses, the events, the commit, the item set."""
    rig = Rig(rg, P, cap, ix64=ix64, tail=tail)
    recs = rig.recs
    if not dense:  # (the sparse form refuses a malformed word on the host: those records go to the dense form only)
        recs = [(g, W) for g, W in recs if not M.word_check(W, P)]
    want, win, answers, items = rig.expect(recs)
    got_answers, got_items, total = rig.apply(recs, dense)
    rig.check(want, win, answers, items, got_answers, got_items, total)
    if P > 1:
        assert {a["status"] for a in answers} >= {M.DONE, M.DEMOTED, M.HOST, M.FAULT}
        assert (cap == 0) == (not items)
    rig.close()


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("G", [1, 65])
def test_one_group_and_sixty_five(rg, G, dense):
    rig = Rig(rg, 3, 4, G=G)
    recs = [(g, W) for g, W in rig.recs if dense or not M.word_check(W, 3)]
    want, win, answers, items = rig.expect(recs)
    got_answers, got_items, total = rig.apply(recs, dense)
    rig.check(want, win, answers, items, got_answers, got_items, total)
    rig.close()


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("limits,max_entries,flags", [({"max_entries": 1}, 1, 0), ({"max_entries": 0}, 0, 1), ({"max_bytes": 9}, 9, 2), ({"max_bytes": (1 << 64) - 1}, (1 << 64) - 1, 2),
                                                     ({"max_bytes": 0}, 0, 2)])
def test_limits_and_flags(rg, limits, max_entries, flags, dense):
    """max_entries_per_msg, RG_SEND_SKIP_BCAST_COMMIT (accepted, no effect) and RG_SEND_BYTES over a size window of 16 entries -- a
    peer that needs more of them is the host's (RG_SEND_HOST)"""
    rig = Rig(rg, 5, 8)
    recs = [(g, W) for g, W in rig.recs if not M.word_check(W, 5)]
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
    want, win, answers, items = rig.expect(recs, **kw)
    got_answers, got_items, total = rig.apply(recs, dense, max_entries=max_entries, flags=flags)
    rig.check(want, win, answers, items, got_answers, got_items, total)
    if flags & 2 and limits["max_bytes"] != (1 << 64) - 1:
        assert any(v[0] == M.SEND_HOST for v in items.values())
    rig.close()


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("short", [None, 0, 1])
def test_item_cap(rg, dense, short):
    """*count with item_cap 0, exact and one short: the total is reported, only item_cap items are written, nothing beyond"""
    rig = Rig(rg, 5, 8)
    recs = [(g, W) for g, W in rig.recs if not M.word_check(W, 5)]
    want, win, answers, items = rig.expect(recs)
    room = 0 if short == 0 else len(items) - (short or 0)
    got_answers, got_items, total = rig.apply(recs, dense, item_cap=room)
    assert total == len(items) and len(got_items) == room
    rig.check(want, win, answers, items, got_answers, got_items, total)
    rig.close()


@pytest.mark.parametrize("cap", [0, 8])
@pytest.mark.parametrize("dense", [False, True])
def test_refusals_leave_a_byte_identical_engine(rg, dense, cap):
    """FAULT (a malformed word in the dense form; a self slot without a Progress in both), NOT_LED with the clock enabled, HOST:
    rg_read_groups and the Inflights dump before and after are the same bytes"""
    cases = [c for c in M.edge_cases(5) if c[4] in (M.FAULT, M.HOST)] + [c for c in M.edge_cases(5) if c[0] in ("add_node", "remove_commits")]
    rig = Rig(rg, 5, cap, cases=cases, clock=True)
    not_led = rig.groups[-2:]
    cells = np.zeros(2, dtype=rig.E.LEAD_CLOCK_CELL_DTYPE)
    for k, g in enumerate(not_led):
        cells[k]["group"], cells[k]["term"], cells[k]["led"] = g, int(rig.st["cur_term"][g]), 0
        rig.led[g] = False
    rig.eng.lead_clock_write(cells)
    recs = [(g, W) for g, W in rig.recs if dense or not M.word_check(W, 5)]
    everyone = np.arange(rig.G, dtype=np.uint64)
    before = (rig.eng.read_groups(everyone).tobytes(), [a.tobytes() for a in rig.eng.read_inflights()] if cap else None, rig.read())
    want, win, answers, items = rig.expect(recs)
    assert {a["status"] for a in answers} == {M.FAULT, M.HOST, M.NOT_LED} and not items
    got_answers, got_items, total = rig.apply(recs, dense)
    for a, b in zip(answers, got_answers):
        assert {k: a[k] for k in b} == b, (a, b)
    assert total == 0
    after = (rig.eng.read_groups(everyone).tobytes(), [a.tobytes() for a in rig.eng.read_inflights()] if cap else None, rig.read())
    assert before[0] == after[0] and before[1] == after[1] and not R.diff(before[2], after[2], cols=READ_COLS)
    rig.close()


@pytest.mark.parametrize("cap", [0, 8])
def test_dense_and_sparse_agree_and_nothing_selected_writes_status_only(rg, cap):
    a, b = Rig(rg, 5, cap), Rig(rg, 5, cap)
    recs = [(g, W) for g, W in a.recs if not M.word_check(W, 5)]
    ra, ia, ta = a.apply(recs, False)
    rb, ib, tb = b.apply(recs, True)
    assert not R.diff(a.read(), b.read(), cols=READ_COLS) and a.read_windows() == b.read_windows()
    assert ta == tb and sendstage.items_dict(ia) == sendstage.items_dict(ib)
    assert [{k: x[k] for k in y} for x, y in zip(ra, rb)] == rb
    before = (b.read(), b.read_windows())
    _, items, total = b.apply([], True)  # (Rig.apply checks the status bytes, the untouched events / commit cells and the canaries)
    assert total == 0 and not R.diff(before[0], b.read(), cols=READ_COLS) and before[1] == b.read_windows()
    a.close()
    b.close()


def test_old_road_and_new_road_leave_identical_columns(rg):
    """rg_set_config + rg_write_cells + rg_recompute against rgc_apply_conf on an engine without device Inflights"""
    cases = [c for c in M.edge_cases(5) if c[4] == M.DONE and not M.fields(c[1]["cfg"])[3]]
    old, new = Rig(rg, 5, 0, cases=cases), Rig(rg, 5, 0, cases=cases)
    new.apply(new.recs, False)
    for g, W in old.recs:
        cfg, hi = int(old.st["cfg"][g]), int(old.st["term_hi"][g])
        added = (W >> 24) & ~(cfg >> 24) & 0xFF
        old.eng.set_config(g, (W & M.FIELDS) | (cfg & M.KEPT))
        cells = [{"group": g, "slot": s, "match": 0, "next": hi + 1, "pr_commit": 0, "pend_snap": 0, "pend_rs": 0, "gid": 0, "pflags": M.PROBE | M.PF_RECENT_ACTIVE}
                 for s in range(5) if added >> s & 1]
        if cells:
            old.eng.write_cells(cells)
    old.eng.recompute()
    # (rg_recompute walks the whole shard: the groups nobody changed move too, where their loaded commit index lags their quorum. The
    # same sweep over the new road's engine moves those alike and finds nothing left to do in the changed groups)
    new.eng.recompute()
    a, b = old.read(), new.read()
    picked = [g for g, _ in old.recs]
    assert not b["out"][picked].any() and a["out"][picked].any()
    b["out"][picked] = a["out"][picked]  # (the old road's result words; the new call answers in its response instead)
    d = R.diff(a, b, cols=READ_COLS)
    assert not d, d
    old.close()
    new.close()


def test_a_tick_with_its_send_stage_after_a_change_equals_the_oracle(rg):
    """The layers behind it: rg_tick_device_send after a change against the oracle loaded with the change applied -- every column
    and every result word; and rg_size_classes after growing 3-slot groups to 5 slots reports the frayed block."""
    import fuzz
    P, cap, G = 5, 8, G_BIG
    cases = [("grow", M.make_group(P, 0b00111), M.word(0b11111), {}, M.DONE)] * 6
    rig = Rig(rg, P, cap, cases=cases)
    # every group a 3-slot group first: the class table then holds 3-slot blocks
    st = rig.st
    three = M.make_group(P, 0b00111)
    for g in range(G):
        R.put_lead(st, g, three)
    for k in LOAD_COLS:
        rig.eng.load_column(rig.E.COL.NAMES.index(k), st[k])
    rig.windows = {}
    before_classes = rig.eng.size_classes()
    want, win, answers, items = rig.expect()
    got_answers, got_items, total = rig.apply(rig.recs, True)
    rig.check(want, win, answers, items, got_answers, got_items, total)
    # a tick: every peer of every group acks everything it was sent so far
    msgs = rig.rg.MsgBuffers(G, P, rig.eng.stride)
    m = msgs.as_dict()
    got = rig.read()
    for g in range(G):
        present = int(got["cfg"][g]) >> 24
        for s in range(1, P):
            if present >> s & 1:
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
    assert (after["out"] == gout).all()
    sendstage.compare_items(rig.eng.send_items(), sent)
    classes = rig.eng.size_classes()
    assert before_classes and classes != before_classes, (before_classes, classes)
    rig.close()


def test_add_node_check_quorum_with_the_leaders_clock(rg):
    """test_add_node_check_quorum (harness/tests/integration_cases/test_raft.rs) with rgx_lead_clock: the added peer comes in
    recent_active (tracker.rs:386-389), so the first election timeout's check-quorum does not step the leader down; the second,
    without an ack of that peer in between, does."""
    import torch
    E = rg.engine
    el = 4
    cases = [("add_to_one", M.make_group(3, 0b001, match=[20, 0, 0]), M.word(0b011), {}, M.DONE)]
    rig = Rig(rg, 3, 0, cases=cases)
    g = rig.groups[0]
    rig.eng.lead_clock_enable(el, 1, E.GATE_CHECK_QUORUM | E.LEAD_CLOCK_START_LED)
    rig.led = {}
    want, win, answers, items = rig.expect()
    got_answers, got_items, total = rig.apply(rig.recs, False)
    rig.check(want, win, answers, items, got_answers, got_items, total)
    events = torch.zeros(rig.G, dtype=torch.uint8, device="cuda")
    downs = []
    for t in range(2 * el):
        counts = rig.eng.lead_clock(events)
        downs.append(bool(int(events.cpu().numpy()[g]) & E.LEAD_EV_STEPPED_DOWN))
    assert not any(downs[:2 * el - 1]) and downs[2 * el - 1], downs
    assert int(rig.eng.lead_clock_read([g])[0]["led"]) == 0
    # ... and a stepped-down group is refused from then on
    got_answers, _, _ = rig.apply([(g, M.word(0b001))], True)
    assert got_answers[0]["status"] == M.NOT_LED
    rig.close()


def test_pending_reads_are_released_after_a_shrinking_change(rg):
    """The ReadIndex re-check of raft.rs:2648-2664 is the existing read call's: a read that waits for a second ack is released by
    RG_READ_ACK_LAST_SELF once the change has shrunk the quorum to the leader alone"""
    E = rg.engine
    d = M.make_group(3, 0b011, 0, 0b011, match=[20, 20, 0])
    cases = [("shrink", d, M.word(0b001), {}, M.DONE)]
    rig = Rig(rg, 3, 0, cases=cases)
    g = rig.groups[0]
    rig.eng.read_index_enable(4)
    assert list(rig.eng.read_index([(g, 77)])) == [E.READ_QUEUED]
    want, win, answers, items = rig.expect()
    got_answers, got_items, total = rig.apply(rig.recs, False)
    rig.check(want, win, answers, items, got_answers, got_items, total)
    assert got_answers[0]["status"] == M.DONE and int(rig.eng.read_pending_counts()[g]) == 1 and len(rig.eng.read_states()) == 0
    rig.eng.read_acks([(g, 0, 0, E.READ_ACK_LAST_SELF)])
    states = rig.eng.read_states()
    assert [(int(s["group"]), int(s["ctx"]), int(s["index"])) for s in states] == [(g, 77, 20)] and int(rig.eng.read_pending_counts()[g]) == 0
    rig.close()


def test_api_states(rg):
    """What the two calls refuse, and that a refused call changes nothing: unknown flags, RG_SEND_BYTES without the size table, item
    arguments on an engine without device Inflights, bad records (a group beyond the shard, a group twice, a non-zero reserved, a
    malformed word), a missing pointer, a send stage that is still owed, a host mirror."""
    E = rg.engine

    def code(call):
        with pytest.raises(rg.EngineError) as ei:
            call()
        return ei.value.code

    for cap in (0, 8):
        rig = Rig(rg, 3, cap)
        g = rig.groups[0]
        good = rig.rec_array([(g, M.word(0b011))])
        before = (rig.read(), rig.read_windows())
        sel, cfg = dev(np.zeros(rig.G, np.uint8)), dev(np.zeros(rig.G, np.uint32))
        status = dev(np.zeros(rig.G, np.uint8))
        count = dev(np.zeros(2, np.uint32)) if cap else None
        assert code(lambda: rig.eng.apply_conf(good, flags=4)) == E.ERR["INVALID_ARG"]
        assert code(lambda: rig.eng.apply_conf_device(sel, cfg, status, count=count, flags=8)) == E.ERR["INVALID_ARG"]
        assert code(lambda: rig.eng.apply_conf(good, flags=2)) == E.ERR["STATE"]  # RG_SEND_BYTES without rg_log_sizes_enable
        assert code(lambda: rig.eng.apply_conf_device(sel, cfg, status, count=count, flags=2)) == E.ERR["STATE"]
        assert code(lambda: rig.eng.apply_conf_device(sel, cfg, None, count=count)) == E.ERR["INVALID_ARG"]
        assert code(lambda: rig.eng.apply_conf_device(None, cfg, status, count=count)) == E.ERR["INVALID_ARG"]
        assert code(lambda: rig.eng.apply_conf_device(sel, None, status, count=count)) == E.ERR["INVALID_ARG"]
        for bad in ([(rig.G, M.word(1))], [(g, M.word(1)), (g, M.word(3))], [(g, M.word(1) | 1 << 16)], [(g, 1 << 24)], [(g, M.word(0b1011))], [(g, M.word(0b011, 0, 0b001))]):
            assert code(lambda: rig.eng.apply_conf(rig.rec_array(bad))) == E.ERR["INVALID_ARG"], bad
        reserved = good.copy()
        reserved["reserved"] = 1
        assert code(lambda: rig.eng.apply_conf(reserved)) == E.ERR["INVALID_ARG"]
        if not cap:  # item arguments on an engine without device Inflights
            n = ctypes.c_uint64(0)
            items = np.zeros(4, dtype=E.SEND_ITEM_DTYPE)
            resp = np.zeros(1, dtype=E.CONF_RESP_DTYPE)
            assert rig.eng.L.rgc_apply_conf(rig.eng.h, good.ctypes.data, 1, resp.ctypes.data, 0, 0, items.ctypes.data, 4, ctypes.byref(n)) == E.ERR["INVALID_ARG"]
            assert code(lambda: rig.eng.apply_conf_device(sel, cfg, status, count=dev(np.zeros(2, np.uint32)))) == E.ERR["INVALID_ARG"]
        else:  # a tick's send stage is still owed
            assert code(lambda: rig.eng.apply_conf_device(sel, cfg, status, items=None, item_cap=4, count=count)) == E.ERR["INVALID_ARG"]
            assert code(lambda: rig.eng.apply_conf_device(sel, cfg, status)) == E.ERR["INVALID_ARG"]  # (no count word)
            rig.eng.tick(rg.MsgBuffers(rig.G, 3, rig.eng.stride))
            after_tick = (rig.read(), rig.read_windows())
            assert code(lambda: rig.eng.apply_conf(good)) == E.ERR["STATE"] and code(lambda: rig.eng.apply_conf_device(sel, cfg, status, count=count)) == E.ERR["STATE"]
            assert not R.diff(after_tick[0], rig.read(), cols=READ_COLS) and after_tick[1] == rig.read_windows()
            rig.eng.send_appends()
            before = (rig.read(), rig.read_windows())
        rig.eng.sync()
        assert not R.diff(before[0], rig.read(), cols=READ_COLS) and before[1] == rig.read_windows()
        resp, items, total = rig.eng.apply_conf(good[:0])  # no record: nothing to do
        assert len(resp) == 0 and total == 0
        # ... and the engine is still usable: the good record goes through
        resp, items, total = rig.eng.apply_conf(good)
        assert int(resp[0]["status"]) == M.DONE
        # a host mirror: both forms are refused
        for grp in range(rig.G):
            rig.eng.set_peers(grp, [101, 102, 103], 3)
        assert code(lambda: rig.eng.apply_conf(good)) == E.ERR["STATE"] and code(lambda: rig.eng.apply_conf_device(sel, cfg, status, count=count)) == E.ERR["STATE"]
        rig.close()
