"""GPU: the leader's term gate (rgt_lead_gate_device) against tests/term_gate_model.py, cell for cell: the filtered flag rows, the
event column, new_term, the list of deposed groups and the three counts, the clock cells, the cfg words, the ReadIndex queues, and
every other column of the leader engine untouched -- at wave and block edges, for 1, 3 and 8 slots, both index widths, aliased and
not. Then the tick on the filtered rows against the oracle stepping only what the model lets through. No test provokes a device
fault: every bad argument used is one the host refuses."""
import random

import numpy as np
import pytest

import handoff_rig as R
import lead_clock_model as L
import readonly_model as RO
import term_gate_model as T
from test_follow_gate_gpu import device_u64
from test_handoff_gpu import LOAD_COLS, READ_COLS, dev

pytestmark = pytest.mark.gpu

CLOCK = L.Config(10, 3, L.CHECK_QUORUM)
EV_SENT, U64_SENT = 0xEE, 0xA5A5A5A5A5A5A5A5
DEPTH = 4


class GateRig:
    """A leader engine of G x P quiet leaders (handoff_rig.base_state) whose terms, transferees and clock cells are the model's:
    led, stopped, or tagged with an older term; optionally the ReadIndex layer with one read pending in every group that can
    queue one."""

    def __init__(self, rg, G, P, ix64=False, reads=False, seed=1, terms=True, transferees=True, **kw):
        import torch
        self.rg, self.E, self.G, self.P, self.torch = rg, rg.engine, G, P, torch
        self.eng = eng = rg.Engine(G, P, flags=self.E.CFGF.IX64 if ix64 else None, **kw)
        assert eng.device_info()["last_tick_offset_bits"] in (0, 64 if ix64 else 32)
        self.stride = eng.stride
        rng = self.rng = random.Random(seed * 1000 + G * 10 + P)
        st = R.base_state(G, P, self.stride)
        for g in range(G):
            if terms:
                st["cur_term"][g] = rng.choice((2, 3, 7, 1 << 40))
            if transferees and P > 1 and rng.random() < 0.4:
                st["cfg"][g] = int(st["cfg"][g]) | (rng.randrange(P) + 1) << 20
        for k in LOAD_COLS:
            eng.load_column(self.E.COL.NAMES.index(k), st[k])
        if reads:
            eng.read_index_enable(DEPTH)
        eng.lead_clock_enable(CLOCK.election_tick, CLOCK.heartbeat_tick, CLOCK.flags)
        self.clock = [T.random_clock(rng, int(st["cfg"][g]), int(st["cur_term"][g])) for g in range(G)]
        cells = np.zeros(G, dtype=self.E.LEAD_CLOCK_CELL_DTYPE)
        for g, c in enumerate(self.clock):
            cells[g]["group"], cells[g]["term"], cells[g]["election_elapsed"], cells[g]["heartbeat_elapsed"], cells[g]["led"] = g, c["tag"], c["el"], c["hb"], c["led"]
        eng.lead_clock_write(cells)
        self.reads = None
        if reads:
            self.reads = [RO.Group(int(st["cfg"][g]), commit=2, term_lo=1, term=int(st["cur_term"][g]), depth=DEPTH) for g in range(G)]
            reqs = [(g, 100 + g) for g in range(G)]
            want = [ro.request(ctx)[0] for ro, (_, ctx) in zip(self.reads, reqs)]
            assert [int(x) for x in eng.read_index(reqs)] == want
        self.state = self.read_state()

    def read_state(self):
        st = {"n_groups": self.G, "n_slots": self.P, "stride": self.stride}
        for k in READ_COLS:
            st[k] = self.eng.read_column(self.E.COL.NAMES.index(k))
        return st

    def rows(self, calm):
        """Random rows for every group -> (u8 [G][8], u64 [P][stride])"""
        flags, terms = np.zeros((self.G, 8), np.uint8), np.full((self.P, self.stride), 0xDEAD, np.uint64)
        for g in range(self.G):
            f, t = T.random_row(self.rng, self.P, self.clock[g]["cur_term"], calm)
            flags[g] = f
            terms[:, g] = t[:self.P]
        return flags, terms

    def model(self, flags, terms):
        """The model over copies of the clock dicts (and of the read groups) -> (rows, events, new_terms, counts, clocks, reads)"""
        import copy
        clocks, reads = [L.copy_group(c) for c in self.clock], copy.deepcopy(self.reads)
        rows, events, new_terms, counts = [], [], [], [0, 0, 0]
        for g in range(self.G):
            t = [int(x) for x in terms[:, g]] + [0] * (8 - self.P)
            row, ev, nt, stale, not_led = T.gate(clocks[g], [int(b) for b in flags[g]], t, self.P, reads[g] if reads else None)
            rows.append(row)
            events.append(ev)
            new_terms.append(nt)
            counts[0] += bool(ev & T.EV_DEPOSED)
            counts[1] += stale
            counts[2] += not_led
        return rows, events, new_terms, tuple(counts), clocks, reads

    def call(self, flags, terms, alias, down_cap, sync=True):
        """One gate call with sentinels around every output -> dict of host copies"""
        torch, G = self.torch, self.G
        d_flags = torch.full((G * 8 + 64,), EV_SENT, dtype=torch.uint8, device="cuda")
        d_flags[:G * 8] = dev(flags.reshape(-1))
        d_out = d_flags if alias else torch.full((G * 8 + 64,), EV_SENT, dtype=torch.uint8, device="cuda")
        d_terms = dev(terms)
        events = torch.full((self.stride + 8,), EV_SENT, dtype=torch.uint8, device="cuda")
        new_term = torch.full((self.stride + 8,), U64_SENT - (1 << 64), dtype=torch.int64, device="cuda")
        down = torch.full((down_cap + 4,), U64_SENT - (1 << 64), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        counts = self.eng.lead_gate_device(d_flags, d_terms, events, new_term, None if alias else d_out, down if down_cap else None, down_cap, sync=sync)
        if not sync:  # the counts are the three device words
            self.eng.sync()
            counts = tuple(device_u64(self.eng.lead_gate_counts(), 3))
        self.eng.sync()
        return {"in": d_flags.cpu().numpy(), "out": d_out.cpu().numpy(), "events": events.cpu().numpy(), "new_term": new_term.cpu().numpy().view(np.uint64),
                "down": down.cpu().numpy().view(np.uint64), "counts": counts, "d_out": d_out}

    def check(self, got, flags, want, alias, down_cap):
        rows, events, new_terms, counts, clocks, reads = want
        G = self.G
        assert [[int(b) for b in r] for r in got["out"][:G * 8].reshape(G, 8)] == rows
        assert (got["out"][G * 8:] == EV_SENT).all()
        if not alias:
            assert (got["in"][:G * 8].reshape(G, 8) == flags).all()  # the input rows are read only
        assert [int(x) for x in got["events"][:G]] == events and (got["events"][G:] == EV_SENT).all()
        assert [int(x) for x in got["new_term"][:G]] == [U64_SENT if t is None else t for t in new_terms] and (got["new_term"][G:] == U64_SENT).all()
        assert got["counts"] == counts, (got["counts"], counts)
        deposed = [g for g, e in enumerate(events) if e & T.EV_DEPOSED]
        listed = min(down_cap, len(deposed))
        lst = [int(x) for x in got["down"][:listed]]
        assert len(set(lst)) == listed and set(lst) <= set(deposed) and (got["down"][listed:] == U64_SENT).all()
        if down_cap >= len(deposed):
            assert sorted(lst) == deposed
        # the clock cells, the cfg words, every other column
        cells = self.eng.lead_clock_read(np.arange(G, dtype=np.uint64))
        for g, (r, c) in enumerate(zip(cells, clocks)):
            assert (int(r["term"]), int(r["election_elapsed"]), int(r["heartbeat_elapsed"]), int(r["led"])) == (c["tag"], c["el"], c["hb"], int(c["led"])), (g, r, c)
            if not events[g] & T.EV_DEPOSED:
                assert c == self.clock[g]
        after = self.read_state()
        assert [int(x) for x in after["cfg"]] == [c["cfg"] for c in clocks]
        after["cfg"] = self.state["cfg"]
        assert not R.diff(self.state, after, R.ALL_COLS + ("out",))
        if reads:
            assert [int(x) for x in self.eng.read_pending_counts()] == [len(ro.queue()) for ro in reads]
            assert [int(x) for x in self.eng.read_last_pending()] == [ro.last_pending() for ro in reads]
        return deposed

    def close(self):
        self.eng.sync()
        self.eng.close()


@pytest.mark.parametrize("ix64", [False, True])
@pytest.mark.parametrize("P", [1, 3, 8])
@pytest.mark.parametrize("G", [1, 63, 64, 65, 257])
def test_gate_equals_the_model(rg, G, P, ix64):
    """Random rows over led, stopped and stale-tagged groups: not aliased with room for every deposed group, aliased with room for
    one, aliased and asynchronous with no list. The ReadIndex layer is on for the 32-bit engines and off for the 64-bit ones."""
    rig = GateRig(rg, G, P, ix64, reads=not ix64)
    rig.eng.checkpoint()
    flags, terms = rig.rows(calm=0.7 if G > 1 else 0.0)
    want = rig.model(flags, terms)
    seen = set()
    for alias, down_cap, sync in ((False, G + 1, True), (True, 1, True), (True, 0, False)):
        got = rig.call(flags, terms, alias, down_cap, sync)
        seen |= set(want[1])
        rig.check(got, flags, want, alias, down_cap)
        rig.eng.restore()
    if G >= 63:
        assert {0, T.EV_NOT_LED, T.EV_DEPOSED} <= {e & ~T.EV_TRANSFER_ABORTED for e in seen} and (P == 1 or T.EV_STALE in seen)
    rig.close()


def test_named_edges(rg):
    """One hand-written row per rule of the header, in the lanes around a wave edge of a 65-group engine."""
    rig = GateRig(rg, 65, 3, seed=2)
    V, H, S, F = T.MF_VALID, T.MF_HEARTBEAT, T.MF_SENT, T.MF_INS_FULL
    flags, terms = np.zeros((65, 8), np.uint8), np.zeros((3, rig.stride), np.uint64)
    cells = np.zeros(65, dtype=rig.E.LEAD_CLOCK_CELL_DTYPE)
    for g, c in enumerate(rig.clock):  # every group led, but 62 (stopped) and 64 (stopped under an older tag: led)
        c["led"], c["tag"] = g not in (62, 64), c["cur_term"] - (1 if g == 64 else 0)
        cells[g]["group"], cells[g]["term"], cells[g]["election_elapsed"], cells[g]["heartbeat_elapsed"], cells[g]["led"] = g, c["tag"], c["el"], c["hb"], c["led"]
    rig.eng.lead_clock_write(cells)
    cur = [c["cur_term"] for c in rig.clock]
    flags[60, :3], terms[:, 60] = (V | S | F | T.MF_REJECT, H | F, V), (cur[60] - 1, cur[60] - 1, cur[60])  # stale slots keep SENT | INS_FULL
    flags[61, :3], terms[:, 61] = (V, V | S, H), (cur[61], cur[61] + 1, cur[61])  # a deposing slot beside valid ones zeroes the row
    flags[62, :3], terms[:, 62] = (V, H, S), (cur[62], cur[62] + 5, 0)  # stopped: NOT_LED whatever the terms say, two records
    flags[63, :3], terms[:, 63] = (V, H, V), (cur[63] + 2, cur[63] + 9, cur[63] + 4)  # the maximum of the higher terms
    flags[64, :3], terms[:, 64] = (V, V, V | T.MF_APPEND), (cur[64], cur[64] - 1, 0)  # a tag that differs from the term: led
    flags[0, :3], terms[:, 0] = (V | T.MF_APPEND, T.MF_REJECT, S), (0, 77, 99)  # local messages; what is no record is never judged
    want = rig.model(flags, terms)
    got = rig.call(flags, terms, False, 8)
    rig.check(got, flags, want, False, 8)
    out, ev, nt = got["out"][:65 * 8].reshape(65, 8), got["events"], got["new_term"]
    assert list(out[60][:3]) == [S | F, F, V] and ev[60] == T.EV_STALE
    assert not out[61].any() and ev[61] & T.EV_DEPOSED and nt[61] == cur[61] + 1
    assert not out[62].any() and ev[62] == T.EV_NOT_LED and nt[62] == U64_SENT
    assert not out[63].any() and nt[63] == cur[63] + 9
    assert list(out[64][:3]) == [V, 0, V | T.MF_APPEND] and ev[64] == T.EV_STALE
    assert list(out[0][:3]) == [V | T.MF_APPEND, T.MF_REJECT, S] and ev[0] == 0
    assert got["counts"] == (2, 3, 2)
    for g in (61, 63):  # the transferee is cleared where there was one
        had = rig.state["cfg"][g] >> 20 & 0xF
        assert bool(ev[g] & T.EV_TRANSFER_ABORTED) == bool(had)
    rig.close()


def test_entry_conditions(rg):
    """RG_ERR_STATE before rgx_lead_clock_enable and on an engine with a host mirror; bad arguments are host errors; an engine
    with device Inflights is allowed."""
    import torch
    E = rg.engine
    eng = rg.Engine(8, 3)
    flags, terms = torch.zeros(64, dtype=torch.uint8, device="cuda"), torch.zeros(3 * eng.stride, dtype=torch.int64, device="cuda")
    events, new_term = torch.zeros(eng.stride, dtype=torch.uint8, device="cuda"), torch.zeros(eng.stride, dtype=torch.int64, device="cuda")
    with pytest.raises(rg.EngineError) as ei:
        eng.lead_gate_device(flags, terms, events, new_term)
    assert ei.value.code == E.ERR["STATE"] and "rgx_lead_clock_enable first" in str(ei.value)
    eng.lead_clock_enable(10, 3, L.START_LED)
    assert eng.lead_gate_device(flags, terms, events, new_term) == (0, 0, 0)
    for bad in (lambda: eng.lead_gate_device(None, terms, events, new_term), lambda: eng.lead_gate_device(flags, None, events, new_term),
                lambda: eng.lead_gate_device(flags, terms, None, new_term), lambda: eng.lead_gate_device(flags, terms, events, None),
                lambda: eng.lead_gate_device(flags, terms, events, new_term, down=None, down_cap=4),
                lambda: eng.lead_gate_device(flags.data_ptr() + 1, terms, events, new_term)):
        with pytest.raises(rg.EngineError) as ei:
            bad()
        assert ei.value.code == E.ERR["INVALID_ARG"]
    eng.set_peers(0, [1, 2, 3], 2)
    with pytest.raises(rg.EngineError) as ei:
        eng.lead_gate_device(flags, terms, events, new_term)
    assert ei.value.code == E.ERR["STATE"] and "host mirror" in str(ei.value)
    eng.close()
    rig = GateRig(rg, 65, 3, seed=3, max_inflight=4)
    f, t = rig.rows(calm=0.5)
    rig.check(rig.call(f, t, True, 65), f, rig.model(f, t), True, 65)
    rig.close()


def test_tick_parity_on_the_filtered_rows(rg):
    """The gate, then rg_tick_device on the rows it left: bit-exact against the oracle stepping only the records the model lets
    through -- acknowledgements of the current term advance their groups, stale ones and those of deposed or stopped groups do
    nothing."""
    G, P = 257, 3
    rig = GateRig(rg, G, P, seed=4, terms=False, transferees=False)
    acks = rg.MsgBuffers(G, P, rig.stride)
    terms = np.zeros((P, rig.stride), np.uint64)
    rng = random.Random(5)
    for g in range(G):
        for s in (1, 2):
            acks.m_flags[g, s], acks.m_index[s, g] = T.MF_VALID | (T.MF_SENT if rng.random() < 0.3 else 0), 3
            terms[s, g] = 2 if rng.random() < 0.7 else rng.choice((1, 2, 3, 5))
    flags = acks.m_flags.copy()
    want = rig.model(flags, terms)
    rows, events = want[0], want[1]
    assert {0, T.EV_STALE, T.EV_NOT_LED, T.EV_DEPOSED} <= {e & ~T.EV_TRANSFER_ABORTED for e in events}
    got = rig.call(flags, terms, False, G)
    rig.check(got, flags, want, False, G)
    cols = [dev(getattr(acks, k)) for k in ("m_index", "m_commit", "m_hint", "m_rs")]
    rig.eng.tick_device(*[c.data_ptr() for c in cols], got["d_out"].data_ptr())
    rig.eng.sync()
    state = R.copy_state(rig.state)
    state["cfg"] = np.array([c["cfg"] for c in want[4]], dtype=state["cfg"].dtype)
    msgs = acks.as_dict()
    msgs["m_flags"] = np.array(rows, dtype=np.uint8)
    after, gout = R.oracle_tick(state, msgs)
    engine_after = rig.read_state()
    assert not R.diff(after, engine_after), R.diff(after, engine_after)
    assert (engine_after["out"][:G] == gout).all()
    moved = [g for g in range(G) if int(engine_after["commit"][g]) != int(rig.state["commit"][g])]
    assert moved and all(events[g] in (0, T.EV_STALE) for g in moved)
    rig.close()
