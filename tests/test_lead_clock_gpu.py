"""GPU: the leader's clock (rgx_lead_clock_enable / _write / _read / rgx_lead_clock / rgx_lead_clock_counts) against
tests/lead_clock_model.py: the clock cells, RG_COL_PFLAGS, RG_COL_CFG, the event column, the heartbeat commits, the lists and the
counts of every group, bit for bit, with sentinels in every output buffer. No test provokes a device fault: every bad argument is
refused on the host."""
import random

import numpy as np
import pytest

import handoff_rig as R
import lead_clock_model as L
from test_follow_gate_gpu import device_u64

pytestmark = pytest.mark.gpu

EV_SENT, U64_SENT = 0xEE, 0xA5A5A5A5A5A5A5A5


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


class Rig:
    """A leader engine of L.SHAPES[P] x P whose groups are the model's: the edge shapes first, random groups behind them."""

    def __init__(self, rg, P, c, seed, ix64=False, start_led=True, write=True, small=False, max_inflight=0, before_enable=None):
        self.rg, self.E, self.P, self.c, self.G = rg, rg.engine, P, c, L.SHAPES[P]
        self.eng = rg.Engine(self.G, P, flags=self.E.CFGF.IX64 if ix64 else None, max_inflight=max_inflight)
        self.stride = self.eng.stride
        rng = random.Random(seed)
        self.groups = [L.random_group(rng, P, c) for _ in range(self.G)]
        for k, (name, (cfg, pflags)) in enumerate(L.edge_groups(P).items()):  # each edge shape at both timeouts at once, and at the election timeout alone
            for j, hb in enumerate((c.heartbeat_tick - 1, 0)):
                g = L.new_group(P, cfg, cur_term=3, pflags=pflags, match=[7 + 3 * s for s in range(P)], commit=12)
                g["el"], g["hb"] = c.election_tick - 1, hb
                self.groups[(2 * k + j) * 5 % self.G] = g
        st = R.base_state(self.G, P, self.stride)
        for g in self.groups if small else ():  # (a log a tick can run on: base_state's three entries)
            g["commit"], g["match"], g["cur_term"] = min(g["commit"], 2), [min(m, 3) for m in g["match"]], 2
        for i, g in enumerate(self.groups):
            st["cfg"][i], st["cur_term"][i], st["commit"][i] = g["cfg"], g["cur_term"], g["commit"]
            st["pflags"][i, :] = g["pflags"]
            st["match"][:P, i] = g["match"]
        for k in ("cfg", "cur_term", "commit", "pflags", "match"):
            self.eng.load_column(self.E.COL.NAMES.index(k), st[k])
        self.adopt()
        if before_enable:  # (what a test does between the load and the enable call)
            before_enable(self)
        self.eng.lead_clock_enable(c.election_tick, c.heartbeat_tick, c.flags | (L.START_LED if start_led else 0))
        if write:
            self.write(range(self.G))
        else:  # what the enable call left: the tag is the column's value, both counters 0
            for g in self.groups:
                g["tag"], g["hb"], g["el"], g["led"] = g["cur_term"], 0, 0, start_led

    def adopt(self):
        """The columns the clock reads, as the engine holds them (it keeps its own bits of a loaded flag row exact; a tick writes them)."""
        col = {k: self.eng.read_column(self.E.COL.NAMES.index(k)) for k in ("cfg", "cur_term", "commit", "pflags", "match")}
        for i, g in enumerate(self.groups):
            g["cfg"], g["cur_term"], g["commit"] = int(col["cfg"][i]), int(col["cur_term"][i]), int(col["commit"][i])
            g["pflags"], g["match"] = [int(b) for b in col["pflags"][i]], [int(x) for x in col["match"][:self.P, i]]

    def write(self, which):
        which = list(which)
        a = np.zeros(len(which), dtype=self.E.LEAD_CLOCK_CELL_DTYPE)
        for k, i in enumerate(which):
            g = self.groups[i]
            a[k]["group"], a[k]["term"], a[k]["election_elapsed"], a[k]["heartbeat_elapsed"], a[k]["led"] = i, g["tag"], g["el"], g["hb"], int(g["led"])
        self.eng.lead_clock_write(a)

    def close(self):
        self.eng.sync()
        self.eng.close()

    def check_cells(self):
        got = self.eng.lead_clock_read(np.arange(self.G, dtype=np.uint64))
        for i, (r, g) in enumerate(zip(got, self.groups)):
            assert (int(r["group"]), int(r["term"]), int(r["election_elapsed"]), int(r["heartbeat_elapsed"]), int(r["led"])) == (i, g["tag"], g["el"], g["hb"], int(g["led"])), (i, r, g)
            assert not r["reserved"].any()
        cfg, pf = self.eng.read_column(self.E.COL.CFG), self.eng.read_column(self.E.COL.PFLAGS)
        assert [int(x) for x in cfg] == [g["cfg"] for g in self.groups]
        assert [[int(b) for b in row] for row in pf] == [g["pflags"] for g in self.groups]

    def clock(self, beat_cap=None, down_cap=None, hb=True, sync=True):
        """One rgx_lead_clock against the model, every output checked. Caps None = room for all. -> the model's events"""
        import torch
        want, want_hb = [], {}
        for i, g in enumerate(self.groups):
            ev = L.tick(self.c, g)
            want.append(ev)
            if ev & L.EV_BEAT:
                want_hb[i] = L.heartbeat_commits(g, self.P)
        beats, downs = [i for i, e in enumerate(want) if e & L.EV_BEAT], [i for i, e in enumerate(want) if e & L.EV_STEPPED_DOWN]
        counts = (len(beats), sum(1 for e in want if e & L.EV_CHECK_QUORUM), len(downs), sum(1 for e in want if e & L.EV_TRANSFER_ABORTED))
        beat_cap = self.G if beat_cap is None else beat_cap(len(beats)) if callable(beat_cap) else beat_cap
        down_cap = self.G if down_cap is None else down_cap(len(downs)) if callable(down_cap) else down_cap
        events = torch.full((self.stride,), EV_SENT, dtype=torch.uint8, device="cuda")
        beat = torch.full((beat_cap + 3,), U64_SENT - (1 << 64), dtype=torch.int64, device="cuda")
        down = torch.full((down_cap + 3,), U64_SENT - (1 << 64), dtype=torch.int64, device="cuda")
        hbc = torch.full((self.P, self.stride), U64_SENT - (1 << 64), dtype=torch.int64, device="cuda") if hb else None
        got = self.eng.lead_clock(events, beat if beat_cap else None, beat_cap, down if down_cap else None, down_cap, hbc, sync=sync)
        if not sync:
            assert got is None
            self.eng.sync()
        words = tuple(device_u64(self.eng.lead_clock_counts(), 4))  # the four device words, either way
        got = words if got is None else got
        assert words == counts, (words, counts)
        assert got == counts, (got, counts)
        ev = events.cpu().numpy()
        assert [int(x) for x in ev[:self.G]] == want and (ev[self.G:] == EV_SENT).all()
        for name, buf, cap, full in (("beat", beat, beat_cap, beats), ("down", down, down_cap, downs)):
            lst = buf.cpu().numpy().view(np.uint64)
            k = min(cap, len(full))
            assert len(set(int(x) for x in lst[:k])) == k and set(int(x) for x in lst[:k]) <= set(full), (name, lst[:k], full)
            assert (lst[k:] == U64_SENT).all(), name
        if hb:
            h = hbc.cpu().numpy().view(np.uint64)
            for i in range(self.stride):
                assert [int(x) for x in h[:, i]] == want_hb.get(i, [U64_SENT] * self.P), (i, want[i] if i < self.G else None)
        self.check_cells()
        return want


CASES = [(1, L.Config(2, 1, L.CHECK_QUORUM), False), (3, L.Config(6, 3, L.CHECK_QUORUM), False), (5, L.Config(6, 3, 0), False),
         (8, L.Config(L.TICK_MAX, L.TICK_MAX - 1, L.CHECK_QUORUM), True), (3, L.Config(2, 1, 0), True)]


@pytest.mark.parametrize("P,c,ix64", CASES)
def test_clock_matches_the_model_cell_for_cell(rg, P, c, ix64):
    """Edge shapes and random groups (cells written one increment before either timeout, 16382 included; stopped groups; tags the
    clock has not seen) through several calls: coinciding timeouts with and without a step-down, check quorum off (no flag byte
    moves, the transferee is still aborted), every group and config shape of the model's edge list."""
    rig = Rig(rg, P, c, seed=40 + P, ix64=ix64)
    rig.check_cells()
    seen = set()
    for _ in range(4 if c.election_tick < 100 else 2):
        seen |= set(rig.clock())
    bits = {b for b in (1, 2, 4, 8, 16) if any(e & b for e in seen)}
    assert bits == ({1, 2, 4, 8, 16} if c.check_quorum else {1, 8, 16}), bits
    rig.close()


def test_lists_at_their_caps_and_the_asynchronous_form(rg):
    """Caps of 0, 1, exactly the number due and one less: the lists are subsets of the event column, the counts are the totals, a
    group that did not fit was still ticked; the asynchronous form leaves the same counts in the device words."""
    c = L.Config(2, 1, L.CHECK_QUORUM)
    rig = Rig(rg, 3, c, seed=50)
    rig.clock(beat_cap=0, down_cap=0)
    rig.clock(beat_cap=1, down_cap=1, hb=False)
    for i, g in enumerate(rig.groups):  # lead every group again, one increment before the election timeout, some of them quorate
        g["led"], g["el"], g["hb"] = True, 1, 0
        if i % 3:
            g["pflags"] = [b | L.PF_RECENT_ACTIVE for b in g["pflags"]]
    rig.write(range(rig.G))
    pf = np.array([g["pflags"] for g in rig.groups], dtype=np.uint8)
    rig.eng.load_column(rig.E.COL.PFLAGS, pf)
    rig.adopt()
    ev = rig.clock(beat_cap=lambda n: n, down_cap=lambda n: max(n - 1, 0))
    assert sum(1 for e in ev if e & L.EV_STEPPED_DOWN) > 1 and sum(1 for e in ev if e & L.EV_BEAT) > 1
    rig.clock(beat_cap=lambda n: max(n - 1, 0), down_cap=lambda n: n, sync=False)
    rig.close()


def test_initial_state_and_lazy_arming(rg):
    """Without START_LED every group starts stopped and costs nothing but its event byte; a new RG_COL_CUR_TERM -- written by an
    RG_MF_BECOME_LEADER tick -- arms the group: NEW_TERM, counters 1 and 1 (0 where a timeout of 1 fires), a stopped cell led."""
    c = L.Config(3, 1, L.CHECK_QUORUM)
    rig = Rig(rg, 3, c, seed=60, start_led=False, write=False, small=True)
    assert set(rig.clock()) == {0}
    # groups 5..24 win an election in a tick: m_flags = RG_MF_BECOME_LEADER on the own slot, m_hint = the new term
    msgs = rig.rg.MsgBuffers(rig.G, 3, rig.stride)
    armed = [i for i in range(5, 25) if H_present_self(rig.groups[i])]
    for i in armed:
        s = rig.groups[i]["cfg"] >> 16 & 7
        msgs.m_flags[i, s] = 0x02
        msgs.m_hint[s, i] = 100 + i
    rig.eng.tick(msgs)
    rig.adopt()  # (what the tick did to the columns the clock reads is the tick's business: take it over)
    assert len(armed) > 10 and all(rig.groups[i]["cur_term"] == 100 + i for i in armed)
    ev = rig.clock()
    assert all(ev[i] == L.EV_NEW_TERM | L.EV_BEAT and rig.groups[i]["led"] and (rig.groups[i]["hb"], rig.groups[i]["el"]) == (0, 1) for i in armed)
    assert all(e == 0 for i, e in enumerate(ev) if i not in armed)
    rig.clock()
    rig.clock()  # the election timeout of the armed groups: nobody answered
    rig.close()


def H_present_self(g):
    return bool(g["cfg"] >> 24 >> (g["cfg"] >> 16 & 7) & 1)


def test_state_travels_with_checkpoint_restore_and_permutation(rg):
    """rg_checkpoint / rg_restore carry the cells, rg_permute_groups moves them with their groups; one more call behind each."""
    c = L.Config(6, 3, L.CHECK_QUORUM)
    rig = Rig(rg, 5, c, seed=70)
    rig.clock()
    before = rig.eng.device_info()["engine_bytes"]
    rig.eng.checkpoint()
    saved = [L.copy_group(g) for g in rig.groups]
    rig.clock()
    rig.clock()
    rig.eng.restore()
    rig.groups = saved
    rig.check_cells()
    rig.clock()
    perm = np.random.default_rng(7).permutation(rig.G).astype(np.uint64)
    rig.eng.permute_groups(perm)
    rig.groups = [rig.groups[int(o)] for o in perm]
    rig.check_cells()
    rig.clock()
    assert rig.eng.device_info()["engine_bytes"] == before
    rig.close()


def test_refusals_are_errors_not_faults(rg):
    """Every bad argument is refused on the host with nothing written; a second enable and calls before the enable are RG_ERR_STATE."""
    E = rg.engine
    eng = rg.Engine(300, 3)
    cells = np.zeros(1, dtype=E.LEAD_CLOCK_CELL_DTYPE)
    for call in (lambda: eng.lead_clock_write(cells), lambda: eng.lead_clock_read([0]), lambda: eng.lead_clock(1)):
        with pytest.raises(rg.EngineError) as ei:
            call()
        assert "rgx_lead_clock_enable first" in str(ei.value)
    assert not eng.lead_clock_counts()
    for bad in ((1, 1, 0), (2, 2, 0), (2, 0, 0), (16384, 1, 0), (10, 3, 2)):
        with pytest.raises(rg.EngineError):
            eng.lead_clock_enable(*bad)
    bytes_before = eng.device_info()["engine_bytes"]
    eng.lead_clock_enable(10, 3, L.CHECK_QUORUM | L.START_LED)
    assert eng.device_info()["engine_bytes"] == bytes_before + eng.stride * 12 + 32 and eng.lead_clock_counts()
    with pytest.raises(rg.EngineError):
        eng.lead_clock_enable(10, 3, 0)
    good = np.zeros(2, dtype=E.LEAD_CLOCK_CELL_DTYPE)
    good["group"], good["term"], good["election_elapsed"], good["heartbeat_elapsed"], good["led"] = (7, 8), 5, 9, 2, 1
    eng.lead_clock_write(good)
    for field, value in (("group", 300), ("election_elapsed", 10), ("heartbeat_elapsed", 3), ("led", 2), ("group", 8)):
        bad = good.copy()
        bad[field][0] = value
        bad["term"] = 99
        with pytest.raises(rg.EngineError):
            eng.lead_clock_write(bad)
    bad = good.copy()
    bad["reserved"][1][6] = 1
    bad["term"] = 99
    with pytest.raises(rg.EngineError):
        eng.lead_clock_write(bad)
    with pytest.raises(rg.EngineError):
        eng.lead_clock_read([0, 300])
    got = eng.lead_clock_read([7, 8, 9])
    t9 = int(eng.read_column(E.COL.CUR_TERM)[9])
    assert [(int(r["term"]), int(r["election_elapsed"]), int(r["heartbeat_elapsed"]), int(r["led"])) for r in got] == [(5, 9, 2, 1), (5, 9, 2, 1), (t9, 0, 0, 1)]
    eng.close()
