"""GPU: corners of the leader's clock and of the way back into the arena that include/raftgroups_lead.h states and nothing ran: a
second rgx_follow_step_down_device over the same event column, an engine with a host mirror (rg_set_peers), an engine with
device Inflights (max_inflight > 0), and a clock layer enabled AFTER the checkpoint a later rg_restore goes back to. Against
tests/lead_clock_model.py composed with gate_model and handoff_model, cell for cell. No test provokes a device fault: every bad
argument used is one the host refuses."""
import numpy as np
import pytest

import handoff_model as H
import handoff_rig as R
import lead_clock_model as L
from test_handoff_gpu import U64_SENT, dev
from test_lead_clock_gpu import Rig as ClockRig
from life_cycle_rig import CLOCK, ClockModel, expect_arena, promoted_rig, tick_until_down

pytestmark = pytest.mark.gpu


def lead_column(rig, pairs):
    lead = np.full(rig.stride, L.NO_LEAD, np.uint64)
    for g, Lg in pairs:
        lead[g] = Lg
    return dev(lead)


def test_a_second_step_down_over_the_same_events_changes_nothing(rg):
    """rgx_follow_step_down_device twice with the event column of ONE clock call: the groups the first call took back answer
    NOT_WON to the second (their soft cells no longer say "leader_id == self_id"), and no cell of the arena's three layers, of the
    leader columns or of the clock moves. The sparse form answers the same."""
    rig, cases, done = promoted_rig(rg)
    events, counts = tick_until_down(rig)
    assert counts[2] == len(done) > 3
    pairs = [(c.g, c.L) for c in done]
    d_lead = lead_column(rig, pairs)
    out = rig.out_columns()
    rig.eng.follow_step_down_device(events, d_lead, out)
    rig.eng.sync()
    status = out["status"].cpu().numpy()
    assert all(int(status[g]) == H.DONE for g, _ in pairs)
    everyone = np.arange(rig.G, dtype=np.uint64)
    lead_state, arena, cells = rig.read_lead(), rig.arena(), rig.eng.lead_clock_read(everyone)
    again = rig.out_columns()
    rig.eng.follow_step_down_device(events, d_lead, again)
    rig.eng.sync()
    rig.dense_answers(again, done, [(H.NOT_WON, 0, 0, 0, 0)] * len(done))
    recs = np.zeros(len(pairs), dtype=rig.E.HANDOFF_REC_DTYPE)
    recs["follow_group"], recs["lead_group"], recs["persisted"] = [p[0] for p in pairs], [p[1] for p in pairs], U64_SENT
    got = rig.eng.follow_step_down(recs)
    assert [tuple(int(r[k]) for k in ("status", "term", "last_index", "commit", "out")) for r in got] == [(H.NOT_WON, 0, 0, 0, 0)] * len(pairs)
    assert rig.arena() == arena and not R.diff(lead_state, rig.read_lead(), R.ALL_COLS + ("out",))
    assert rig.eng.lead_clock_read(everyone).tobytes() == cells.tobytes()
    rig.close()


def test_a_mirrored_engine_takes_the_sparse_road(rg):
    """An engine with a host mirror (rg_set_peers): the dense step-down is RG_ERR_STATE, as the header says. rg_step + rg_flush
    make the peers of every other promoted group recent_active; rgx_lead_clock, synchronous and asynchronous, then matches the
    model -- those groups pass their check, the others step down --, the sparse rgx_follow_step_down takes the others back as the
    model says, and an rg_local_append + rg_local_persisted behind it still lands in the group's own slot (the mirror re-reads its
    copy of the cfg words the clock may have written)."""
    import torch
    rig, cases, done = promoted_rig(rg)
    eng, P = rig.eng, rig.P
    st = rig.read_lead()
    stay, leave = done[::2], done[1::2]
    ids = {c.L: [8 * c.L + s + 1 for s in range(P)] for c in done}
    for c in done:
        eng.set_peers(c.L, ids[c.L], int(st["cur_term"][c.L]))
    events = torch.zeros(eng.stride, dtype=torch.uint8, device="cuda")
    d_lead = lead_column(rig, [(c.g, c.L) for c in done])
    torch.cuda.synchronize()
    with pytest.raises(rg.EngineError) as ei:
        eng.follow_step_down_device(events, d_lead, rig.out_columns())
    assert ei.value.code == -8 and "host mirror" in str(ei.value)
    model = ClockModel(rig, CLOCK)
    for g in model.groups:  # (promoted_rig enabled the clock with START_LED)
        g["led"] = True
    want = model.tick()
    assert eng.lead_clock(events)[2] == 0
    model.check(events, want)
    for c in stay:  # every peer acknowledges the leader's last index at the leader's term
        self_slot = H.cfg_fields(int(st["cfg"][c.L]))[2]
        for s in range(P):
            if s != self_slot:
                eng.step(c.L, ids[c.L][s], int(st["cur_term"][c.L]), int(st["term_hi"][c.L]))
    eng.flush()
    model.adopt()
    for c in stay:
        self_slot = H.cfg_fields(int(st["cfg"][c.L]))[2]
        assert all(model.groups[c.L]["pflags"][s] & L.PF_RECENT_ACTIVE for s in range(P) if s != self_slot), c.name
    want = model.tick()
    assert eng.lead_clock(events, sync=False) is None
    eng.sync()
    model.check(events, want)
    assert all(want[c.L] & L.EV_CHECK_QUORUM and not want[c.L] & L.EV_STEPPED_DOWN for c in stay)
    assert all(want[c.L] == L.EV_CHECK_QUORUM | L.EV_STEPPED_DOWN for c in leave)
    # ---- the sparse road back ----
    lead_state, before = rig.read_lead(), rig.arena()
    pairs = [(c.g, c.L) for c in leave]
    arena_want, answers = expect_arena(before, lead_state, pairs)
    assert all(a[0] == H.DONE for a in answers)
    recs = np.zeros(len(pairs), dtype=rig.E.HANDOFF_REC_DTYPE)
    recs["follow_group"], recs["lead_group"], recs["persisted"] = [p[0] for p in pairs], [p[1] for p in pairs], U64_SENT
    got = eng.follow_step_down(recs)
    assert [tuple(int(r[k]) for k in ("status", "term", "last_index", "commit")) for r in got] == answers and not got["out"].any()
    assert rig.arena() == arena_want and not R.diff(lead_state, rig.read_lead(), R.ALL_COLS + ("out",))
    assert not eng.lead_clock_read([c.L for c in leave])["led"].any() and eng.lead_clock_read([c.L for c in stay])["led"].all()
    # ---- the mirror still knows which slot is the group's own ----
    for c in stay:
        eng.local_append(c.L, int(lead_state["term_hi"][c.L]) + 1)
    eng.flush()
    for c in stay:
        eng.local_persisted(c.L, int(lead_state["term_hi"][c.L]) + 1)
    eng.flush()
    after = rig.read_lead()
    for c in stay:
        self_slot, hi = H.cfg_fields(int(lead_state["cfg"][c.L]))[2], int(lead_state["term_hi"][c.L])
        assert int(after["term_hi"][c.L]) == hi + 1 and int(after["match"][self_slot, c.L]) == hi + 1, c.name
        assert all(int(after["match"][s, c.L]) == int(lead_state["match"][s, c.L]) for s in range(P) if s != self_slot), c.name
    rig.close()


def test_an_engine_with_device_inflights_matches_the_model(rg):
    """max_inflight > 0 (the header: "Engines with max_inflight > 0 are allowed"): the shape of test_lead_clock_gpu's three-slot
    case on such an engine, cell for cell through two election timeouts."""
    c = L.Config(6, 3, L.CHECK_QUORUM)
    rig = ClockRig(rg, 3, c, seed=43, max_inflight=4)
    assert rig.eng.device_info()["engine_bytes"] > 0
    rig.check_cells()
    seen = set()
    for _ in range(4):
        seen |= set(rig.clock())
    assert {b for b in (1, 2, 4, 8, 16) if any(e & b for e in seen)} == {1, 2, 4, 8, 16}
    rig.close()


def test_a_clock_enabled_after_the_checkpoint_survives_the_restore(rg):
    """rg_checkpoint, THEN half the groups move to their next term and the clock layer is enabled: the image does not hold the
    layer, so rg_restore leaves its cells alone while RG_COL_CUR_TERM goes back. By the tag rule the next call takes such a group
    for a new leadership: NEW_TERM, both counters restarted, whatever the cell held; the other groups tick on."""
    c = L.Config(6, 3, L.CHECK_QUORUM)
    moved = []

    def checkpoint_then_move(rig):
        rig.eng.checkpoint()
        term = rig.eng.read_column(rig.E.COL.CUR_TERM)
        moved.extend(range(0, rig.G, 2))
        term[moved] += np.uint64(1)
        rig.eng.load_column(rig.E.COL.CUR_TERM, term)
        rig.adopt()
    rig = ClockRig(rg, 3, c, seed=44, write=False, before_enable=checkpoint_then_move)
    rig.check_cells()
    rig.clock()
    rig.clock()
    cells = rig.eng.lead_clock_read(np.arange(rig.G, dtype=np.uint64))
    rig.eng.restore()
    assert rig.eng.lead_clock_read(np.arange(rig.G, dtype=np.uint64)).tobytes() == cells.tobytes()
    before = [g["cur_term"] for g in rig.groups]
    rig.adopt()
    assert all(rig.groups[i]["cur_term"] == before[i] - (1 if i in set(moved) else 0) for i in range(rig.G))
    rig.check_cells()
    ev = rig.clock()
    for i, g in enumerate(rig.groups):
        if i in set(moved):
            assert ev[i] == L.EV_NEW_TERM and g["led"] and g["tag"] == g["cur_term"] and (g["hb"], g["el"]) == (1, 1), (i, ev[i], g)
        else:
            assert not ev[i] & L.EV_NEW_TERM and (g["hb"], g["el"]) == (0, 3), (i, ev[i], g)
    rig.clock()
    rig.close()
