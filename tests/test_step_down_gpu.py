"""GPU: the way back into the follower arena (rgx_follow_step_down / _device) and the life of a group from its promotion to its
step-down and on to its next election timeout, against tests/lead_clock_model.py composed with gate_model and handoff_model: every
answer field, every cell of the arena's three layers, the leader columns and the clock cells. No test provokes a device fault:
every bad argument is refused on the host, every bad dense cell is an ANSWER."""
import numpy as np
import pytest

import elect_model as M
import gate_model as G
import handoff_model as H
import handoff_rig as R
import lead_clock_model as L
from life_cycle_rig import CLOCK, ClockModel, elect_out, expect_arena, node_of, promoted_rig, tick_until_down, vote_round
from test_follow_elect_gpu import cells_array
from test_follow_gate_gpu import soft_array, states_array
from test_handoff_gpu import GATE, U64_SENT, Rig, dev

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize("ix64", [False, True])
def test_step_down_dense_equals_sparse_equals_the_model(rg, ix64):
    """Promote, tick to the step-down, take the groups back: the dense form selects by the clock's event column (NO_LEAD and
    unselected groups get status 0, a lead value beyond n_groups FAULT), the arena afterwards is rg_follow_demote followed by the
    model's become_follower(term, 0), the leader columns are untouched, the sparse form gives the same answers and cells."""
    rig, cases, done = promoted_rig(rg, ix64)
    events, counts = tick_until_down(rig)
    ev = events.cpu().numpy()
    assert counts[2] == len(done) and all(ev[c.L] == L.EV_CHECK_QUORUM | L.EV_STEPPED_DOWN for c in done)
    cells = rig.eng.lead_clock_read([c.L for c in done])
    assert not cells["led"].any() and not cells["election_elapsed"].any()
    lead_state, before = rig.read_lead(), rig.arena()
    pairs = [(c.g, c.L) for c in done]
    want, answers = expect_arena(before, lead_state, pairs)
    assert all(a[0] == H.DONE for a in answers)
    rig.eng.checkpoint()
    lead = np.full(rig.stride, L.NO_LEAD, np.uint64)
    for g, Lg in pairs:
        lead[g] = Lg
    lead[3], lead[4], lead[300] = 5, rig.G, 0  # a lead group that did not step down; not a group (FAULT); beyond n_follow (never read)
    out = rig.out_columns()
    d_lead = dev(lead)
    rig.eng.follow_step_down_device(events, d_lead, out)
    rig.eng.sync()
    fault = H.Case("bad_lead", 4, 0, None, None)
    rig.dense_answers(out, [c for c in done] + [fault], [a + (0,) for a in answers] + [(H.FAULT, 0, 0, 0, 0)])
    after = rig.arena()
    assert after == want, [(g, after[g], want[g]) for g in range(rig.n) if after[g] != want[g]][:3]
    for g, _ in pairs:
        assert after[g][1][2] == 0 and after[g][1][5] == 0 and after[g][1][0] == before[g][1][0] and after[g][1][1] == before[g][1][1]
    assert not R.diff(lead_state, rig.read_lead(), R.ALL_COLS + ("out",))
    assert not rig.eng.lead_clock_read([c.L for c in done])["led"].any()
    # ... the sparse form from the same state
    rig.eng.restore()
    assert rig.arena() == before
    recs = np.zeros(len(pairs), dtype=rig.E.HANDOFF_REC_DTYPE)
    recs["follow_group"], recs["lead_group"], recs["persisted"] = [p[0] for p in pairs], [p[1] for p in pairs], U64_SENT
    got = rig.eng.follow_step_down(recs)
    assert [tuple(int(r[k]) for k in ("status", "term", "last_index", "commit")) for r in got] == answers and not got["out"].any()
    assert rig.arena() == want and not R.diff(lead_state, rig.read_lead(), R.ALL_COLS + ("out",))
    rig.close()


def test_refusals_in_order_leave_everything_untouched(rg):
    """NOT_WON (a fresh follow group: self_id 0), FAULT twice (soft.term != RG_COL_CUR_TERM[L], for a group whose promotion was
    refused and for a promoted group paired with another lead group): every cell of both sides as it was. Bad arguments are host
    errors, and so is a call before rg_follow_elect_enable."""
    rig, cases, done = promoted_rig(rg)
    tick_until_down(rig)
    lead_state, before = rig.read_lead(), rig.arena()
    refused = next(c for c in cases if c.expect != H.DONE)  # its soft cells say "won" at a term its lead group never got
    pairs = [(50, 60), (refused.g, refused.L), (done[0].g, 61)]
    want, answers = expect_arena(before, lead_state, pairs)
    assert [a[0] for a in answers] == [H.NOT_WON, H.FAULT, H.FAULT] and want == before
    recs = np.zeros(len(pairs), dtype=rig.E.HANDOFF_REC_DTYPE)
    recs["follow_group"], recs["lead_group"] = [p[0] for p in pairs], [p[1] for p in pairs]
    got = rig.eng.follow_step_down(recs)
    assert [tuple(int(r[k]) for k in ("status", "term", "last_index", "commit", "out")) for r in got] == [a + (0,) for a in answers]
    assert rig.arena() == before and not R.diff(lead_state, rig.read_lead(), R.ALL_COLS + ("out",))
    for field, value in (("follow_group", rig.n), ("lead_group", rig.G), ("follow_group", 50), ("lead_group", 60)):
        bad = recs.copy()
        bad[field][2] = value
        with pytest.raises(rg.EngineError):
            rig.eng.follow_step_down(bad)
    assert rig.arena() == before
    rig.close()
    bare = Rig(rg, 3, elect=False)
    with pytest.raises(rg.EngineError) as ei:
        bare.eng.follow_step_down(recs)
    assert "rg_follow_elect_enable first" in str(ei.value)
    bare.close()


def test_a_device_promotion_arms_the_clock_lazily(rg):
    """RG_COL_CUR_TERM changed by rg_follow_promote_device BETWEEN two clock calls, into stopped cells and into led ones: the next
    call reports NEW_TERM with counters 1 and 1 and the cell led, whatever it held; no hand-off kernel knows of the clock. A group
    stepped down (sparse) before the clock saw its promotion is stopped with the new tag and is NOT re-armed."""
    import torch
    c = L.Config(6, 3, L.CHECK_QUORUM)
    rig = Rig(rg, 3)
    cases = H.gpu_cases(3)
    st = R.state_with(rig.G, 3, rig.eng.stride, cases)
    rig.load_lead(st)
    rig.load_arena(cases)
    done = [k for k in cases if k.expect == H.DONE]
    rig.eng.lead_clock_enable(c.election_tick, c.heartbeat_tick, c.flags)  # every group starts stopped
    model = ClockModel(rig, c)
    led = [k.L for k in done[::2]] + [200, 201]  # half of the lead groups to be promoted into, and two others, are led already
    cells = np.zeros(len(led), dtype=rig.E.LEAD_CLOCK_CELL_DTYPE)
    for k, i in enumerate(led):
        g = model.groups[i]
        g["led"], g["el"], g["hb"] = True, 4, 2 - k % 2
        cells[k]["group"], cells[k]["term"], cells[k]["election_elapsed"], cells[k]["heartbeat_elapsed"], cells[k]["led"] = i, g["tag"], g["el"], g["hb"], 1
    rig.eng.lead_clock_write(cells)
    events = torch.full((rig.eng.stride,), 0xEE, dtype=torch.uint8, device="cuda")
    rig.eng.lead_clock(events)
    model.check(events, model.tick())
    _, answers = R.model_state(st, cases)
    rig.promote(cases, True, answers, vouch=True)
    lead_state = model.adopt()
    assert all(model.groups[k.L]["tag"] != model.groups[k.L]["cur_term"] for k in done)
    early = done[1]  # taken back before the clock has seen its promotion
    arena = rig.arena()
    node = node_of(early.g, arena[early.g][1], arena[early.g][2])
    a, canon = L.step_down(node, R.get_lead(lead_state, early.L), model.groups[early.L])
    recs = np.zeros(1, dtype=rig.E.HANDOFF_REC_DTYPE)
    recs["follow_group"], recs["lead_group"] = early.g, early.L
    got = rig.eng.follow_step_down(recs)
    assert a[0] == H.DONE and tuple(int(got[0][k]) for k in ("status", "term", "last_index", "commit")) == a
    assert rig.arena()[early.g] == (canon, node.soft(), arena[early.g][2])
    want = model.tick()
    rig.eng.lead_clock(events)
    model.check(events, want)
    for k in done:
        g = model.groups[k.L]
        if k is early:
            assert want[k.L] == 0 and not g["led"] and g["tag"] == g["cur_term"] and (g["hb"], g["el"]) == (0, 0)
        else:
            assert want[k.L] == L.EV_NEW_TERM and g["led"] and (g["hb"], g["el"]) == (1, 1)
    assert want[200] & L.EV_CHECK_QUORUM and want[201] & L.EV_CHECK_QUORUM  # (the led bystanders reached their election timeout meanwhile)
    rig.close()


LIFE = L.Config(5, 2, L.CHECK_QUORUM)  # heartbeat_tick above 1, election_tick = 2 * heartbeat_tick + 1
LIFE_TICKS = 11                         # two election timeouts


def test_life_cycle_from_the_election_timeout_to_the_next_one(rg):
    """The point of the feature, with no per-group state crossing to the host between the first rg_follow_clock and the last
    step-down: followed groups tick until they are due, campaign, win both rounds and are promoted on the device; the clock arms
    them lazily and ticks them; the groups whose peers answer through the existing tick stay leaders and beat exactly every
    heartbeat_tick ticks, the silent ones step down at the tick the model names and are taken back; then they tick as followers
    again and are due at the model's tick, with the freshly drawn timeout. Against gate_model / elect_model (the election),
    handoff_model and the oracle's tick (the promotion, the acks), lead_clock_model (the clock, the step-down), composed."""
    import torch
    P, r = 3, Rig(rg, 3)
    E, eng, S = r.E, r.eng, r.stride
    winners = [0, 1, 63, 64, 255, 256]
    answered, silent = winners[::2], winners[1::2]
    lead_of = {g: 299 - 7 * k for k, g in enumerate(winners)}
    log = H.canon(0, 0, [(1, 1), (4, 2)], 6, 5)
    nodes = {}
    for g in winners:
        nd = M.Node(GATE, g, H.log_of(log), self_id=2, incoming=(0, 1, 2), self_slot=1)
        nd.load(2, 0, 1, 0, G.FOLLOWER, 0, 0, True)
        nd.elapsed = nd.timeout - 3  # due on the third tick from here
        nodes[g] = nd
    st = R.base_state(r.G, P, eng.stride)
    for g in winners:
        st["cfg"][lead_of[g]] = H.mask((0, 1, 2)) | 1 << 16 | 7 << 24
    r.load_lead(st)
    eng.follow_write(states_array(E, winners, [nodes[g].log.canonical() for g in winners]))
    eng.follow_soft_write(soft_array(E, winners, [nodes[g].soft() for g in winners]))
    eng.follow_elect_write(cells_array(E, winners, [nodes[g].cells() for g in winners]))
    eng.lead_clock_enable(LIFE.election_tick, LIFE.heartbeat_tick, LIFE.flags)  # every group stopped: the promotion arms the winners
    model = ClockModel(r, LIFE)

    pre, real = vote_round(S, winners, M.PREVOTE, 3), vote_round(S, winners, M.VOTE, 3)
    lead = np.full(S, L.NO_LEAD, np.uint64)
    for g in winners:
        lead[g] = lead_of[g]
    d_lead = dev(lead)
    acks = rg.MsgBuffers(r.G, P, eng.stride)  # what the peers of an ANSWERED group send in every tick: both acknowledge index 7
    for g in answered:
        for s in (0, 2):
            acks.m_flags[lead_of[g], s], acks.m_index[s, lead_of[g]] = 0x01, 7
    keep = [dev(getattr(acks, k)) for k in ("m_index", "m_commit", "m_hint", "m_rs", "m_flags")]
    d_acks = [t.data_ptr() for t in keep]

    hup = torch.full((S,), -1, dtype=torch.int64, device="cuda")
    o_camp, o_pre, o_real, o_hand = elect_out(S), elect_out(S), elect_out(S), r.out_columns()
    events = [torch.full((eng.stride,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(LIFE_TICKS)]
    downs = [r.out_columns() for _ in range(LIFE_TICKS)]
    beat = [torch.full((r.G,), -1, dtype=torch.int64, device="cuda") for _ in range(LIFE_TICKS)]
    torch.cuda.synchronize()
    # ---- the device chain: one synchronisation at its end ----
    for _ in range(3):  # (the first two calls find nobody due: the campaign behind them consumes an empty list)
        eng.follow_clock(hup, S, sync=False)
        eng.follow_campaign_device(hup, eng.follow_clock_counts(), S, o_camp)
    eng.follow_vote_resps_device(pre, o_pre)
    eng.follow_vote_resps_device(real, o_real)
    eng.follow_promote_device(o_real["result"], d_lead, o_hand)
    for t in range(LIFE_TICKS):
        eng.tick_device(*d_acks)
        eng.lead_clock(events[t], beat[t], r.G, sync=False)
        eng.follow_step_down_device(events[t], d_lead, downs[t])
    eng.sync()
    # ---- the models ----
    for g in winners:
        nd = nodes[g]
        assert [nd.tick() for _ in range(3)] == [False, False, True]
        assert nd.record(M.Rec(M.HUP))[0] == M.REQUESTS and nd.role == G.PRE_CANDIDATE
        assert nd.record(M.Rec(M.PREVOTE, term=3, frm=0))[0] == M.REQUESTS and nd.role == G.CANDIDATE and nd.term == 3
        assert nd.record(M.Rec(M.VOTE, term=3, frm=0))[0] == M.WON and nd.lead == nd.self_id
    assert sorted(int(g) for g in np.nonzero(o_real["result"].cpu().numpy()[:r.n] == M.WON)[0]) == winners
    cases = [H.Case("life%d" % g, g, lead_of[g], H.Follower(log, 3, 2, (0, 1, 2), (), 1), R.get_lead(st, lead_of[g])) for g in winners]
    state, answers = R.model_state(st, cases)
    assert all(a == (H.DONE, 3, 7, 5, 0x18) for a in answers)
    r.dense_answers(o_hand, cases, answers)
    arena_want = {}
    for t in range(LIFE_TICKS):
        state, _ = R.oracle_tick(state, acks.as_dict())  # the existing tick: an ack makes its Progress recent_active
        for i, g in enumerate(model.groups):
            d = R.get_lead(state, i)
            g.update(cfg=d["cfg"], cur_term=d["cur_term"], commit=d["commit"], match=d["match"], pflags=d["pflags"] + [0] * (8 - P))
        want = model.tick()
        for i, g in enumerate(model.groups):  # what the clock wrote: RECENT_ACTIVE bits, the TRANSFEREE bits
            state["cfg"][i] = g["cfg"]
            state["pflags"][i, :P] = g["pflags"][:P]
        ev = events[t].cpu().numpy()
        assert [int(x) for x in ev[:r.G]] == want, (t, [(i, int(ev[i]), w) for i, w in enumerate(want) if int(ev[i]) != w][:5])
        tick_no = t + 1
        for g in answered:
            e = want[lead_of[g]]
            assert bool(e & L.EV_BEAT) == (tick_no % LIFE.heartbeat_tick == 0) and bool(e & L.EV_CHECK_QUORUM) == (tick_no % LIFE.election_tick == 0)
            assert not e & L.EV_STEPPED_DOWN and bool(e & L.EV_NEW_TERM) == (t == 0)
        for g in silent:
            e = want[lead_of[g]]
            assert bool(e & L.EV_STEPPED_DOWN) == (tick_no == LIFE.election_tick) and bool(e & L.EV_BEAT) == (tick_no in (2, 4))
        beats = sorted(int(x) for x in beat[t].cpu().numpy() if x >= 0)
        assert beats == sorted(i for i, e in enumerate(want) if e & L.EV_BEAT)
        status = downs[t]["status"].cpu().numpy()
        for g in winners:
            stepped = g in silent and tick_no == LIFE.election_tick
            assert int(status[g]) == (H.DONE if stepped else H.NONE), (t, g)
            if stepped:  # the way back, on the lead group as this tick left it
                a, canon = L.step_down(nodes[g], R.get_lead(state, lead_of[g]), model.groups[lead_of[g]])
                assert a[0] == H.DONE and int(downs[t]["term"].cpu().numpy().view(np.uint64)[g]) == a[1]
                arena_want[g] = (canon, nodes[g].soft(), nodes[g].cells())
    assert sorted(arena_want) == silent
    got = r.read_lead()
    assert not R.diff(state, got), R.diff(state, got)
    model.check(events[-1], want)
    arena = r.arena()
    for g in winners:
        assert arena[g] == (arena_want[g] if g in silent else (nodes[g].log.canonical(), nodes[g].soft(), nodes[g].cells())), g
    # ---- followers again: due at the model's tick, with the freshly drawn timeout ----
    due_at = {}
    for t in range(GATE.max_timeout):
        n = eng.follow_clock(hup, S)
        got_due = set(int(x) for x in hup.cpu().numpy().view(np.uint64)[:n]) & set(silent)
        want_due = {g for g in silent if nodes[g].tick()}
        assert got_due == want_due, (t, got_due, want_due)
        for g in got_due:
            due_at.setdefault(g, t + 1)
    assert due_at == {g: arena_want[g][1][6] for g in silent}
    r.close()
