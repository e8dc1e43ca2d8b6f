"""GPU: nobody led twice. The same follow groups are promoted into the same lead positions ten times over -- into Progress cells
the previous leadership left, a STOPPED clock cell with the previous term's tag, and a term-run table that the step-down
exported and the promotion imports again until it overflows (RG_TERM_RUNS 8, RG_FOLLOW_RUNS 9). Each leadership is one device
chain without a host round trip inside it: rg_follow_promote_device, rgx_lead_clock twice (acks from nobody: the election
timeout of clock config (2, 1, CHECK_QUORUM)), rgx_follow_step_down_device. After every chain every cell is compared with the
composed models: handoff_model (promotion, demotion), lead_clock_model (the clock, the step-down), gate_model (become_follower).
In the first test the win itself is written by the host (rg_follow_soft_write: Follower, leader_id == self_id at the next term)
over the log shapes of handoff_model's edge list, stale cells are planted before one promotion and the logs grow between two
others; in the second the election runs on the device too, against elect_model. No test provokes a device fault."""
import numpy as np
import pytest

import elect_model as M
import gate_model as G
import handoff_model as H
import handoff_rig as R
import lead_clock_model as L
import readonly_model as RO
from test_follow_gate_gpu import soft_array, states_array
from test_handoff_gpu import Rig, dev
from life_cycle_rig import CLOCK, ClockModel, elect_out, node_of, vote_round

pytestmark = pytest.mark.gpu

LEADERSHIPS = 10
CFG = H.mask((0, 1, 2)) | 1 << 16 | 7 << 24
SELF_ID = 7
# (log shape of handoff_model.LOG_EDGES, follow group, lead group): lanes 0, 63, 64 and 256 of the arena, scattered lead positions
ROWS = (("empty_dummy0", 0, 299), ("one_run", 63, 5), ("eight_older_plus_tail", 64, 130), ("gap_present", 256, 64))


def test_ten_leaderships_per_position(rg):
    """Four log shapes of the hand-off's edge list, ten terms each: after every chain the promotion's answers (term, the index of
    the term's empty entry), every leader column, the clock cells and events (NEW_TERM with the counters restarted, then the
    step-down), the step-down's answers and the winners' three arena layers are the models'; every other arena group is untouched.
    Before the sixth promotion one lead group gets what a busy leadership leaves (Progress moved, a recent_active peer with a
    pending snapshot, a transferee); after the fourth and the seventh the logs grow, so that the runs differ in length."""
    import random
    import torch
    rng = random.Random(10)
    rig = Rig(rg, 3)
    E, eng, S = rig.E, rig.eng, rig.stride
    cases = [H.Case(name, g, Lg, H.Follower(H.LOG_EDGES[name][0], H.LOG_EDGES[name][1], SELF_ID, (0, 1, 2), (), 1), H.make_lead(3, CFG, rng)) for name, g, Lg in ROWS]
    rig.load_lead(R.state_with(rig.G, 3, eng.stride, cases))
    rig.load_arena(cases)
    eng.lead_clock_enable(CLOCK.election_tick, CLOCK.heartbeat_tick, CLOCK.flags)  # every group stopped: a promotion arms its lead group
    model = ClockModel(rig, CLOCK)
    untouched = rig.arena()
    result, lead = np.zeros(S, np.uint8), np.full(S, L.NO_LEAD, np.uint64)
    for c in cases:
        result[c.g], lead[c.g] = M.WON, c.L
    d_result, d_lead = dev(result), dev(lead)
    term = {c.g: c.f.term for c in cases}
    dropped = set()
    for k in range(LEADERSHIPS):
        if k == 5:  # what a busy leadership leaves behind in lead group 130: Progress moved, a peer recent_active with a pending snapshot, a transferee
            st = rig.read_lead()
            st["match"][0, 130], st["next"][0, 130], st["pend_snap"][0, 130] = 5, 6, 17
            st["pflags"][130, 0] = H.REPLICATE | L.PF_RECENT_ACTIVE | H.PF_PEND_SNAP
            st["cfg"][130] = int(st["cfg"][130]) | 3 << 20
            rig.load_lead(st)
        if k:  # the next win, as the election would leave it: Follower with leader_id == self_id at the next term
            eng.follow_soft_write(soft_array(E, [c.g for c in cases], [(term[c.g], SELF_ID, SELF_ID, 0, G.FOLLOWER, 0, 0, 1) for c in cases]))
        before, st = rig.arena(), rig.read_lead()
        if k == 5:
            assert int(st["cfg"][130]) >> 20 & 0xF == 3 and int(st["pflags"][130, 0]) & L.PF_RECENT_ACTIVE and int(st["pend_snap"][0, 130]) == 17
        o_hand, o_down = rig.out_columns(), rig.out_columns()
        events = [torch.full((eng.stride,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        # ---- the device chain: one synchronisation at its end ----
        eng.follow_promote_device(d_result, d_lead, o_hand)
        eng.lead_clock(events[0], sync=False)
        eng.lead_clock(events[1], sync=False)
        eng.follow_step_down_device(events[1], d_lead, o_down)
        eng.sync()
        # ---- the models ----
        want, answers = R.copy_state(st), []
        for c in cases:
            f = H.Follower(before[c.g][0], term[c.g], SELF_ID, (0, 1, 2), (), 1)
            m = R.get_lead(st, c.L)
            answers.append(H.promote(f, m, 3))
            last = before[c.g][0]["last_index"]
            assert answers[-1] == (H.DONE, term[c.g], last + 1, before[c.g][0]["committed"], 0x18), (k, c.name, answers[-1])  # the empty entry of the term
            R.put_lead(want, c.L, m)
            d = R.get_lead(want, c.L)  # every Progress cell is become_leader's, whatever the last leadership left
            assert d["match"] == [0, last, 0] and d["next"] == [last + 1] * 3 and d["pflags"][0] & 0x0B == d["pflags"][2] & 0x0B == H.PROBE and d["cfg"] >> 20 & 0xF == 0
            assert d["run_count"] == min(len(before[c.g][0]["runs"]), H.TERM_RUNS)
        rig.dense_answers(o_hand, cases, answers)
        seen = []
        for t in range(2):
            for i, g in enumerate(model.groups):
                d = R.get_lead(want, i)
                g.update(cfg=d["cfg"], cur_term=d["cur_term"], commit=d["commit"], match=d["match"], pflags=d["pflags"] + [0] * 5)
            seen.append(model.tick())
            for i, g in enumerate(model.groups):
                want["cfg"][i] = g["cfg"]
                want["pflags"][i, :3] = g["pflags"][:3]
        ev = events[0].cpu().numpy()
        assert [int(x) for x in ev[:rig.G]] == seen[0] and (ev[rig.G:] == 0xEE).all()
        leads = [c.L for c in cases]
        assert all(seen[0][i] == (L.EV_NEW_TERM | L.EV_BEAT if i in leads else 0) for i in range(rig.G))  # armed lazily: counters (1, 1), the beat is due at once
        assert all(seen[1][i] == (L.EV_CHECK_QUORUM | L.EV_STEPPED_DOWN if i in leads else 0) for i in range(rig.G))
        arena_want, downs = list(before), []
        for c in cases:
            node = node_of(c.g, before[c.g][1], before[c.g][2])
            a, canon = L.step_down(node, R.get_lead(want, c.L), model.groups[c.L])
            assert a == (H.DONE, term[c.g], before[c.g][0]["last_index"] + 1, before[c.g][0]["committed"]), (k, c.name, a)
            downs.append(a + (0,))
            arena_want[c.g] = (canon, node.soft(), before[c.g][2])
            # the run table: the log of this leadership is one run more, and beyond RG_FOLLOW_RUNS the oldest is dropped
            runs = before[c.g][0]["runs"] + [(a[2], a[1])]
            if len(runs) > H.FOLLOW_RUNS:
                dropped.add(c.name)
            assert canon["runs"] == runs[-H.FOLLOW_RUNS:] and H.state_check(canon) == 0, (k, c.name, canon)
        model.check(events[1], seen[1])
        got = rig.read_lead()
        assert not R.diff(want, got, R.ALL_COLS + ("out",)), (k, R.diff(want, got, R.ALL_COLS + ("out",)))
        rig.dense_answers(o_down, cases, downs)
        after = rig.arena()
        assert after == arena_want, (k, [(g, after[g], arena_want[g]) for g in range(rig.n) if after[g] != arena_want[g]][:2])
        assert all(after[g] == untouched[g] for g in range(rig.n) if g not in term)
        for c in cases:
            term[c.g] += 1
        if k in (3, 6):  # entries appended while leading, as a follower would hold them afterwards: the runs differ in length
            grown = []
            for c in cases:
                canon = dict(after[c.g][0])
                canon["last_index"] += 2 + k % 3
                canon["committed"] = canon["last_index"] - 1
                grown.append(canon)
            eng.follow_write(states_array(E, [c.g for c in cases], grown))
    assert dropped == {c.name for c in cases}  # every table overflowed, the one that began empty after leadership 9
    rig.close()


GATE_LOG = H.canon(0, 0, [(1, 1), (4, 2)], 6, 5)  # the log every winner starts with, at term 2
WINNERS = {0: 299, 63: 5, 64: 130, 256: 64}        # follow group -> lead group
BUSY = 4                                           # the leadership that appends, is acknowledged, queues a read and begins a transfer
MF_VALID, MF_APPEND = 0x01, 0x20


def test_ten_elections_won_on_the_device(rg):
    """The same ten leaderships with the election on the device as well: per cycle rg_follow_clock to the timeout (the host writes
    election_elapsed three ticks short of it), rg_follow_campaign_device, both vote rounds, rg_follow_promote_device on the vote
    round's result column, the clock up to the step-down and rgx_follow_step_down_device behind every clock call -- ONE
    synchronisation at the end of the cycle, then every cell of the winners' arena layers, of the leader columns and of the clock
    against elect_model / gate_model, handoff_model, the oracle's tick and lead_clock_model composed.
    Leadership BUSY runs the existing tick in front of every clock call: the peers acknowledge the term's empty entry while the
    leader appends and persists two entries, then acknowledge those -- Progress moves, RECENT_ACTIVE is set, and the acks of the
    new term carry the group past its first CHECK_QUORUM; the host queues a read and names a transferee; two silent ticks later
    the group steps down and exports a run of three entries. The promotion behind it finds nothing of that: the read queue is
    empty and the old term's acks release nothing, the clock reports NEW_TERM with its counters restarted, every Progress cell is
    become_leader's."""
    import torch
    from test_follow_elect_gpu import cells_array
    from test_handoff_gpu import GATE
    r = Rig(rg, 3)
    E, eng, S, P = r.E, r.eng, r.stride, 3
    winners = sorted(WINNERS)
    nodes = {}
    for g in winners:
        nd = M.Node(GATE, g, H.log_of(GATE_LOG), self_id=2, incoming=(0, 1, 2), self_slot=1)
        nd.load(2, 0, 1, 0, G.FOLLOWER, 0, 0, True)
        nodes[g] = nd
    st = R.base_state(r.G, P, eng.stride)
    for g in winners:
        st["cfg"][WINNERS[g]] = CFG
    r.load_lead(st)
    eng.follow_write(states_array(E, winners, [nodes[g].log.canonical() for g in winners]))
    eng.follow_soft_write(soft_array(E, winners, [nodes[g].soft() for g in winners]))
    eng.follow_elect_write(cells_array(E, winners, [nodes[g].cells() for g in winners]))
    eng.lead_clock_enable(CLOCK.election_tick, CLOCK.heartbeat_tick, CLOCK.flags)
    model = ClockModel(r, CLOCK)
    lead = np.full(S, L.NO_LEAD, np.uint64)
    for g in winners:
        lead[g] = WINNERS[g]
    d_lead = dev(lead)
    cases = [H.Case("w%d" % g, g, WINNERS[g], None, None) for g in winners]

    hup = torch.full((S,), -1, dtype=torch.int64, device="cuda")
    eng.read_index_enable(2)
    leads = set(WINNERS.values())
    ctx_of = {Lg: 0x5000 + Lg for Lg in leads}  # the read each lead group queues in its busy leadership

    def busy_ticks(last):
        """The messages of the busy leadership's four ticks, `last` = the index of the term's empty entry: the peers acknowledge
        it while the leader appends and persists two entries; the peers acknowledge those; then silence."""
        ticks = [rg.MsgBuffers(r.G, P, eng.stride) for _ in range(4)]
        for Lg in leads:
            for s in (0, 2):
                ticks[0].m_flags[Lg, s], ticks[0].m_index[s, Lg] = MF_VALID, last
                ticks[1].m_flags[Lg, s], ticks[1].m_index[s, Lg] = MF_VALID, last + 2
            ticks[0].m_flags[Lg, 1], ticks[0].m_index[1, Lg], ticks[0].m_commit[1, Lg] = MF_VALID | MF_APPEND, last + 2, last + 2
        return ticks
    overflowed = False
    for k in range(LEADERSHIPS):
        T = 3 + k
        for g in winners:  # at most three ticks away from the timeout
            nodes[g].elapsed = nodes[g].timeout - 3
        eng.follow_soft_write(soft_array(E, winners, [nodes[g].soft() for g in winners]))
        if k:  # what the group learned while it followed: everything it holds is committed (a campaign needs term(committed), and
            for g in winners:  # a commit index the overflowing table no longer covers is the host's to answer)
                canon = dict(nodes[g].log.canonical())
                canon["committed"] = canon["last_index"]
                nodes[g].log = H.log_of(canon)
            eng.follow_write(states_array(E, winners, [nodes[g].log.canonical() for g in winners]))
        before_lead = r.read_lead()
        empty_entry = nodes[winners[0]].log.canonical()["last_index"] + 1
        assert all(nodes[g].log.canonical()["last_index"] + 1 == empty_entry for g in winners)
        n_calls = 4 if k == BUSY else 2
        ticks = busy_ticks(empty_entry) if k == BUSY else [None] * n_calls
        keep = [[dev(getattr(m, c)) for c in ("m_index", "m_commit", "m_hint", "m_rs", "m_flags")] if m else None for m in ticks]
        pre, real = vote_round(S, winners, M.PREVOTE, T), vote_round(S, winners, M.VOTE, T)
        o_camp, o_pre, o_real, o_hand = elect_out(S), elect_out(S), elect_out(S), r.out_columns()
        o_downs = [r.out_columns() for _ in range(n_calls)]
        events = [torch.full((eng.stride,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(n_calls)]
        torch.cuda.synchronize()
        # ---- the device chain: one synchronisation at its end (the busy leadership and the one behind it stop once in the middle,
        #      where the host queues a read and names a transferee, and where it looks at the queue the promotion found) ----
        for _ in range(3):
            eng.follow_clock(hup, S, sync=False)
            eng.follow_campaign_device(hup, eng.follow_clock_counts(), S, o_camp)
        eng.follow_vote_resps_device(pre, o_pre)
        eng.follow_vote_resps_device(real, o_real)
        eng.follow_promote_device(o_real["result"], d_lead, o_hand)
        for t in range(n_calls):
            if keep[t]:
                eng.tick_device(*[x.data_ptr() for x in keep[t]])
            eng.lead_clock(events[t], sync=False)
            eng.follow_step_down_device(events[t], d_lead, o_downs[t])
            if k == BUSY and t == 1:  # both peers acked, the term's entry is committed: a read queues; then a transfer begins
                reqs = [(Lg, ctx_of[Lg]) for Lg in sorted(leads)]
                assert [int(x) for x in eng.read_index(reqs)] == [RO.QUEUED] * len(reqs)
                counts, pending = eng.read_pending_counts(), eng.read_last_pending()
                assert all(int(counts[Lg]) == 1 and int(pending[Lg]) == ctx_of[Lg] for Lg in leads)
                for Lg in leads:
                    eng.set_config(Lg, CFG | 3 << 20)
            if k == BUSY + 1 and t == 0:  # the promotion behind the busy leadership, armed by this clock call: nothing of the old term is left
                counts, pending = eng.read_pending_counts(), eng.read_last_pending()
                assert not counts.any() and not pending.any()
                eng.read_acks([(Lg, ctx_of[Lg], s, 0) for Lg in leads for s in range(P)])  # the acks the old term's read waited for
                assert len(eng.read_states()) == 0
                cells = eng.lead_clock_read(sorted(leads))
                assert all((int(c["term"]), int(c["led"]), int(c["heartbeat_elapsed"]), int(c["election_elapsed"])) == (T, 1, 0, 1) for c in cells)  # (1, 1): the heartbeat counter wraps at heartbeat_tick 1
        eng.sync()
        # ---- the models ----
        want, answers = R.copy_state(before_lead), []
        for g in winners:
            nd = nodes[g]
            assert [nd.tick() for _ in range(3)] == [False, False, True], (k, g)
            assert nd.record(M.Rec(M.HUP))[0] == M.REQUESTS and nd.role == G.PRE_CANDIDATE, (k, g)
            assert nd.record(M.Rec(M.PREVOTE, term=T, frm=0))[0] == M.REQUESTS and nd.role == G.CANDIDATE and nd.term == T, (k, g)
            assert nd.record(M.Rec(M.VOTE, term=T, frm=0))[0] == M.WON and nd.lead == nd.self_id, (k, g)
            m = R.get_lead(before_lead, WINNERS[g])
            last, committed = nd.log.canonical()["last_index"], nd.log.canonical()["committed"]
            answers.append(H.promote(nd, m, P))
            assert answers[-1] == (H.DONE, T, last + 1, committed, 0x18) and committed == (last if k else 5), (k, g, answers[-1])
            R.put_lead(want, WINNERS[g], m)
            d = R.get_lead(want, WINNERS[g])  # every Progress cell is become_leader's, whatever the busy leadership left
            assert d["match"] == [0, last, 0] and d["next"] == [last + 1] * 3 and d["pflags"][0] & 0x0B == d["pflags"][2] & 0x0B == H.PROBE and d["cfg"] == CFG
        if k == BUSY + 1:  # ... and it did leave something: Progress moved, the peers recent_active at some point, a transferee until the step-down
            assert all(int(before_lead["match"][s, Lg]) == empty_entry - 1 and int(before_lead["next"][s, Lg]) >= empty_entry for Lg in leads for s in (0, 2))
        assert sorted(int(g) for g in np.nonzero(o_real["result"].cpu().numpy()[:r.n] == M.WON)[0]) == winners
        r.dense_answers(o_hand, cases, answers)
        seen = []
        for t in range(n_calls):
            if ticks[t]:
                want, _ = R.oracle_tick(want, ticks[t].as_dict())  # the existing tick: an ack moves its Progress and makes it recent_active
            if k == BUSY and t == 2:
                for Lg in leads:
                    want["cfg"][Lg] = CFG | 3 << 20
            for i, grp in enumerate(model.groups):
                d = R.get_lead(want, i)
                grp.update(cfg=d["cfg"], cur_term=d["cur_term"], commit=d["commit"], match=d["match"], pflags=d["pflags"] + [0] * 5)
            seen.append(model.tick())
            for i, grp in enumerate(model.groups):
                want["cfg"][i] = grp["cfg"]
                want["pflags"][i, :P] = grp["pflags"][:P]
            ev = events[t].cpu().numpy()
            assert [int(x) for x in ev[:r.G]] == seen[t], (k, t, [(i, int(ev[i]), w) for i, w in enumerate(seen[t]) if int(ev[i]) != w][:5])
            if t < n_calls - 1:
                r.dense_answers(o_downs[t], cases, [(H.NONE, 0, 0, 0, 0)] * len(cases))
        assert all(seen[0][i] == (L.EV_NEW_TERM | L.EV_BEAT if i in leads else 0) for i in range(r.G))
        assert all(seen[-1][i] == (L.EV_CHECK_QUORUM | L.EV_STEPPED_DOWN if i in leads else 0) for i in range(r.G))
        if k == BUSY:  # the acks of the new term carried the group past its first CHECK_QUORUM; the transferee went with the step-down
            assert all(seen[1][Lg] == L.EV_BEAT | L.EV_CHECK_QUORUM and seen[2][Lg] == L.EV_BEAT for Lg in leads)
            assert all(int(want["cfg"][Lg]) == CFG and int(want["commit"][Lg]) == int(want["term_hi"][Lg]) == empty_entry + 2 for Lg in leads)
        downs, arena_want = [], {}
        for g in winners:
            nd = nodes[g]
            runs = nd.log.canonical()["runs"] + [(nd.log.canonical()["last_index"] + 1, T)]
            a, canon = L.step_down(nd, R.get_lead(want, WINNERS[g]), model.groups[WINNERS[g]])
            assert a[0] == H.DONE and canon["runs"] == runs[-H.FOLLOW_RUNS:], (k, g, a, canon)
            assert canon["last_index"] == empty_entry + (2 if k == BUSY else 0)  # the run of the busy term is three entries long
            overflowed |= len(runs) > H.FOLLOW_RUNS
            downs.append(a + (0,))
            nd.log = H.log_of(canon)
            assert nd.log.canonical() == canon
            arena_want[g] = (canon, nd.soft(), nd.cells())
        model.check(events[-1], seen[-1])
        got = r.read_lead()
        cols = R.ALL_COLS + (() if k == BUSY else ("out",))  # (RG_COL_OUT is the tick's: test_parity_gpu.py pins it)
        assert not R.diff(want, got, cols), (k, R.diff(want, got, cols))
        r.dense_answers(o_downs[-1], cases, downs)
        arena = r.arena()
        for g in winners:
            assert arena[g] == arena_want[g], (k, g, arena[g], arena_want[g])
    assert overflowed
    r.close()
