"""GPU: the deposition (rgt_follow_depose / _device / _scan_device) and the life of a group from its election to the higher term
that ends its leadership and on to its next campaign, against tests/term_gate_model.py composed with gate_model, elect_model,
handoff_model, lead_clock_model and readonly_model: every answer field, every cell of the arena's three layers, the leader columns
and the clock cells. No test provokes a device fault: every bad argument is refused on the host, every bad dense cell is an ANSWER."""
import numpy as np
import pytest

import elect_model as M
import gate_model as G
import handoff_model as H
import handoff_rig as R
import lead_clock_model as L
import term_gate_model as T
from life_cycle_rig import ClockModel, elect_out, node_of, promoted_rig, vote_round
from test_follow_elect_gpu import cells_array
from test_follow_gate_gpu import records_arrays, soft_array, states_array
from test_handoff_gpu import GATE, U64_SENT, Rig, dev

pytestmark = pytest.mark.gpu

EV_SENT = 0xEE


def gate_call(rig, records, sync=True):
    """One rgt_lead_gate_device over a rig's leader engine: records = {lead group: [(slot, flag byte, term)]} -> (events, new_term,
    filtered flags) device columns and the counts"""
    import torch
    flags, terms = np.zeros((rig.G, 8), np.uint8), np.zeros((rig.P, rig.eng.stride), np.uint64)
    for Lg, recs in records.items():
        for s, f, t in recs:
            flags[Lg, s], terms[s, Lg] = f, t
    d_flags, d_terms = dev(flags.reshape(-1)), dev(terms)
    events = torch.full((rig.eng.stride,), EV_SENT, dtype=torch.uint8, device="cuda")
    new_term = torch.full((rig.eng.stride,), U64_SENT - (1 << 64), dtype=torch.int64, device="cuda")
    counts = rig.eng.lead_gate_device(d_flags, d_terms, events, new_term, sync=sync)
    return events, new_term, d_flags, counts


def expect_deposed(before, lead_state, triples, clocks=None, soft=True):
    """The model's arena after deposing `triples` [(follow group, lead group, T)] -> (arena list, answers)"""
    want, answers = list(before), []
    for g, Lg, new_term in triples:
        canon, soft_cells, cells = before[g]
        node = node_of(g, soft_cells, cells)
        a, c = T.depose(node, R.get_lead(lead_state, Lg), new_term, clocks[Lg] if clocks else None, soft=soft)
        answers.append(a)
        if a[0] == H.DONE:
            want[g] = (c, node.soft(), cells)
    return want, answers


def clock_cells(rig, groups):
    return [(int(r["term"]), int(r["election_elapsed"]), int(r["heartbeat_elapsed"]), int(r["led"])) for r in rig.eng.lead_clock_read(np.array(groups, dtype=np.uint64))]


def lead_column(rig, pairs, extra=()):
    lead = np.full(rig.stride, L.NO_LEAD, np.uint64)
    for g, Lg in list(pairs) + list(extra):
        lead[g] = Lg
    return dev(lead)


@pytest.mark.parametrize("ix64", [False, True])
def test_depose_dense_equals_sparse_equals_the_model(rg, ix64):
    """Promote, let a response of a higher term through the gate, take the groups back: the dense form selects by the gate's event
    column and takes T from its new_term column (NO_LEAD and unselected groups get status 0, a lead value beyond n_groups FAULT);
    the arena afterwards is rg_follow_demote followed by the model's become_follower(T, 0); of the leader columns only the clock
    cells changed. The sparse form WITHOUT a gate call gives the same answers and the same cells on both sides."""
    rig, cases, done = promoted_rig(rg, ix64)
    lead_state, before = rig.read_lead(), rig.arena()
    cur = {c.L: int(lead_state["cur_term"][c.L]) for c in done}
    triples = [(c.g, c.L, cur[c.L] + 1 + k) for k, c in enumerate(done)]
    want, answers = expect_deposed(before, lead_state, triples)
    assert all(a[0] == H.DONE and a[1] == t[2] for a, t in zip(answers, triples))
    rig.eng.checkpoint()
    records = {Lg: [(0, T.MF_VALID, cur[Lg]), (2, T.MF_HEARTBEAT, t)] for _, Lg, t in triples}
    records[5] = [(0, T.MF_VALID, 1), (2, T.MF_VALID, 2)]  # a quiet leader of term 2: one stale record, one of its term
    events, new_term, _, counts = gate_call(rig, records)
    assert counts == (len(done), 1, 0)
    assert clock_cells(rig, [c.L for c in done]) == [(cur[c.L], 0, 0, 0) for c in done]
    out = rig.out_columns()
    d_lead = lead_column(rig, [(g, Lg) for g, Lg, _ in triples], [(3, 5), (4, rig.G), (300, 0)])  # not deposed; not a group (FAULT); beyond n_follow
    rig.eng.follow_depose_device(events, new_term, d_lead, out)
    rig.eng.sync()
    fault = H.Case("bad_lead", 4, 0, None, None)
    rig.dense_answers(out, list(done) + [fault], [a + (0,) for a in answers] + [(H.FAULT, 0, 0, 0, 0)])
    after = rig.arena()
    assert after == want, [(g, after[g], want[g]) for g in range(rig.n) if after[g] != want[g]][:3]
    for g, _, t in triples:  # term = T, vote = 0, leader_id = 0, election_elapsed = 0, the role stays Follower; the election cells are untouched
        assert after[g][1][:3] == (t, 0, 0) and after[g][1][4:6] == (G.FOLLOWER, 0) and after[g][2] == before[g][2]
        assert GATE.min_timeout <= after[g][1][6] < GATE.max_timeout
    assert not R.diff(lead_state, rig.read_lead(), R.ALL_COLS + ("out",))
    cells_dense = clock_cells(rig, range(rig.G))
    # ... the sparse form from the state before the gate
    rig.eng.restore()
    assert rig.arena() == before and clock_cells(rig, [c.L for c in done]) == [(cur[c.L], 0, 0, 1) for c in done]
    recs = np.zeros(len(triples), dtype=rig.E.DEPOSE_REC_DTYPE)
    recs["follow_group"], recs["lead_group"], recs["term"] = [t[0] for t in triples], [t[1] for t in triples], [t[2] for t in triples]
    got = rig.eng.follow_depose(recs)
    assert [tuple(int(r[k]) for k in ("status", "term", "last_index", "commit")) for r in got] == answers and not got["out"].any()
    assert rig.arena() == want and not R.diff(lead_state, rig.read_lead(), R.ALL_COLS + ("out",))
    assert clock_cells(rig, range(rig.G)) == cells_dense
    rig.close()


def test_refusals_in_order_leave_everything_untouched(rg):
    """NOT_WON (a fresh follow group), FAULT four ways (soft.term != RG_COL_CUR_TERM[L] twice, T <= soft.term, a lead log
    rg_follow_demote refuses): every cell of both sides as it was, in the sparse and in the dense form. Bad arguments are host
    errors, and so is a call before rg_follow_elect_enable."""
    rig, cases, done = promoted_rig(rg)
    commit = rig.eng.read_column(rig.E.COL.COMMIT)
    commit[done[2].L] = int(rig.eng.read_column(rig.E.COL.TERM_HI)[done[2].L]) + 5  # committed > last_index: no canonical state
    rig.eng.load_column(rig.E.COL.COMMIT, commit)
    lead_state, before, cells = rig.read_lead(), rig.arena(), clock_cells(rig, range(rig.G))
    refused = next(c for c in cases if c.expect != H.DONE)
    t0 = before[done[0].g][1][0]
    triples = [(50, 60, 9), (refused.g, refused.L, 1 << 40), (done[0].g, done[0].L, t0), (done[1].g, 61, 1 << 40), (done[2].g, done[2].L, 1 << 40)]
    want, answers = expect_deposed(before, lead_state, triples)
    assert [a[0] for a in answers] == [H.NOT_WON, H.FAULT, H.FAULT, H.FAULT, H.FAULT] and want == before
    recs = np.zeros(len(triples), dtype=rig.E.DEPOSE_REC_DTYPE)
    recs["follow_group"], recs["lead_group"], recs["term"] = [t[0] for t in triples], [t[1] for t in triples], [t[2] for t in triples]
    got = rig.eng.follow_depose(recs)
    assert [tuple(int(r[k]) for k in ("status", "term", "last_index", "commit", "out")) for r in got] == [a + (0,) for a in answers]

    def untouched():
        return rig.arena() == before and not R.diff(lead_state, rig.read_lead(), R.ALL_COLS + ("out",)) and clock_cells(rig, range(rig.G)) == cells
    assert untouched()
    events, new_term = np.zeros(rig.eng.stride, np.uint8), np.zeros(rig.eng.stride, np.uint64)
    for _, Lg, t in triples:
        events[Lg], new_term[Lg] = T.EV_DEPOSED, t
    out = rig.out_columns()
    rig.eng.follow_depose_device(dev(events), dev(new_term), lead_column(rig, [(g, Lg) for g, Lg, _ in triples]), out)
    rig.eng.sync()
    status = out["status"].cpu().numpy()
    assert [int(status[g]) for g, _, _ in triples] == [a[0] for a in answers] and untouched()
    for field, value in (("follow_group", rig.n), ("lead_group", rig.G), ("follow_group", 50), ("lead_group", 60), ("reserved", 1)):
        bad = recs.copy()
        bad[field][2] = value
        with pytest.raises(rg.EngineError) as ei:
            rig.eng.follow_depose(bad)
        assert ei.value.code == rig.E.ERR["INVALID_ARG"]
    assert untouched()
    rig.close()
    bare = Rig(rg, 3, elect=False)
    col = dev(np.zeros(bare.stride, np.uint64))
    for call in (lambda: bare.eng.follow_depose(recs), lambda: bare.eng.follow_depose_device(col, col, col, bare.out_columns()),
                 lambda: bare.eng.follow_depose_scan_device(col, col, col, bare.out_columns())):
        with pytest.raises(rg.EngineError) as ei:
            call()
        assert "rg_follow_elect_enable first" in str(ei.value)
    bare.close()


def dense_gated(rig, recs):
    """rg_follow_step_gated_device over [(g, Msg)] -> (device columns of the call, {g: answer tuple})"""
    import torch
    E, S = rig.E, rig.stride
    msgs, hdrs, _ = records_arrays(E, recs)
    cols = {k: np.zeros(S, dtype=np.uint64) for k in ("index", "log_term", "commit", "ent_term")}
    term, frm, flags, n_entries = np.zeros(S, np.uint64), np.zeros(S, np.uint64), np.zeros(S, np.uint8), np.zeros(S, np.uint32)
    for m, h in zip(msgs, hdrs):
        g = int(m["group"])
        flags[g], n_entries[g], term[g], frm[g] = m["flags"], m["n_entries"], h["term"], h["from"]
        for k in cols:
            cols[k][g] = m[k]
    d = {k: dev(v) for k, v in cols.items()}
    d["flags"], d["n_entries"] = dev(flags), torch.from_numpy(n_entries.view(np.int32)).cuda()
    return d, dev(term), dev(frm)


def run_gated(rig, d, d_term, d_from, groups):
    import torch
    S = rig.stride
    out = {k: torch.zeros(S, dtype=torch.int64, device="cuda") for k in ("index", "commit", "conflict", "reject_hint", "log_term", "resp_term")}
    for k in ("status", "gate", "events"):
        out[k] = torch.zeros(S, dtype=torch.uint8, device="cuda")
    rig.eng.follow_step_gated_device(d, d_term, d_from, out, out["gate"], out["events"], out["resp_term"])
    rig.eng.sync()
    o = {k: v.cpu().numpy() for k, v in out.items()}
    return {g: (int(o["gate"][g]), int(o["events"][g]), int(o["resp_term"][g]), int(o["status"][g]), int(o["index"][g]), int(o["commit"][g])) for g in groups}


def test_scan_then_gated_step_equals_the_host_sequence(rg):
    """A new leader's MsgHeartbeat of a higher term arrives in the follower stream for groups this store leads. Engine A: the scan
    form in front of rg_follow_step_gated_device, on that call's own columns. Engine B, its twin: the documented host sequence
    rg_follow_demote, the gated step, rgx_lead_clock_write(led = 0). Same answers, same arena, same leader columns, the same groups
    stopped; a follow group that leads nothing and a led group whose record is of its own term are not selected."""
    A, cases, done = promoted_rig(rg)
    B, _, _ = promoted_rig(rg)
    lead_state, before = A.read_lead(), A.arena()
    cur = {c.L: int(lead_state["cur_term"][c.L]) for c in done}
    recs = [(c.g, G.Msg(G.HEARTBEAT, cur[c.L] + 2 + k, 3, commit=int(lead_state["commit"][c.L]))) for k, c in enumerate(done[:-1])]
    same = done[-1]
    recs.append((same.g, G.Msg(G.HEARTBEAT, cur[same.L], 3, commit=0)))  # of the group's own term: not selected
    recs.append((50, G.Msg(G.HEARTBEAT, 5, 3, commit=0)))               # a plain follower
    groups = [g for g, _ in recs]
    d, d_term, d_from = dense_gated(A, recs)
    pairs = [(c.g, c.L) for c in done]
    out = A.out_columns()
    A.eng.follow_depose_scan_device(d["flags"], d_term, lead_column(A, pairs, [(4, A.G)]), out)
    A.eng.sync()
    selected = [(c.g, c.L, m.term) for c, (_, m) in zip(done[:-1], recs)]
    want, answers = expect_deposed(before, lead_state, selected, soft=False)
    assert all(a[0] == H.DONE for a in answers)
    A.dense_answers(out, list(done[:-1]), [a + (0,) for a in answers])  # (group 4 has no message: its bad lead value is never read)
    assert A.arena() == want  # the log import alone: the soft cells wait for the gated step
    got_a = run_gated(A, d, d_term, d_from, groups)
    # ---- the twin: the host sequence ----
    demote = np.zeros(len(selected), dtype=B.E.HANDOFF_REC_DTYPE)
    demote["follow_group"], demote["lead_group"] = [t[0] for t in selected], [t[1] for t in selected]
    assert (B.eng.follow_demote(demote)["status"] == H.DONE).all()
    msgs, hdrs, ext = records_arrays(B.E, recs)
    resp, gate = B.eng.follow_step_gated(msgs, hdrs, ext)
    got_b = {g: (int(q["gate"]), int(q["events"]), int(q["term"]), int(r["status"]), int(r["index"]), int(r["commit"])) for (g, _), r, q in zip(recs, resp, gate)}
    stop = np.zeros(len(selected), dtype=B.E.LEAD_CLOCK_CELL_DTYPE)
    stop["group"], stop["term"] = [t[1] for t in selected], [cur[t[1]] for t in selected]
    B.eng.lead_clock_write(stop)
    assert got_a == got_b and all(v[0] == B.E.GATE_PASS for v in got_a.values())
    assert A.arena() == B.arena()
    for g, _, t in selected:
        assert A.arena()[g][1][:3] == (t, 0, 3)  # become_follower(m.term, from) ran in the gated step
    assert not R.diff(A.read_lead(), B.read_lead(), R.ALL_COLS + ("out",)) and not R.diff(lead_state, A.read_lead(), R.ALL_COLS + ("out",))
    assert clock_cells(A, range(A.G)) == clock_cells(B, range(B.G))
    assert clock_cells(A, [same.L]) == [(cur[same.L], 0, 0, 1)]
    A.close()
    B.close()


def test_mirror_engine_and_device_inflights(rg):
    """On an engine with a host mirror the gate and the dense forms answer RG_ERR_STATE and the sparse form works; an engine
    with device Inflights runs the whole dense road."""
    rig, cases, done = promoted_rig(rg)
    lead_state, before = rig.read_lead(), rig.arena()
    rig.eng.set_peers(200, [1, 2, 3], 2)
    col8, col64 = dev(np.zeros(rig.eng.stride * 8, np.uint8)), dev(np.zeros(rig.eng.stride * 3, np.uint64))
    for call in (lambda: rig.eng.lead_gate_device(col8, col64, col8, col64), lambda: rig.eng.follow_depose_device(col8, col64, col64, rig.out_columns()),
                 lambda: rig.eng.follow_depose_scan_device(col8, col64, col64, rig.out_columns())):
        with pytest.raises(rg.EngineError) as ei:
            call()
        assert ei.value.code == rig.E.ERR["STATE"] and "host mirror" in str(ei.value)
    triples = [(c.g, c.L, int(lead_state["cur_term"][c.L]) + 3) for c in done]
    want, answers = expect_deposed(before, lead_state, triples)
    recs = np.zeros(len(triples), dtype=rig.E.DEPOSE_REC_DTYPE)
    recs["follow_group"], recs["lead_group"], recs["term"] = [t[0] for t in triples], [t[1] for t in triples], [t[2] for t in triples]
    got = rig.eng.follow_depose(recs)
    assert [tuple(int(r[k]) for k in ("status", "term", "last_index", "commit")) for r in got] == answers and rig.arena() == want
    assert not any(c[3] for c in clock_cells(rig, [c.L for c in done]))
    rig.close()
    # ---- device Inflights: the promotion is the host's there, so the leader columns are loaded as a promotion leaves them ----
    rig = Rig(rg, 3, max_inflight=4)
    cases = H.gpu_cases(3)
    st = R.state_with(rig.G, 3, rig.eng.stride, cases)
    promoted, _ = R.model_state(st, cases)
    rig.load_lead(promoted)
    rig.load_arena(cases)
    rig.eng.lead_clock_enable(10, 3, L.START_LED)
    done = [c for c in cases if c.expect == H.DONE]
    lead_state, before = rig.read_lead(), rig.arena()
    triples = [(c.g, c.L, c.f.term + 1) for c in done]
    want, answers = expect_deposed(before, lead_state, triples)
    events, new_term, _, counts = gate_call(rig, {Lg: [(2, T.MF_VALID | T.MF_SENT, t)] for _, Lg, t in triples})
    assert counts == (len(done), 0, 0)
    out = rig.out_columns()
    rig.eng.follow_depose_device(events, new_term, lead_column(rig, [(g, Lg) for g, Lg, _ in triples]), out)
    rig.eng.sync()
    rig.dense_answers(out, done, [a + (0,) for a in answers])
    assert rig.arena() == want and not any(c[3] for c in clock_cells(rig, [c.L for c in done]))
    rig.close()


def reads_rig(rg):
    """Quiet leaders of term 2 with the ReadIndex layer and the clock (every group led); four followed groups hold the win state
    of four of them. -> (rig, [(follow group, lead group)])"""
    rig = Rig(rg, 3)
    st = R.base_state(rig.G, 3, rig.eng.stride)
    rig.load_lead(st)
    pairs = [(0, 299), (63, 64), (64, 63), (256, 0)]
    cases = [H.Case("reads%d" % g, g, Lg, H.Follower(H.demote(R.get_lead(st, Lg))[1], 2, 2, (0, 1, 2), (), 0), R.get_lead(st, Lg)) for g, Lg in pairs]
    rig.load_arena(cases)
    rig.eng.read_index_enable(4)
    rig.eng.lead_clock_enable(10, 3, L.START_LED)
    reqs = [(Lg, 1000 + Lg) for _, Lg in pairs] + [(5, 1005)]  # ... and a bystander
    assert [int(x) for x in rig.eng.read_index(reqs)] == [rig.E.READ_QUEUED] * len(reqs)
    return rig, pairs, reqs


def ack_round(rig, reqs):
    """A late heartbeat round of the SAME term: slots 1 and 2 acknowledge every context -> the groups whose reads were released"""
    ctx = np.zeros((3, rig.eng.stride), np.uint64)
    for Lg, c in reqs:
        ctx[1, Lg] = ctx[2, Lg] = c
    d = dev(ctx)
    rig.eng.read_acks_device(d.data_ptr())
    rig.eng.sync()
    return sorted(int(s["group"]) for s in rig.eng.read_states())


def test_pending_reads_are_dropped_by_the_gate_and_survive_the_host_sequence(rg):
    """Raft::reset's ReadOnly::new (raft.rs:957) for the higher-term case. Engine A: after the gate call that deposes a group its
    pending count is 0 and a late same-term ack releases nothing through rg_read_acks_device, while the bystander's read is
    released. Engine B, the twin, on the documented host sequence (rg_follow_demote, gated step, rgx_lead_clock_write(led = 0)):
    the same reads survive and ARE released -- the hole this call closes."""
    A, pairs, reqs = reads_rig(rg)
    B, _, _ = reads_rig(rg)
    leads = [Lg for _, Lg in pairs]
    for rig in (A, B):
        counts = rig.eng.read_pending_counts()
        assert [int(counts[Lg]) for Lg in leads + [5]] == [1] * 5
    events, new_term, _, counts = gate_call(A, {Lg: [(1, T.MF_HEARTBEAT, 5)] for Lg in leads})
    assert counts == (4, 0, 0)
    pending = A.eng.read_pending_counts()
    assert [int(pending[Lg]) for Lg in leads] == [0] * 4 and int(pending[5]) == 1 and pending.sum() == 1
    assert [int(x) for x in A.eng.read_last_pending()[leads]] == [0] * 4
    assert ack_round(A, reqs) == [5]
    out = A.out_columns()
    A.eng.follow_depose_device(events, new_term, lead_column(A, pairs), out)
    A.eng.sync()
    assert [int(out["status"].cpu().numpy()[g]) for g, _ in pairs] == [H.DONE] * 4
    assert [A.arena()[g][1][:3] for g, _ in pairs] == [(5, 0, 0)] * 4
    # ---- the twin ----
    demote = np.zeros(4, dtype=B.E.HANDOFF_REC_DTYPE)
    demote["follow_group"], demote["lead_group"] = [g for g, _ in pairs], leads
    assert (B.eng.follow_demote(demote)["status"] == H.DONE).all()
    msgs, hdrs, ext = records_arrays(B.E, [(g, G.Msg(G.HEARTBEAT, 5, 3, commit=0)) for g, _ in pairs])
    _, gate = B.eng.follow_step_gated(msgs, hdrs, ext)
    assert (gate["gate"] == B.E.GATE_PASS).all() and (gate["term"] == 5).all()
    stop = np.zeros(4, dtype=B.E.LEAD_CLOCK_CELL_DTYPE)
    stop["group"], stop["term"] = leads, 2
    B.eng.lead_clock_write(stop)
    pending = B.eng.read_pending_counts()
    assert [int(pending[Lg]) for Lg in leads] == [1] * 4
    assert ack_round(B, reqs) == sorted(leads + [5])
    A.close()
    B.close()


def test_life_cycle_from_the_election_to_the_next_campaign(rg):
    """Followed groups tick until they are due, campaign, win both rounds and are promoted on the device; the per-tick loop
    rgx_lead_clock, rgt_lead_gate_device, rg_tick_device, rgt_follow_depose_device runs four times with ONE synchronisation at its
    end; in the third tick half of the new leaders meet a MsgAppendResponse of term 5 beside an acknowledgement of their own term.
    Those are deposed at that tick and taken back at term 5; the others keep leading and advance. Then the deposed tick as
    followers and campaign at term 6 at the tick the model names."""
    import torch
    P, r = 3, Rig(rg, 3)
    E, eng, S = r.E, r.eng, r.stride
    CLOCK = L.Config(10, 3, L.CHECK_QUORUM)
    TICKS, AT, NEW = 4, 2, 5
    winners = [0, 1, 63, 64, 255, 256]
    stay, go = winners[::2], winners[1::2]
    lead_of = {g: 299 - 7 * k for k, g in enumerate(winners)}
    log = H.canon(0, 0, [(1, 1), (4, 2)], 6, 5)
    nodes = {}
    for g in winners:
        nd = M.Node(GATE, g, H.log_of(log), self_id=2, incoming=(0, 1, 2), self_slot=1)
        nd.load(2, 0, 1, 0, G.FOLLOWER, 0, 0, True)
        nd.elapsed = nd.timeout - 3
        nodes[g] = nd
    st = R.base_state(r.G, P, eng.stride)
    for g in winners:
        st["cfg"][lead_of[g]] = H.mask((0, 1, 2)) | 1 << 16 | 7 << 24
    r.load_lead(st)
    eng.follow_write(states_array(E, winners, [nodes[g].log.canonical() for g in winners]))
    eng.follow_soft_write(soft_array(E, winners, [nodes[g].soft() for g in winners]))
    eng.follow_elect_write(cells_array(E, winners, [nodes[g].cells() for g in winners]))
    eng.lead_clock_enable(CLOCK.election_tick, CLOCK.heartbeat_tick, CLOCK.flags)  # every group stopped: the promotion arms the winners
    model = ClockModel(r, CLOCK)
    pre, real = vote_round(S, winners, M.PREVOTE, 3), vote_round(S, winners, M.VOTE, 3)
    d_lead = lead_column(r, [(g, lead_of[g]) for g in winners])
    acks = rg.MsgBuffers(r.G, P, eng.stride)  # both peers of every new leader acknowledge index 7 in every tick
    for g in winners:
        for s in (0, 2):
            acks.m_flags[lead_of[g], s], acks.m_index[s, lead_of[g]] = T.MF_VALID, 7
    keep = [dev(getattr(acks, k)) for k in ("m_index", "m_commit", "m_hint", "m_rs")]
    terms = [np.zeros((P, eng.stride), np.uint64) for _ in range(TICKS)]
    for t in range(TICKS):
        for g in winners:
            terms[t][0, lead_of[g]], terms[t][2, lead_of[g]] = 3, (NEW if t == AT and g in go else 3)
    d_terms = [dev(x) for x in terms]
    d_flags = [dev(acks.m_flags.reshape(-1).copy()) for _ in range(TICKS)]  # filtered in place, tick by tick
    hup = torch.full((S,), -1, dtype=torch.int64, device="cuda")
    o_camp, o_pre, o_real, o_hand = elect_out(S), elect_out(S), elect_out(S), r.out_columns()
    clock_ev = [torch.full((eng.stride,), EV_SENT, dtype=torch.uint8, device="cuda") for _ in range(TICKS)]
    gate_ev = [torch.full((eng.stride,), EV_SENT, dtype=torch.uint8, device="cuda") for _ in range(TICKS)]
    new_term = [torch.zeros(eng.stride, dtype=torch.int64, device="cuda") for _ in range(TICKS)]
    downs = [r.out_columns() for _ in range(TICKS)]
    torch.cuda.synchronize()
    # ---- the device chain: one synchronisation at its end ----
    for _ in range(3):
        eng.follow_clock(hup, S, sync=False)
        eng.follow_campaign_device(hup, eng.follow_clock_counts(), S, o_camp)
    eng.follow_vote_resps_device(pre, o_pre)
    eng.follow_vote_resps_device(real, o_real)
    eng.follow_promote_device(o_real["result"], d_lead, o_hand)
    for t in range(TICKS):
        eng.lead_clock(clock_ev[t], sync=False)
        eng.lead_gate_device(d_flags[t], d_terms[t], gate_ev[t], new_term[t], sync=False)
        eng.tick_device(*[k.data_ptr() for k in keep], d_flags[t].data_ptr())
        eng.follow_depose_device(gate_ev[t], new_term[t], d_lead, downs[t])
    eng.sync()
    # ---- the models ----
    for g in winners:
        nd = nodes[g]
        assert [nd.tick() for _ in range(3)] == [False, False, True]
        assert nd.record(M.Rec(M.HUP))[0] == M.REQUESTS
        assert nd.record(M.Rec(M.PREVOTE, term=3, frm=0))[0] == M.REQUESTS and nd.term == 3
        assert nd.record(M.Rec(M.VOTE, term=3, frm=0))[0] == M.WON and nd.lead == nd.self_id
    cases = [H.Case("life%d" % g, g, lead_of[g], H.Follower(log, 3, 2, (0, 1, 2), (), 1), R.get_lead(st, lead_of[g])) for g in winners]
    state, answers = R.model_state(st, cases)
    r.dense_answers(o_hand, cases, answers)
    arena_want = {}
    for t in range(TICKS):
        for i, g in enumerate(model.groups):
            d = R.get_lead(state, i)
            g.update(cfg=d["cfg"], cur_term=d["cur_term"], commit=d["commit"], match=d["match"], pflags=d["pflags"] + [0] * (8 - P))
        want_clock = model.tick()
        assert [int(x) for x in clock_ev[t].cpu().numpy()[:r.G]] == want_clock
        rows, want_gate = [], []
        for i, g in enumerate(model.groups):
            row, ev, nt, _, _ = T.gate(g, [int(b) for b in acks.m_flags[i]], [int(x) for x in terms[t][:, i]] + [0] * 5, P)
            rows.append(row)
            want_gate.append(ev)
            if ev & T.EV_DEPOSED:
                assert nt == NEW and int(new_term[t].cpu().numpy()[i]) == NEW
        assert [int(x) for x in gate_ev[t].cpu().numpy()[:r.G]] == want_gate
        assert (d_flags[t].cpu().numpy().reshape(r.G, 8) == np.array(rows, dtype=np.uint8)).all()
        for i, g in enumerate(model.groups):  # what the clock and the gate wrote
            state["cfg"][i] = g["cfg"]
            state["pflags"][i, :P] = g["pflags"][:P]
        msgs = acks.as_dict()
        msgs["m_flags"] = np.array(rows, dtype=np.uint8)
        state, _ = R.oracle_tick(state, msgs)
        status = downs[t]["status"].cpu().numpy()
        for g in winners:
            i = lead_of[g]
            deposed = g in go and t == AT
            assert bool(want_gate[i] & T.EV_DEPOSED) == deposed and int(status[g]) == (H.DONE if deposed else H.NONE), (t, g)
            if t > AT and g in go:
                assert want_gate[i] == T.EV_NOT_LED and rows[i] == [0] * 8
            if deposed:
                a, canon = T.depose(nodes[g], R.get_lead(state, i), NEW, model.groups[i])
                assert a == (H.DONE, NEW, 7, int(state["commit"][i])) and int(downs[t]["term"].cpu().numpy()[g]) == NEW
                arena_want[g] = (canon, nodes[g].soft(), nodes[g].cells())
    assert sorted(arena_want) == go
    got = r.read_lead()
    assert not R.diff(state, got), R.diff(state, got)
    assert clock_cells(r, range(r.G)) == [(g["tag"], g["el"], g["hb"], int(g["led"])) for g in model.groups]
    assert all(model.groups[lead_of[g]]["led"] for g in stay) and not any(model.groups[lead_of[g]]["led"] for g in go)
    arena = r.arena()
    for g in winners:
        assert arena[g] == (arena_want[g] if g in go else (nodes[g].log.canonical(), nodes[g].soft(), nodes[g].cells())), g
    for g in go:
        assert (nodes[g].term, nodes[g].vote, nodes[g].lead, nodes[g].role) == (NEW, 0, 0, G.FOLLOWER)
    # ---- followers again: due at the model's tick; the campaign asks for votes at T + 1 ----
    due_at = {}
    for t in range(GATE.max_timeout):
        n = eng.follow_clock(hup, S)
        got_due = set(int(x) for x in hup.cpu().numpy().view(np.uint64)[:n]) & set(go)
        want_due = {g for g in go if nodes[g].tick()}
        assert got_due == want_due, (t, got_due, want_due)
        if got_due:
            reqs = np.zeros(len(got_due), dtype=E.FOLLOW_CAMPAIGN_REQ_DTYPE)
            reqs["group"] = sorted(got_due)
            resp = eng.follow_campaign(reqs)
            for g, q in zip(sorted(got_due), resp):
                assert nodes[g].record(M.Rec(M.HUP))[0] == M.REQUESTS and nodes[g].role == G.PRE_CANDIDATE
                assert (int(q["result"]), int(q["req_term"])) == (M.REQUESTS, NEW + 1), (g, q)
        for g in got_due:
            due_at.setdefault(g, t + 1)
        if len(due_at) == len(go):
            break
    assert due_at == {g: arena_want[g][1][6] for g in go}
    r.close()
