"""GPU: the hand-off between the follower arena and the leader columns (rg_follow_promote / _promote_device / rg_follow_demote /
_demote_device) against tests/handoff_model.py, against the road a host takes today (rg_follow_read, whole-column rg_load_column,
one tick with RG_MF_BECOME_LEADER) on a second engine, and against the oracle's tick: every column of every group, bit for bit.
No test provokes a device fault: every bad argument is refused on the host, every bad dense cell is an ANSWER."""
import numpy as np
import pytest

import elect_model as M
import gate_model as G
import handoff_model as H
import handoff_rig as R
import oracle_lib as O
from test_follow_gate_gpu import canon_of, soft_array, soft_of, states_array
from test_follow_elect_gpu import cells_array, cells_of

pytestmark = pytest.mark.gpu

GATE = G.Config(5, flags=G.PRE_VOTE, seed=9)
LOAD_COLS = O.STATE_COLS + O.TERM_TABLE_COLS + ("out",)
READ_COLS = R.ALL_COLS + ("out", "host_hint")
OUT_SENT = 0x7F
U64_SENT = 0xA5A5A5A5A5A5A5A5


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


class Rig:
    """A leader engine of SHAPES[P] x P with a follower arena of 257 groups (stride 512), gate and election cells enabled."""

    def __init__(self, rg, P, ix64=False, elect=True, arena=True, **kw):
        self.rg, self.E, self.P, self.G, self.n = rg, rg.engine, P, H.SHAPES[P], H.N_FOLLOW
        self.eng = rg.Engine(self.G, P, flags=self.E.CFGF.IX64 if ix64 else None, **kw)
        assert self.eng.device_info()["last_tick_offset_bits"] in (0, 32, 64)
        self.all = np.arange(self.n, dtype=np.uint64)
        if arena:
            self.eng.follow_enable(self.n)
            self.stride = self.eng.follow_stride()
            assert self.stride == 512
            if elect:
                self.eng.follow_gate_enable(GATE.election_tick, GATE.min_timeout, GATE.max_timeout, GATE.flags, GATE.seed)
                self.eng.follow_elect_enable()

    def close(self):
        self.eng.sync()
        self.eng.close()

    def load_lead(self, st):
        for k in LOAD_COLS:
            self.eng.load_column(self.E.COL.NAMES.index(k), st[k])

    def read_lead(self):
        st = {"n_groups": self.G, "n_slots": self.P, "stride": self.eng.stride}
        for k in READ_COLS:
            st[k] = self.eng.read_column(self.E.COL.NAMES.index(k))
        return st

    def load_arena(self, cases):
        gs = [c.g for c in cases]
        self.eng.follow_write(states_array(self.E, gs, [c.f.canonical() for c in cases]))
        self.eng.follow_soft_write(soft_array(self.E, gs, [c.soft() for c in cases]))
        with_cells = [c for c in cases if c.cells()]
        self.eng.follow_elect_write(cells_array(self.E, [c.g for c in with_cells], [c.cells() for c in with_cells]))

    def arena(self):
        logs, softs, cells = self.eng.follow_read(self.all), self.eng.follow_soft_read(self.all), self.eng.follow_elect_read(self.all)
        return [(canon_of(a), soft_of(b), cells_of(c)) for a, b, c in zip(logs, softs, cells)]

    def recs(self, cases):
        a = np.zeros(len(cases), dtype=self.E.HANDOFF_REC_DTYPE)
        for k, c in enumerate(cases):
            a[k]["follow_group"], a[k]["lead_group"] = c.g, c.L
            a[k]["persisted"] = c.f.canonical()["last_index"] if c.persisted is None else c.persisted
        return a

    def out_columns(self):
        import torch
        return {"status": torch.full((self.stride,), OUT_SENT, dtype=torch.uint8, device="cuda"),
                "term": torch.full((self.stride,), U64_SENT - (1 << 64), dtype=torch.int64, device="cuda"),
                "last_index": torch.full((self.stride,), U64_SENT - (1 << 64), dtype=torch.int64, device="cuda")}

    def dense_answers(self, out, cases, answers):
        """the dense form's columns against the sparse form's answers: status for every group below n_follow and nothing
        beyond it, term and last_index where the status is DONE, their sentinel everywhere else"""
        status = out["status"].cpu().numpy()
        term, last = (out[k].cpu().numpy().view(np.uint64) for k in ("term", "last_index"))
        want = {c.g: a for c, a in zip(cases, answers)}
        assert (status[self.n:] == OUT_SENT).all()
        for g in range(self.stride):
            a = want.get(g)
            assert g >= self.n or int(status[g]) == (a[0] if a else H.NONE), (g, int(status[g]), a)
            if a and a[0] == H.DONE:
                assert (int(term[g]), int(last[g])) == (a[1], a[2]), (g, a)
            else:
                assert int(term[g]) == U64_SENT and int(last[g]) == U64_SENT, g

    def promote(self, cases, dense, answers, vouch=False):
        """promote `cases` and compare every answer field with the model's `answers`"""
        if not dense:
            got = self.eng.follow_promote(self.recs(cases))
            assert [tuple(int(r[k]) for k in ("status", "term", "last_index", "commit", "out")) for r in got] == answers
            return
        result, lead, persisted = np.zeros(self.stride, np.uint8), np.full(self.stride, U64_SENT, np.uint64), np.full(self.stride, U64_SENT, np.uint64)
        result[:self.n] = np.arange(self.n) % M.WON  # every value but WON selects nothing, whatever the lead column holds
        for c, r in zip(cases, self.recs(cases)):
            result[c.g], lead[c.g], persisted[c.g] = M.WON, c.L, r["persisted"]
        out = self.out_columns()
        cols = (dev(result), dev(lead), None if vouch else dev(persisted))
        self.eng.follow_promote_device(cols[0], cols[1], out, cols[2])
        self.eng.sync()
        self.dense_answers(out, cases, answers)

    def demote(self, pairs, dense):
        """[(follow group, lead group)] -> [(status, term, last_index, commit)] (the dense form: commit from the lead column)"""
        if not dense:
            a = np.zeros(len(pairs), dtype=self.E.HANDOFF_REC_DTYPE)
            for k, (g, L) in enumerate(pairs):
                a[k]["follow_group"], a[k]["lead_group"], a[k]["persisted"] = g, L, U64_SENT
            got = self.eng.follow_demote(a)
            assert not got["out"].any()
            return [tuple(int(r[k]) for k in ("status", "term", "last_index", "commit")) for r in got]
        select, lead = np.zeros(self.stride, np.uint8), np.full(self.stride, U64_SENT, np.uint64)
        for g, L in pairs:
            select[g], lead[g] = 1 + g % 250, L
        out = self.out_columns()
        cols = (dev(select), dev(lead))
        self.eng.follow_demote_device(cols[0], cols[1], out)
        self.eng.sync()
        status = out["status"].cpu().numpy()
        term, last = (out[k].cpu().numpy().view(np.uint64) for k in ("term", "last_index"))
        sel = {g for g, _ in pairs}
        assert (status[self.n:] == OUT_SENT).all() and all(int(status[g]) == H.NONE for g in range(self.n) if g not in sel)
        assert all(int(term[g]) == U64_SENT for g in range(self.stride) if g not in sel or status[g] != H.DONE)
        commit = self.eng.read_column(self.E.COL.COMMIT)
        return [(int(status[g]), int(term[g]), int(last[g]), int(commit[L])) if status[g] == H.DONE else (int(status[g]), 0, 0, 0) for g, L in pairs]


def same_but_out(a, b, what):
    d = R.diff(a, b)
    assert not d, (what, d)


# ---------------------------------------------------------------------------------------------------------------------
# 1 + 2. the existing route is the yardstick; the edges, sparse and dense, 32- and 64-bit cell offsets
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ix64", [False, True])
@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("P", [3, 8])
def test_promotion_equals_the_existing_route_the_oracle_and_the_model(rg, P, dense, ix64):
    cases = H.gpu_cases(P)
    a, b = Rig(rg, P, ix64), Rig(rg, P, ix64, arena=False)
    st = R.state_with(a.G, P, a.eng.stride, cases)
    want, answers = R.model_state(st, cases)
    a.load_lead(st)
    a.load_arena(cases)
    before_lead, before_arena = a.read_lead(), a.arena()
    same_but_out(st, before_lead, "the load")  # (RG_COL_RUN_COUNT and the PEND bits as the engine derives them)
    a.promote(cases, dense, answers)
    got = a.read_lead()
    same_but_out(want, got, "promotion against the model")
    assert (got["out"] == st["out"]).all() and (got["out"] == before_lead["out"]).all() and (got["host_hint"] == before_lead["host_hint"]).all()
    assert a.arena() == before_arena, "a promotion leaves all three layers of the arena alone"
    for c in cases:  # the cells of absent slots keep their sentinel
        for s in range(P):
            if not H.cfg_fields(c.lead["cfg"])[4] >> s & 1:
                assert all(int(got[k][s, c.L]) == H.SENTINEL for k in H.SLOT_KEYS), (c.name, s)
    # the road available today, on a second engine: rg_follow_read, whole columns, one tick with RG_MF_BECOME_LEADER alone
    logs = {int(r["group"]): canon_of(r) for r in a.eng.follow_read(np.array([c.g for c in cases], dtype=np.uint64))}
    assert all(logs[c.g] == c.f.canonical() for c in cases)
    route, msgs = R.route_state(st, cases)
    b.load_lead(st)
    for k in ("commit", "term_lo", "term_hi", "run_first", "run_term", "dummy_index", "dummy_term", "cur_term", "match"):
        b.eng.load_column(b.E.COL.NAMES.index(k), route[k])
    mb = rg.MsgBuffers(b.G, P, b.eng.stride)
    mb.m_flags[...], mb.m_hint[...] = msgs["m_flags"], msgs["m_hint"]
    b.eng.tick(mb)
    via_tick = b.read_lead()
    same_but_out(via_tick, got, "promotion against the existing route")
    done = [c for c in cases if c.expect == H.DONE]
    assert all(int(via_tick["out"][c.L]) == 0x18 for c in done) and int(np.count_nonzero(via_tick["out"] & 0x18)) == len(done)
    after, gout = R.oracle_tick(route, msgs)
    same_but_out(after, got, "promotion against the oracle")
    assert (gout == via_tick["out"]).all()
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dense", [False, True])
def test_refusals_change_nothing(rg, dense):
    cases = H.refusal_cases() + [c for c in H.gpu_cases(3) if c.name in ("one_run", "last_2_63_minus_1")]
    r = Rig(rg, 3)
    st = R.state_with(r.G, 3, r.eng.stride, cases)
    want, answers = R.model_state(st, cases)
    assert sorted({a[0] for a in answers}) == [H.DONE, H.NOT_WON, H.CONF, H.NOT_PERSISTED, H.FAULT]
    r.load_lead(st)
    r.load_arena(cases)
    before_arena = r.arena()
    r.promote(cases, dense, answers)
    got = r.read_lead()
    same_but_out(want, got, "refusals")  # (`want` differs from the load in the one promoted group only)
    for c in cases:
        if c.expect != H.DONE:
            assert R.get_lead(got, c.L) == R.get_lead(st, c.L), c.name
    assert (got["out"] == st["out"]).all() and r.arena() == before_arena
    if dense:  # a lead group beyond the engine is an answer, and persisted == NULL vouches for last_index
        bad = H.Case("beyond", 200, r.G, cases[-2].f, cases[-2].lead, None, H.FAULT)
        r.load_arena([H.Case("x", 200, 0, cases[-2].f, cases[-2].lead)])
        result, lead = np.zeros(r.stride, np.uint8), np.zeros(r.stride, np.uint64)
        result[[200, 60]], lead[200], lead[60] = M.WON, r.G, 70  # (group 60: NOT_PERSISTED above, DONE once the host vouches)
        out = r.out_columns()
        cols = (dev(result), dev(lead))
        r.eng.follow_promote_device(cols[0], cols[1], out, None)
        r.eng.sync()
        status = out["status"].cpu().numpy()
        others = (np.arange(r.n) != 200) & (np.arange(r.n) != 60)
        assert int(status[200]) == H.FAULT == bad.expect and int(status[60]) == H.DONE and not status[:r.n][others].any()
        vouched = r.read_lead()
        c60 = next(c for c in cases if c.g == 60)
        m = H.copy_lead(c60.lead)
        assert H.promote(c60.f, m, 3)[0] == H.DONE and R.get_lead(vouched, 70) == m
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. round trips
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("P,ix64", [(3, False), (8, True)])
def test_round_trips(rg, P, dense, ix64):
    cases = [c for c in H.gpu_cases(P) if c.expect == H.DONE]
    r = Rig(rg, P, ix64)
    st = R.state_with(r.G, P, r.eng.stride, cases)
    want, answers = R.model_state(st, cases)
    r.load_lead(st)
    r.load_arena(cases)
    r.promote(cases, dense, answers, vouch=all(c.persisted is None for c in cases))
    # promote then demote: the old log plus one entry of term T, through rg_follow_read
    before_lead, before_arena = r.read_lead(), r.arena()
    got = r.demote([(c.g, c.L) for c in cases], dense)
    after_arena = r.arena()
    for c, a in zip(cases, got):
        (status, term, last, commit), canon = H.demote(R.get_lead(want, c.L))
        old = c.f.canonical()
        assert a == (status, term, last, commit) == (H.DONE, c.f.term, old["last_index"] + 1, old["committed"]), (c.name, a)
        assert canon["runs"] == (old["runs"] + [(old["last_index"] + 1, c.f.term)])[-H.FOLLOW_RUNS:], c.name
        assert after_arena[c.g] == (canon,) + before_arena[c.g][1:], (c.name, after_arena[c.g][0], canon)  # soft and election cells untouched
        if c.name.endswith("eight_older_plus_tail") or c.name == "all_eight_group_commit":
            assert canon["runs"][0][0] > canon["dummy_index"] + 1, "the dropped run reads back as a declared gap"
    touched = {c.g for c in cases}
    assert all(after_arena[g] == before_arena[g] for g in range(r.n) if g not in touched)
    lead_after = r.read_lead()
    same_but_out(before_lead, lead_after, "a demotion leaves the leader columns alone")
    assert (lead_after["out"] == before_lead["out"]).all()
    # a group loaded directly into the leader columns is demoted, wins at T + 1 and is promoted again
    g2, L2 = 129, 5
    d = R.get_lead(lead_after, L2)  # a quiet base group: entries 1..3 of term 2
    (status, term, last, commit), canon = H.demote(d)
    assert r.demote([(g2, L2)], dense) == [(H.DONE, 2, 3, 2)] == [(status, term, last, commit)]
    f = H.Follower(canon, term + 1, 3, range(P), (), 0)
    again = H.Case("again", g2, L2, f, d)
    r.eng.follow_soft_write(soft_array(r.E, [g2], [again.soft()]))
    r.eng.follow_elect_write(cells_array(r.E, [g2], [again.cells()]))
    assert r.arena()[g2][0] == canon
    m = H.copy_lead(d)
    a = H.promote(f, m, P)
    assert a == (H.DONE, 3, 4, 2, 0x18)
    r.promote([again], dense, [a], vouch=True)
    assert R.get_lead(r.read_lead(), L2) == m
    # ... and a table that is not canonical is an answer: nothing of the arena changes
    bad = R.copy_state(lead_after)
    bad["commit"][6] = 9  # beyond last_index
    r.eng.load_column(r.E.COL.COMMIT, bad["commit"])
    before_arena = r.arena()
    assert r.demote([(130, 6)], dense) == [(H.FAULT, 0, 0, 0)] and r.arena() == before_arena
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. a storm with no host synchronisation inside
# ---------------------------------------------------------------------------------------------------------------------
def test_storm_from_timeout_to_a_ticking_leader_without_a_host_round_trip(rg):
    import torch
    from test_follow_elect_gpu import U8_COLS, U64_COLS
    P, r = 3, Rig(rg, 3)
    E, eng, S = r.E, r.eng, r.stride
    winners = [0, 1, 63, 64, 255, 256]
    lead_of = {g: 299 - 7 * k for k, g in enumerate(winners)}
    log = H.canon(0, 0, [(1, 1), (4, 2)], 6, 5)
    nodes = {}
    for g in winners:
        nd = M.Node(GATE, g, H.log_of(log), self_id=2, incoming=(0, 1, 2), self_slot=1)
        nd.load(2, 0, 1, 0, G.FOLLOWER, 0, 0, True)  # a follower of peer 1 at term 2 ...
        nd.elapsed = nd.timeout - 1                  # ... whose election timeout fires on the next tick
        nodes[g] = nd
    st = R.base_state(r.G, P, eng.stride)
    for g in winners:  # the lead groups' cfg words name this store's slot
        st["cfg"][lead_of[g]] = H.mask((0, 1, 2)) | 1 << 16 | 7 << 24
    r.load_lead(st)
    eng.follow_write(states_array(E, winners, [nodes[g].log.canonical() for g in winners]))
    eng.follow_soft_write(soft_array(E, winners, [nodes[g].soft() for g in winners]))
    eng.follow_elect_write(cells_array(E, winners, [nodes[g].cells() for g in winners]))
    # everything the chain reads is on the device before it starts: the peers' answers of both rounds, the lead column, the acks
    def round_cols(kind, term):
        cols = {k: np.zeros(S, np.uint8) for k in ("kind", "slot", "reject")}
        cols.update({k: np.zeros(S, np.uint64) for k in ("term", "commit", "commit_term")})
        for g in winners:
            cols["kind"][g], cols["slot"][g], cols["term"][g] = kind, 0, term
        return {k: dev(v) for k, v in cols.items()}
    pre, real = round_cols(M.PREVOTE, 3), round_cols(M.VOTE, 3)
    lead = np.full(S, U64_SENT, np.uint64)
    for g in winners:
        lead[g] = lead_of[g]
    d_lead = dev(lead)
    acks = rg.MsgBuffers(r.G, P, eng.stride)
    for g in winners:
        for s in (0, 2):
            acks.m_flags[lead_of[g], s], acks.m_index[s, lead_of[g]] = 0x01, 7
    d_acks = {k: dev(getattr(acks, k)) for k in ("m_index", "m_commit", "m_hint", "m_rs", "m_flags")}

    def elect_out(size):
        o = {k: torch.full((size,), OUT_SENT, dtype=torch.uint8, device="cuda") for k in U8_COLS}
        o.update({k: torch.zeros(size, dtype=torch.int64, device="cuda") for k in U64_COLS})
        return o
    hup = torch.zeros(S, dtype=torch.int64, device="cuda")
    o_camp, o_pre, o_real, o_hand = elect_out(S), elect_out(S), elect_out(S), r.out_columns()
    torch.cuda.synchronize()
    # ---- the chain: queued back to back, one synchronisation at the end ----
    assert eng.follow_clock(hup, S, sync=False) is None
    eng.follow_campaign_device(hup, eng.follow_clock_counts(), S, o_camp)
    eng.follow_vote_resps_device(pre, o_pre)
    eng.follow_vote_resps_device(real, o_real)
    eng.follow_promote_device(o_real["result"], d_lead, o_hand)
    eng.tick_device(d_acks["m_index"].data_ptr(), d_acks["m_commit"].data_ptr(), d_acks["m_hint"].data_ptr(), d_acks["m_rs"].data_ptr(),
                    d_acks["m_flags"].data_ptr())
    eng.sync()
    # ---- the models: hup, the pre-vote round, the vote round, the promotion, the oracle's tick over the acks ----
    for g in winners:
        nd = nodes[g]
        assert nd.tick()
        assert nd.record(M.Rec(M.HUP))[0] == M.REQUESTS and nd.role == G.PRE_CANDIDATE
        assert nd.record(M.Rec(M.PREVOTE, term=3, frm=0))[0] == M.REQUESTS and nd.role == G.CANDIDATE and nd.term == 3
        assert nd.record(M.Rec(M.VOTE, term=3, frm=0))[0] == M.WON and nd.lead == nd.self_id
    result = o_real["result"].cpu().numpy()
    assert sorted(int(g) for g in np.nonzero(result[:r.n] == M.WON)[0]) == winners
    arena = r.arena()
    for g in winners:
        assert arena[g] == (nodes[g].log.canonical(), nodes[g].soft(), nodes[g].cells()), g
    cases = [H.Case("storm%d" % g, g, lead_of[g], H.Follower(log, 3, 2, (0, 1, 2), (), 1), R.get_lead(st, lead_of[g])) for g in winners]
    promoted, answers = R.model_state(st, cases)
    assert all(a == (H.DONE, 3, 7, 5, 0x18) for a in answers)
    r.dense_answers(o_hand, cases, answers)
    after, gout = R.oracle_tick(promoted, acks.as_dict())
    got = r.read_lead()
    same_but_out(after, got, "the tick behind the promotion against the oracle")
    assert (got["out"] == gout).all()
    for g in winners:  # the empty entry of term 3 is committed by the two acks, in the new term
        L = lead_of[g]
        assert (int(got["commit"][L]), int(got["term_lo"][L]), int(got["term_hi"][L]), int(got["cur_term"][L])) == (7, 7, 7, 3) and got["out"][L] & 1
        assert [int(got["match"][s, L]) for s in range(3)] == [7, 6, 7]
    r.close()


def test_read_index_across_a_promotion(rg):
    """A read queued at the old term is gone after the promotion; a new one is RG_READ_NOT_READY until the tick that commits
    the new leader's empty entry, and accepted after it."""
    r = Rig(rg, 3)
    E, eng, L, g = r.E, r.eng, 17, 40
    st = R.base_state(r.G, 3, eng.stride)
    st["cfg"][L] = H.mask((0, 1, 2)) | 1 << 16 | 7 << 24
    st["match"][:, L] = (2, 3, 2)
    r.load_lead(st)
    eng.read_index_enable(4)
    assert list(eng.read_index([(L, 11)])) == [E.READ_QUEUED] and eng.read_pending_counts()[L] == 1
    case = H.Case("read", g, L, H.Follower(H.canon(0, 0, [(1, 2)], 3, 2), 5, 2, (0, 1, 2), (), 1), R.get_lead(st, L))
    r.load_arena([case])
    r.promote([case], False, [(H.DONE, 5, 4, 2, 0x18)])
    assert list(eng.read_index([(L, 12)])) == [E.READ_NOT_READY]
    acks = rg.MsgBuffers(r.G, 3, eng.stride)
    for s in (0, 1):  # peer 0 acks the empty entry and the leader has persisted it
        acks.m_flags[L, s], acks.m_index[s, L] = 0x01, 4
    eng.tick(acks)
    assert int(eng.read_column(E.COL.COMMIT)[L]) == 4
    assert list(eng.read_index([(L, 13)])) == [E.READ_QUEUED]
    assert eng.read_pending_counts()[L] == 1 and int(eng.read_last_pending()[L]) == 13  # (the read of the old term went with the term)
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. API states
# ---------------------------------------------------------------------------------------------------------------------
def test_api_states(rg):
    E = rg.engine
    one_rec = np.zeros(1, dtype=E.HANDOFF_REC_DTYPE)

    def code(call):
        with pytest.raises(rg.EngineError) as ei:
            call()
        return ei.value.code

    # before the layers are enabled: promotion needs all three, demotion the first
    r = Rig(rg, 3, arena=False)
    r.stride = 512
    r.load_lead(R.base_state(r.G, 3, r.eng.stride))  # (every group a quiet leader: entries 1..3 of term 2, commit 2)
    cols, out = dev(np.zeros(512, np.uint8)), r.out_columns()
    lead = dev(np.zeros(512, np.uint64))
    calls = [lambda: r.eng.follow_promote(one_rec), lambda: r.eng.follow_promote_device(cols, lead, out),
             lambda: r.eng.follow_demote(one_rec), lambda: r.eng.follow_demote_device(cols, lead, out)]
    assert [code(c) for c in calls] == [E.ERR["STATE"]] * 4
    r.eng.follow_enable(r.n)
    assert [code(c) for c in calls[:2]] == [E.ERR["STATE"]] * 2
    r.eng.follow_gate_enable(5)
    assert [code(c) for c in calls[:2]] == [E.ERR["STATE"]] * 2
    lead_before = r.read_lead()
    assert tuple(int(r.eng.follow_demote(one_rec)[0][k]) for k in ("status", "term", "last_index", "commit")) == (H.DONE, 2, 3, 2)
    r.eng.follow_demote_device(cols, lead, out)
    r.eng.follow_elect_enable()
    # bad records: refused on the host, nothing applied
    arena_before = r.arena()
    for bad in ([(r.n, 0)], [(0, r.G)], [(1, 5), (1, 6)], [(1, 5), (2, 5)]):
        a = np.zeros(len(bad), dtype=E.HANDOFF_REC_DTYPE)
        for k, (g, L) in enumerate(bad):
            a[k]["follow_group"], a[k]["lead_group"] = g, L
        assert code(lambda: r.eng.follow_promote(a)) == E.ERR["INVALID_ARG"] and code(lambda: r.eng.follow_demote(a)) == E.ERR["INVALID_ARG"]
    for bad_out in ({**out, "status": None}, {**out, "last_index": None}):
        assert code(lambda: r.eng.follow_promote_device(cols, lead, bad_out)) == E.ERR["INVALID_ARG"]
        assert code(lambda: r.eng.follow_demote_device(cols, lead, bad_out)) == E.ERR["INVALID_ARG"]
    assert code(lambda: r.eng.follow_promote_device(cols, None, out)) == E.ERR["INVALID_ARG"]
    r.eng.sync()
    assert r.arena() == arena_before
    same_but_out(lead_before, r.read_lead(), "refused calls")
    assert len(r.eng.follow_promote(one_rec[:0])) == 0 and len(r.eng.follow_demote(one_rec[:0])) == 0
    r.close()
    # device Inflights: promotion is left out, demotion is allowed
    r = Rig(rg, 3, max_inflight=8)
    r.load_lead(R.base_state(r.G, 3, r.eng.stride))
    out = r.out_columns()
    assert code(lambda: r.eng.follow_promote(one_rec)) == E.ERR["STATE"] and code(lambda: r.eng.follow_promote_device(cols, lead, out)) == E.ERR["STATE"]
    assert int(r.eng.follow_demote(one_rec)[0]["status"]) == H.DONE
    r.eng.follow_demote_device(cols, lead, out)
    r.close()


def test_mirrored_engine(rg):
    """rg_set_peers: the dense forms are refused; the sparse promotion refuses a lead group with queued mirror events and
    registers T in the mirror's gate -- a response of term T is applied, one of the old term dropped."""
    E = rg.engine
    r = Rig(rg, 3)
    L, g = 9, 33
    st = R.base_state(r.G, 3, r.eng.stride)
    st["cfg"][L] = H.mask((0, 1, 2)) | 1 << 16 | 7 << 24
    st["match"][:, L] = (2, 3, 1)
    r.load_lead(st)
    for grp in range(r.G):
        r.eng.set_peers(grp, [101, 102, 103], 2)
    case = H.Case("mirror", g, L, H.Follower(H.canon(0, 0, [(1, 2)], 3, 3), 6, 102, (0, 1, 2), (), 1), R.get_lead(st, L))
    r.load_arena([case])
    cols, lead, out = dev(np.zeros(r.stride, np.uint8)), dev(np.zeros(r.stride, np.uint64)), r.out_columns()
    for call in (lambda: r.eng.follow_promote_device(cols, lead, out), lambda: r.eng.follow_demote_device(cols, lead, out)):
        with pytest.raises(rg.EngineError) as ei:
            call()
        assert ei.value.code == E.ERR["STATE"]
    r.eng.step(L, 101, 2, 3)  # an ack of the old term waits in the mirror's queue
    with pytest.raises(rg.EngineError) as ei:
        r.eng.follow_promote(r.recs([case]))
    assert ei.value.code == E.ERR["SLOT_BUSY"]
    r.eng.flush()
    assert int(r.eng.read_column(E.COL.MATCH)[0, L]) == 3 and int(r.eng.read_column(E.COL.COMMIT)[L]) == 3
    lead_dict = R.get_lead(r.read_lead(), L)
    m = H.copy_lead(lead_dict)
    a = H.promote(case.f, m, 3)
    r.promote([case], False, [a])
    assert a == (H.DONE, 6, 4, 3, 0x18) and R.get_lead(r.read_lead(), L) == m
    r.eng.step(L, 103, 2, 3)   # the old term: dropped by the gate
    r.eng.step(L, 101, 6, 4)   # the new leader's term: applied
    r.eng.flush()
    match = r.eng.read_column(E.COL.MATCH)
    assert [int(match[s, L]) for s in range(3)] == [4, 3, 0] and int(r.eng.read_column(E.COL.COMMIT)[L]) == 3
    with pytest.raises(rg.EngineError) as ei:
        r.eng.step(L, 103, 7, 4)
    assert ei.value.code == E.ERR["HIGHER_TERM"]
    r.close()
