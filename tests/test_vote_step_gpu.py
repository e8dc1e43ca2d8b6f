"""GPU: the dense vote step (rgv_follow_vote_device / rgv_follow_vote) against tests/vote_step_model.py composed with gate_model,
handoff_model, lead_clock_model, term_gate_model and readonly_model: every answer field, every cell of the arena's three layers,
the leader columns and the clock cells; the not-led half also against rg_follow_step_gated over the same records. No test provokes
a device fault: every bad argument is refused on the host, every bad dense cell is an ANSWER."""
import copy
import random

import numpy as np
import pytest

import elect_model as M
import follower_model as F
import gate_model as G
import handoff_model as H
import handoff_rig as R
import lead_clock_model as L
import term_gate_model as T
import vote_step_model as V
from life_cycle_rig import elect_out, promoted_rig
from test_follow_gate_gpu import Gated, records_arrays
from test_handoff_gpu import Rig, dev

pytestmark = pytest.mark.gpu

B_SENT, U64_SENT = 0x7F, 0xA5A5A5A5A5A5A5A5
ANSWERED = (G.G_VOTE_GRANT, G.G_VOTE_REJECT, G.G_PREVOTE_LOW)


def dense_vote(eng, E, S, n, recs, lead=None, cap=None, other=None, sync=True, wait=True):
    """One rgv_follow_vote_device: recs = [(g, Msg)] (at most one per group), lead = {g: lead group} or None (dev_lead NULL), other =
    {g: flag byte that is no request}, cap = the answered list's capacity (None: no list).
    -> ({g: (status, gate, events, term, commit, log_term)}, counts, the answered places). Every output cell the call must leave
    alone is checked against a sentinel, and every group below n without a request answers 0 / 0 / 0. wait = False: the call is
    launched and nothing is read; -> a function that synchronises and returns the triple."""
    import torch
    cols = {k: np.zeros(S, np.uint64) for k in ("index", "log_term", "commit", "ent_term")}
    term, frm, prio = np.zeros(S, np.uint64), np.zeros(S, np.uint64), np.zeros(S, np.int64)
    flags, hdr = np.zeros(S, np.uint8), np.zeros(S, np.uint8)
    for g, m in recs:
        assert flags[g] == 0
        flags[g], term[g], frm[g], prio[g], hdr[g] = m.kind, m.term, m.frm, m.priority, E.GATE_FORCE if m.force else 0
        cols["index"][g], cols["log_term"][g], cols["commit"][g], cols["ent_term"][g] = m.index, m.log_term, m.commit, m.commit_term
    for g, b in (other or {}).items():
        flags[g], term[g], frm[g] = b, 3, 2
    d = {k: dev(v) for k, v in cols.items()}
    d["flags"] = dev(flags)
    d_lead = None
    if lead is not None:
        col = np.full(S, L.NO_LEAD, np.uint64)
        for g, Lg in lead.items():
            col[g] = Lg
        d_lead = dev(col)
    out = {k: torch.full((S,), B_SENT, dtype=torch.uint8, device="cuda") for k in ("status", "gate", "events")}
    out.update({k: torch.full((S,), U64_SENT - (1 << 64), dtype=torch.int64, device="cuda") for k in ("term", "commit", "log_term")})
    answered = torch.full(((cap or 0) + 2,), U64_SENT - (1 << 64), dtype=torch.int64, device="cuda") if cap is not None else None
    cols_in = (dev(term), dev(frm), dev(prio), dev(hdr))
    torch.cuda.synchronize()
    counts = eng.follow_vote_device(d, cols_in[0], cols_in[1], out, priority=cols_in[2], hdr_flags=cols_in[3], lead=d_lead, answered=answered, answered_cap=cap or 0, sync=sync)

    def collect():
        eng.sync()
        return _collect(out, answered, counts, recs, S, n)
    return collect() if wait else collect


def _collect(out, answered, counts, recs, S, n):
    o = {k: v.cpu().numpy() for k, v in out.items()}
    o = {k: v.view(np.uint64) if v.dtype == np.int64 else v for k, v in o.items()}
    req = np.zeros(S, bool)
    req[[g for g, _ in recs]] = True
    for k in ("status", "gate", "events"):
        assert (o[k][n:] == B_SENT).all() and not o[k][:n][~req[:n]].any(), k
    for k in ("term", "commit", "log_term"):
        assert (o[k][~req] == U64_SENT).all(), k
    got = {g: tuple(int(o[k][g]) for k in ("status", "gate", "events", "term", "commit", "log_term")) for g, _ in recs}
    places = [int(x) for x in answered.cpu().numpy().view(np.uint64)] if answered is not None else None
    return got, counts, places


def check_counts(got, counts, places, cap):
    gates = [a[1] for a in got.values()]
    want = (len(got), gates.count(G.G_VOTE_GRANT), gates.count(G.G_VOTE_REJECT) + gates.count(G.G_PREVOTE_LOW), gates.count(G.G_IGNORED),
            sum(1 for a in got.values() if a[2] & V.EV_DEPOSED))
    assert counts == want, (counts, want)
    if places is not None:
        due = {g for g, a in got.items() if a[1] in ANSWERED}
        k = min(cap, len(due))
        assert len(set(places[:k])) == k and set(places[:k]) <= due and all(p == U64_SENT for p in places[k:]), (places, sorted(due))


def vote_recs(E, recs, lead=None):
    a = np.zeros(len(recs), dtype=E.VOTE_REC_DTYPE)
    for k, (g, m) in enumerate(recs):
        a[k]["follow_group"], a[k]["lead_group"] = g, (lead or {}).get(g, L.NO_LEAD)
        a[k]["term"], a[k]["from"], a[k]["index"], a[k]["log_term"], a[k]["commit"], a[k]["commit_term"] = m.term, m.frm, m.index, m.log_term, m.commit, m.commit_term
        a[k]["priority"], a[k]["kind"], a[k]["flags"] = m.priority, m.kind, E.GATE_FORCE if m.force else 0
    return a


def sparse_answers(resp):
    return [tuple(int(r[k]) for k in ("status", "gate", "events", "term", "commit", "log_term", "last_index")) for r in resp]


# ---------------------------------------------------------------------------------------------------------------------
# 1. not led
# ---------------------------------------------------------------------------------------------------------------------
def test_not_led_dense_equals_the_sparse_gated_step_equals_the_model(rg):
    """n_follow = 600: three blocks, the middle one without a request (other kinds and a two-kind byte only), the last one partial.
    Seeded soft states of all three roles, logs with and without gaps, requests in about half the groups of blocks 0 and 2. From one
    checkpoint: the dense call (dev_lead NULL), rg_follow_step_gated over the same records, the sparse form -- the same answers and
    the same arena, equal to the model; groups without a request keep every cell; the counts and the answered list with a cap below
    the total and without a list."""
    n = 600
    cfg = G.Config(5, flags=G.CHECK_QUORUM | G.PRE_VOTE, seed=21)
    f = Gated(rg, n, cfg)
    E, eng = f.E, f.eng
    eng.follow_elect_enable()
    rng = random.Random(5)
    groups = list(range(n))
    logs = [F.random_log(rng, 12, bounded=True) for _ in groups]
    f.load_many(groups, logs, [G.random_soft(rng, cfg, log) for log in logs])
    recs, other = [], {300: G.APPEND, 301: G.VOTE | G.PREVOTE, 511: G.TOUCH}
    for g in groups:
        if 256 <= g < 512:
            continue
        x = rng.random()
        if x < 0.5:
            m = G.random_msg(rng, f.nodes[g])
            while m.kind not in (G.VOTE, G.PREVOTE):
                m = G.random_msg(rng, f.nodes[g])
            recs.append((g, m))
        elif x < 0.6:
            other[g] = rng.choice((G.APPEND, G.HEARTBEAT, G.TOUCH, G.VOTE | G.PREVOTE, G.VOTE | G.APPEND, 0x20))
    assert {g // 256 for g, _ in recs} == {0, 2} and len(recs) > 150
    before = (f.read_soft(), f.read_logs())
    eng.checkpoint()
    want = {g: V.step_follower(f.nodes[g], m) for g, m in recs}  # (the model's nodes move on)
    assert {a[1] for a in want.values()} >= {G.G_IGNORED, G.G_PREVOTE_LOW, G.G_VOTE_GRANT, G.G_VOTE_REJECT} and F.HOST in {a[0] for a in want.values()}
    total = sum(1 for a in want.values() if a[1] in ANSWERED)
    cap = total // 2
    got, counts, places = dense_vote(eng, E, f.stride, n, recs, cap=cap, other=other)
    assert got == {g: a[:6] for g, a in want.items()}, [(g, got[g], want[g]) for g in got if got[g] != want[g][:6]][:4]
    check_counts(got, counts, places, cap)
    f.check_state("dense")
    touched = {g for g, _ in recs}
    after = (f.read_soft(), f.read_logs())
    assert all(after[0][g] == before[0][g] and after[1][g] == before[1][g] for g in groups if g not in touched)
    # ---- the parent's way: the sparse gated step over the same records ----
    eng.restore()
    assert (f.read_soft(), f.read_logs()) == before
    msgs, hdrs, ext = records_arrays(E, recs)
    resp, gate = eng.follow_step_gated(msgs, hdrs, ext)
    gated = {g: (int(r["status"]), int(q["gate"]), int(q["events"]), int(q["term"]), int(r["commit"]), int(r["log_term"])) for (g, _), r, q in zip(recs, resp, gate)}
    assert gated == got
    assert (f.read_soft(), f.read_logs()) == after
    # ---- the sparse form; then the dense one without a list, asynchronous, and two malformed requests ----
    eng.restore()
    assert sparse_answers(eng.follow_vote(vote_recs(E, recs))) == [want[g] for g, _ in recs]
    assert (f.read_soft(), f.read_logs()) == after
    eng.restore()
    bad = [(300, G.Msg(G.VOTE, 0, 2)), (302, G.Msg(G.PREVOTE, 4, 0))]
    got2, none, _ = dense_vote(eng, E, f.stride, n, recs + bad, other={301: G.VOTE | G.PREVOTE}, sync=False)
    assert none is None and {g: got2[g] for g, _ in recs} == got and all(got2[g] == V.FAULT_ANSWER[:6] for g, _ in bad)
    from test_follow_gate_gpu import device_u64
    assert tuple(device_u64(eng.follow_vote_counts(), 5)) == (counts[0] + 2,) + counts[1:]
    assert (f.read_soft(), f.read_logs()) == after
    f.close()


def test_an_arena_of_more_tiles_than_blocks(rg):
    """The dense launch has at most 1024 blocks and a block walks the tiles blockIdx.x, blockIdx.x + 1024, ...: at 1024 * 256 + 300
    groups block 0 makes a second trip and block 1 a partial one. Requests in the first, the last-of-the-first-trip, the two second-trip
    tiles; every other group of every tile answers 0 / 0 / 0, nothing beyond n_follow is written, the counts are the sums over trips."""
    n = 1024 * 256 + 300
    cfg = G.Config(5, flags=G.PRE_VOTE, seed=4)
    eng = rg.Engine(300, 3)
    E = rg.engine
    eng.follow_enable(n)
    eng.follow_gate_enable(cfg.election_tick, cfg.min_timeout, cfg.max_timeout, cfg.flags, cfg.seed)
    eng.follow_elect_enable()
    S = eng.follow_stride()
    groups = [5, 64, 1024 * 256 - 1, 1024 * 256, 1024 * 256 + 63, 1025 * 256, n - 1]
    recs = [(g, G.Msg((G.VOTE, G.PREVOTE)[k % 2], 3 + k, 11, index=k % 3, log_term=k % 2, priority=-(k % 2))) for k, g in enumerate(groups)]
    want = {g: V.step_follower(G.Node(cfg, g), m) for g, m in recs}
    assert {a[1] for a in want.values()} == {G.G_VOTE_GRANT, G.G_VOTE_REJECT}
    got, counts, places = dense_vote(eng, E, S, n, recs, cap=4, other={1024 * 256 + 1: G.APPEND})
    assert got == {g: a[:6] for g, a in want.items()}
    check_counts(got, counts, places, 4)
    soft = eng.follow_soft_read(np.array(groups, dtype=np.uint64))
    assert [int(r["term"]) for r in soft] == [m.term if m.kind == G.VOTE else 0 for _, m in recs]
    eng.sync()
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. - 6. led groups
# ---------------------------------------------------------------------------------------------------------------------
def vote_rig(rg, cq, ix64=False, clock=True, election_tick=5, reads=0, **kw):
    """life_cycle_rig.promoted_rig with ONE Config on both sides: the arena's gate and the leader's clock share CHECK_QUORUM.
    reads: the depth of the ReadIndex layer, enabled behind the promotion (0: the layer stays off)."""
    cfg = G.Config(election_tick, flags=G.PRE_VOTE | (G.CHECK_QUORUM if cq else 0), seed=9)
    rig = Rig(rg, 3, ix64=ix64, elect=False, **kw)
    rig.eng.follow_gate_enable(cfg.election_tick, cfg.min_timeout, cfg.max_timeout, cfg.flags, cfg.seed)
    rig.eng.follow_elect_enable()
    cases = H.gpu_cases(3)
    st = R.state_with(rig.G, 3, rig.eng.stride, cases)
    if kw.get("max_inflight"):  # the promotion is the host's there: the leader columns are loaded as a promotion leaves them
        rig.load_lead(R.model_state(st, cases)[0])
        rig.load_arena(cases)
    else:
        rig.load_lead(st)
        rig.load_arena(cases)
        rig.promote(cases, True, R.model_state(st, cases)[1], vouch=True)
    if reads:
        rig.eng.read_index_enable(reads)
    if clock:
        rig.eng.lead_clock_enable(cfg.election_tick, 1, (L.CHECK_QUORUM if cq else 0) | L.START_LED)
    return rig, cfg, [c for c in cases if c.expect == H.DONE]


def clock_cells(rig, groups):
    return [(int(r["term"]), int(r["election_elapsed"]), int(r["heartbeat_elapsed"]), int(r["led"])) for r in rig.eng.lead_clock_read(np.array(groups, dtype=np.uint64))]


def set_elapsed(rig, pairs, el):
    cells = np.zeros(len(pairs), dtype=rig.E.LEAD_CLOCK_CELL_DTYPE)
    cells["group"], cells["term"], cells["election_elapsed"], cells["led"] = [Lg for Lg, _ in pairs], [t for _, t in pairs], el, 1
    rig.eng.lead_clock_write(cells)


def snapshot(rig):
    return rig.arena(), rig.read_lead(), clock_cells(rig, range(rig.G))


def same_snapshot(a, b):
    return a[0] == b[0] and not R.diff(a[1], b[1], R.ALL_COLS + ("out",)) and a[2] == b[2]


def model_round(rig, cfg, snap, recs, lead_map):
    """The model over one call: -> ({g: answer}, the arena, the leader state and the clock cells it expects)"""
    arena, lead_state, cells = snap
    want_arena, want_lead, want_cells, answers = list(arena), R.copy_state(lead_state), list(cells), {}
    for g, m in recs:
        canon, soft, ecells = arena[g]
        node = G.Node(cfg, g, H.log_of(canon))
        node.load(*soft)
        node.self_id = ecells[0]
        Lg = lead_map.get(g)
        lead = clock = None
        if Lg is not None and Lg < rig.G:
            lead = R.get_lead(lead_state, Lg)
            tag, el, hb, led = cells[Lg]
            clock = L.new_group(3, lead["cfg"], cur_term=lead["cur_term"], led=bool(led), tag=tag)
            clock["el"], clock["hb"] = el, hb
        if Lg is not None and Lg >= rig.G:
            a, deposed = V.FAULT_ANSWER, False
        else:
            a, deposed = V.step(cfg, cfg.election_tick, node, lead, clock, None, m)
        answers[g] = a
        want_arena[g] = (node.log.canonical(), node.soft(), ecells)
        if deposed:
            want_lead["cfg"][Lg] = lead["cfg"]
            want_cells[Lg] = (clock["tag"], clock["el"], clock["hb"], int(clock["led"]))
    return answers, want_arena, want_lead, want_cells


def check_round(rig, cfg, snap, recs, lead_map, cap=None, also=None):
    """From the checkpoint `snap` was taken at: the dense call, then the sparse form, both against the model -- answers, arena
    layers, leader columns, clock cells, and whatever also(what) asserts after each. Leaves the engine restored.
    -> the model's answers"""
    want, want_arena, want_lead, want_cells = model_round(rig, cfg, snap, recs, lead_map)
    got, counts, places = dense_vote(rig.eng, rig.E, rig.stride, rig.n, recs, lead=lead_map, cap=cap)
    assert got == {g: a[:6] for g, a in want.items()}, [(g, m.key(), got[g], want[g]) for g, m in recs if got[g] != want[g][:6]][:3]
    check_counts(got, counts, places, cap or 0)

    def same(what):
        arena, lead_state, cells = snapshot(rig)
        assert arena == want_arena, (what, [(g, arena[g], want_arena[g]) for g in range(rig.n) if arena[g] != want_arena[g]][:2])
        assert not R.diff(want_lead, lead_state, R.ALL_COLS + ("out",)), (what, R.diff(want_lead, lead_state, R.ALL_COLS + ("out",)))
        assert cells == want_cells, (what, [(i, cells[i], want_cells[i]) for i in range(rig.G) if cells[i] != want_cells[i]][:3])
        if also:
            also(what)
    same("dense")
    rig.eng.restore()
    assert snapshot(rig)[0] == snap[0]
    sparse = [(g, m) for g, m in recs if lead_map.get(g, 0) < rig.G]  # (a lead group beyond n_groups is refused on the host)
    assert sparse_answers(rig.eng.follow_vote(vote_recs(rig.E, sparse, lead_map))) == [want[g] for g, _ in sparse]
    same("sparse")
    rig.eng.restore()
    return want


def table_rounds(done, cur, last):
    """Every row of the header's case table, one request per led group and round: [(name, {g: Msg})]"""
    def rnd(f):
        return {c.g: f(k, c, cur[c.L], last[c.L]) for k, c in enumerate(done)}
    kinds = (G.VOTE, G.PREVOTE)
    return [
        ("lower", rnd(lambda k, c, t, hi: G.Msg(kinds[k % 2], max(t - 1, 1), 11, index=hi + 1, log_term=t))),
        ("equal", rnd(lambda k, c, t, hi: G.Msg(kinds[k % 2], t, 11, index=hi + 1, log_term=t + 1, commit=hi, commit_term=t))),
        ("higher_ahead", rnd(lambda k, c, t, hi: G.Msg(kinds[k % 2], t + 1 + k % 3, 11, index=hi + 1, log_term=t + 1))),
        ("higher_ahead_forced", rnd(lambda k, c, t, hi: G.Msg(kinds[k % 2], t + 2, 12, index=hi + 1, log_term=t + 1, force=True))),
        ("higher_behind_forced", rnd(lambda k, c, t, hi: G.Msg(kinds[(k + 1) % 2], t + 1, 12, index=max(hi - 1, 0), log_term=t, commit=hi, commit_term=t, force=True))),
        ("higher_equal_priority", rnd(lambda k, c, t, hi: G.Msg(kinds[k % 2], t + 1, 13, index=hi, log_term=t, priority=(-1, 0, 0, -1, 1, -1)[k % 6], force=True))),
    ]


@pytest.mark.parametrize("cq", [False, True])
@pytest.mark.parametrize("ix64", [False, True])
def test_led_every_row_of_the_case_table_dense_equals_sparse_equals_the_model(rg, cq, ix64):
    """On the promoted rig, with and without CHECK_QUORUM, with the lead clock's election_elapsed written to 0 and to
    election_tick - 1: every row of the case table for six led groups (logs empty, behind a snapshot, one run, with a declared gap,
    near 2^63) beside a plain follower and a request whose dev_lead cell names no group. Dense = sparse = model in every answer, every
    arena layer, every leader column and every clock cell; the rows where nothing changes compare everything too."""
    rig, cfg, done = vote_rig(rg, cq, ix64)
    lead_state = rig.read_lead()
    cur = {c.L: int(lead_state["cur_term"][c.L]) for c in done}
    last = {c.L: int(lead_state["term_hi"][c.L]) for c in done}
    lead_map = {c.g: c.L for c in done}
    lead_map[60] = 5  # names a led group, but the arena holds no win state for it: the gated step
    seen = set()
    for el in (0, cfg.election_tick - 1):
        set_elapsed(rig, [(c.L, cur[c.L]) for c in done], el)
        rig.eng.checkpoint()
        snap = snapshot(rig)
        for name, reqs in table_rounds(done, cur, last):
            recs = sorted(reqs.items()) + [(50, G.Msg(G.VOTE, 3, 11, index=1, log_term=1)), (60, G.Msg(G.PREVOTE, 2, 12))]
            want = check_round(rig, cfg, snap, recs, lead_map, cap=3)
            for c in done:
                a = want[c.g]
                assert a[0] == F.NONE and a[2] & V.EV_LED, (name, c.name, a)
                seen.add((name.split("_")[0], a[1], bool(a[2] & V.EV_DEPOSED)))
                if name in ("lower", "equal") or (cq and name == "higher_ahead"):
                    assert not a[2] & V.EV_DEPOSED and a[3] == cur[c.L]
                    assert a[1] == (G.G_VOTE_REJECT if name == "equal" else G.G_IGNORED if cq and name == "higher_ahead" else a[1])
            assert not want[50][2] & V.EV_LED and not want[60][2] & V.EV_LED
    assert seen >= {("lower", G.G_IGNORED, False), ("lower", G.G_PREVOTE_LOW, False), ("equal", G.G_VOTE_REJECT, False), ("higher", G.G_VOTE_GRANT, True),
                    ("higher", G.G_VOTE_GRANT, False), ("higher", G.G_VOTE_REJECT, True), ("higher", G.G_VOTE_REJECT, False)}, seen
    assert (("higher", G.G_IGNORED, False) in seen) == cq
    rig.close()


def test_led_faults_are_answers_and_change_nothing(rg):
    """FAULT four ways in one call -- a dev_lead value beyond n_groups, soft.term != RG_COL_CUR_TERM[L], a clock cell the lead side
    has stopped under the current tag, a lead log rg_follow_demote refuses -- beside a HOST undo of a led VOTE (the lead log's commit
    index lies in the declared gap: commit_info cannot be answered) and a deposition that goes through: every cell of the refused
    groups stays, dense = sparse; the sparse form refuses its bad arguments on the host. The ReadIndex layer is on and every one of
    these lead groups, and a bystander, has a read pending: after the dense and after the sparse call the pending counts of the HOST
    and the FAULT groups are what they were and the deposed group's is 0, and a late ack round releases exactly the surviving reads."""
    rig, cfg, done = vote_rig(rg, False, reads=4)
    by = {c.name: c for c in done}
    stopped, mismatch, bad_log, gap, fine = by["one_run"], by["empty_dummy0"], by["empty_behind_snapshot"], by["eight_older_plus_tail"], by["gap_present"]
    E, eng = rig.E, rig.eng
    commit = eng.read_column(E.COL.COMMIT)
    hi = eng.read_column(E.COL.TERM_HI)
    kept, bystander = [c.L for c in (stopped, mismatch, bad_log, gap)], 5
    for Lg in kept + [fine.L]:  # commit_to_current_term: the empty entry of the own term is committed, so a read can be queued ...
        commit[Lg] = hi[Lg]
    eng.load_column(E.COL.COMMIT, commit)
    reads = [(Lg, 7000 + Lg) for Lg in kept + [fine.L, bystander]]
    assert [int(x) for x in eng.read_index(reads)] == [E.READ_QUEUED] * len(reads)
    # ... and only then the two logs go bad
    commit[bad_log.L] = int(eng.read_column(E.COL.TERM_HI)[bad_log.L]) + 5  # committed > last_index: no canonical state
    commit[gap.L] = 2                                                       # ... and one inside the dropped gap (1..3)
    eng.load_column(E.COL.COMMIT, commit)
    lead_state = rig.read_lead()
    assert int(lead_state["run_first"][0, gap.L]) == 4 and int(lead_state["dummy_index"][gap.L]) == 0
    cur = {c.L: int(lead_state["cur_term"][c.L]) for c in done}
    stop = np.zeros(1, dtype=E.LEAD_CLOCK_CELL_DTYPE)
    stop["group"], stop["term"] = stopped.L, cur[stopped.L]
    eng.lead_clock_write(stop)
    soft = rig.arena()[mismatch.g][1]
    from test_follow_gate_gpu import soft_array
    eng.follow_soft_write(soft_array(E, [mismatch.g], [(soft[0] + 1,) + soft[1:]]))
    eng.checkpoint()
    snap = snapshot(rig)
    lead_map = {c.g: c.L for c in done}
    lead_map[50] = rig.G
    recs = sorted((c.g, G.Msg(G.VOTE, cur[c.L] + 5, 12, index=0, log_term=0)) for c in (stopped, mismatch, bad_log, gap, fine)) + [(50, G.Msg(G.VOTE, 9, 12))]
    pending0 = eng.read_pending_counts()
    assert [int(pending0[Lg]) for Lg, _ in reads] == [1] * len(reads) and int(pending0.sum()) == len(reads)

    def queues(what):
        pending = eng.read_pending_counts()
        assert [int(pending[Lg]) for Lg in kept + [bystander]] == [1] * 5 and int(pending[fine.L]) == 0 and int(pending.sum()) == 5, (what, pending.nonzero())
    want = check_round(rig, cfg, snap, recs, lead_map, cap=8, also=queues)
    assert (eng.read_pending_counts() == pending0).all()  # (the checkpoint carries the queues)
    for c in (stopped, mismatch, bad_log):
        assert want[c.g] == V.FAULT_ANSWER
    assert want[50] == V.FAULT_ANSWER
    assert want[gap.g][:4] == (F.HOST, G.G_PASS, 0, cur[gap.L])
    assert want[fine.g][1] == G.G_VOTE_REJECT and want[fine.g][2] & V.EV_DEPOSED
    good = vote_recs(E, [(fine.g, G.Msg(G.VOTE, 99, 12))], lead_map)
    for field, value in (("follow_group", rig.n), ("lead_group", rig.G), ("kind", G.VOTE | G.PREVOTE), ("kind", G.APPEND), ("term", 0), ("from", 0), ("flags", 2)):
        bad = good.copy()
        bad[field][0] = value
        with pytest.raises(rg.EngineError) as ei:
            eng.follow_vote(bad)
        assert ei.value.code == E.ERR["INVALID_ARG"], field
    twice = vote_recs(E, [(fine.g, G.Msg(G.VOTE, 99, 12)), (51, G.Msg(G.VOTE, 99, 12))], {fine.g: fine.L, 51: fine.L})
    with pytest.raises(rg.EngineError):
        eng.follow_vote(twice)
    assert same_snapshot(snapshot(rig), snap) and (eng.read_pending_counts() == pending0).all()
    # ---- once more, and a late heartbeat round of the same term: the reads of the HOST and FAULT groups are still answered ----
    dense_vote(eng, E, rig.stride, rig.n, recs, lead=lead_map)
    queues("again")
    ctx = np.zeros((3, eng.stride), np.uint64)
    for Lg, c in reads:
        ctx[0, Lg] = ctx[2, Lg] = c  # (the own slot is 1)
    d_ctx = dev(ctx)
    eng.read_acks_device(d_ctx.data_ptr())
    eng.sync()
    assert sorted(int(s["group"]) for s in eng.read_states()) == sorted(kept + [bystander])
    assert not eng.read_pending_counts().any()
    rig.close()


def test_a_forced_vote_deposes_a_leader_in_transfer_and_the_unforced_one_is_ignored(rg):
    """CHECK_QUORUM, a transferee set: the MsgRequestVote of the transfer's target (RG_GATE_FORCE, Message.context ==
    CAMPAIGN_TRANSFER) deposes and reports TRANSFER_ABORTED, the TRANSFEREE bits are gone; the same request without FORCE is IGNORED
    and everything stays."""
    rig, cfg, done = vote_rig(rg, True)
    E, eng = rig.E, rig.eng
    cfgw = eng.read_column(E.COL.CFG)
    for c in done[:3]:
        cfgw[c.L] |= 2 << 20  # slot 1 is the transferee
    eng.load_column(E.COL.CFG, cfgw)
    lead_state = rig.read_lead()
    eng.checkpoint()
    snap = snapshot(rig)
    lead_map = {c.g: c.L for c in done}
    for force in (False, True):
        recs = sorted((c.g, G.Msg(G.VOTE, int(lead_state["cur_term"][c.L]) + 1, 12, index=int(lead_state["term_hi"][c.L]), log_term=int(lead_state["cur_term"][c.L]), force=force))
                      for c in done)
        want = check_round(rig, cfg, snap, recs, lead_map)
        for k, c in enumerate(done):
            a = want[c.g]
            if not force:
                assert (a[1], a[2]) == (G.G_IGNORED, V.EV_LED)
            else:
                assert a[1] == G.G_VOTE_GRANT and a[2] == G.EV_HARD_STATE | G.EV_LEADER_CHANGED | V.EV_LED | V.EV_DEPOSED | (V.EV_TRANSFER_ABORTED if k < 3 else 0), (c.name, a)
    rig.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. inside the loop
# ---------------------------------------------------------------------------------------------------------------------
def test_deposition_by_vote_inside_the_loop_and_the_next_leadership(rg):
    """Quiet leaders of term 2 with the ReadIndex layer and the clock; four followed groups hold the win state of four of them and
    each has a read pending. rgv_follow_vote_device, rgt_lead_gate_device, rg_tick_device with ONE synchronisation at the end: the
    vote of term 5 deposes the four, the gate reports NOT_LED for them and zeroes their rows, the tick leaves their columns alone,
    their pending reads are gone while the bystander's is released by a late ack. Then the life goes on: the groups tick as
    followers, campaign at term 6, win both rounds and are promoted on the device."""
    import torch
    cfg = G.Config(5, flags=G.PRE_VOTE, seed=9)
    rig = Rig(rg, 3, elect=False)
    E, eng, S = rig.E, rig.eng, rig.stride
    eng.follow_gate_enable(cfg.election_tick, cfg.min_timeout, cfg.max_timeout, cfg.flags, cfg.seed)
    eng.follow_elect_enable()
    st = R.base_state(rig.G, 3, eng.stride)
    rig.load_lead(st)
    pairs = [(0, 299), (63, 64), (64, 63), (256, 0)]
    cases = [H.Case("loop%d" % g, g, Lg, H.Follower(H.demote(R.get_lead(st, Lg))[1], 2, 2, (0, 1, 2), (), 0), R.get_lead(st, Lg)) for g, Lg in pairs]
    rig.load_arena(cases)
    eng.read_index_enable(4)
    eng.lead_clock_enable(10, 3, L.START_LED)
    leads = [Lg for _, Lg in pairs]
    reqs = [(Lg, 1000 + Lg) for Lg in leads] + [(5, 1005)]
    assert [int(x) for x in eng.read_index(reqs)] == [E.READ_QUEUED] * len(reqs)
    snap = snapshot(rig)
    lead_map = dict(pairs)
    recs = [(g, G.Msg(G.VOTE, 5, 3, index=3, log_term=2)) for g, _ in pairs]
    want, want_arena, want_lead, want_cells = model_round(rig, cfg, snap, recs, lead_map)
    assert all(a[1] == G.G_VOTE_GRANT and a[2] & V.EV_DEPOSED for a in want.values())
    # ---- the device chain ----
    acks = rg.MsgBuffers(rig.G, 3, eng.stride)
    for Lg in leads + [5, 6]:
        for s in (1, 2):
            acks.m_flags[Lg, s], acks.m_index[s, Lg] = T.MF_VALID, 3
    keep = [dev(getattr(acks, k)) for k in ("m_index", "m_commit", "m_hint", "m_rs")]
    d_flags, d_terms = dev(acks.m_flags.reshape(-1).copy()), dev(np.full((3, eng.stride), 2, np.uint64))
    gate_ev = torch.full((eng.stride,), 0xEE, dtype=torch.uint8, device="cuda")
    new_term = torch.zeros(eng.stride, dtype=torch.int64, device="cuda")
    collect = dense_vote(eng, E, S, rig.n, recs, lead=lead_map, sync=False, wait=False)
    eng.lead_gate_device(d_flags, d_terms, gate_ev, new_term, sync=False)
    eng.tick_device(*[k.data_ptr() for k in keep], d_flags.data_ptr())
    got, _, _ = collect()
    assert got == {g: a[:6] for g, a in want.items()}
    ev, rows = gate_ev.cpu().numpy(), d_flags.cpu().numpy().reshape(rig.G, 8)
    assert all(int(ev[Lg]) == T.EV_NOT_LED and not rows[Lg].any() for Lg in leads) and int(ev[5]) == 0 and rows[5].any()
    after = snapshot(rig)
    assert after[0] == want_arena and after[2] == want_cells
    for Lg in leads:  # the tick left the deposed groups' columns alone; the bystanders advanced
        assert R.get_lead(after[1], Lg) == R.get_lead(snap[1], Lg), Lg
    pending = eng.read_pending_counts()
    assert [int(pending[Lg]) for Lg in leads] == [0] * 4 and int(pending[5]) == 1
    ctx = np.zeros((3, eng.stride), np.uint64)
    for Lg, c in reqs:
        ctx[1, Lg] = ctx[2, Lg] = c
    d_ctx = dev(ctx)
    eng.read_acks_device(d_ctx.data_ptr())
    eng.sync()
    assert sorted(int(s["group"]) for s in eng.read_states()) == [5]
    # ---- followers again, then candidates, then leaders of term 6 ----
    nodes = {}
    for g, _ in pairs:
        canon, soft, cells = after[0][g]
        nd = M.Node(cfg, g, H.log_of(canon), self_id=2, incoming=(0, 1, 2), self_slot=0)
        nd.load(*soft)
        assert (nd.term, nd.vote, nd.lead, nd.role) == (5, 3, 0, G.FOLLOWER)
        nodes[g] = nd
    hup = torch.full((S,), -1, dtype=torch.int64, device="cuda")
    waiting = {g for g, _ in pairs}
    for _ in range(cfg.max_timeout):
        k = eng.follow_clock(hup, S)
        due = set(int(x) for x in hup.cpu().numpy().view(np.uint64)[:k]) & waiting
        assert due == {g for g in waiting if nodes[g].tick()}
        if due:
            camp = np.zeros(len(due), dtype=E.FOLLOW_CAMPAIGN_REQ_DTYPE)
            camp["group"] = sorted(due)
            for g, q in zip(sorted(due), eng.follow_campaign(camp)):
                assert nodes[g].record(M.Rec(M.HUP))[0] == M.REQUESTS and (int(q["result"]), int(q["req_term"])) == (M.REQUESTS, 6), (g, q)
        waiting -= due
        if not waiting:
            break
    assert not waiting
    winners = [g for g, _ in pairs]

    def round_cols(kind):
        cols = {k: np.zeros(S, np.uint8) for k in ("kind", "slot", "reject")}
        cols.update({k: np.zeros(S, np.uint64) for k in ("term", "commit", "commit_term")})
        for g in winners:
            cols["kind"][g], cols["slot"][g], cols["term"][g] = kind, 1, 6
        return {k: dev(v) for k, v in cols.items()}
    o_pre, o_real, o_hand = elect_out(S), elect_out(S), rig.out_columns()
    lead_col = np.full(S, L.NO_LEAD, np.uint64)
    for g, Lg in pairs:
        lead_col[g] = Lg
    pre, real, d_lead = round_cols(M.PREVOTE), round_cols(M.VOTE), dev(lead_col)
    eng.follow_vote_resps_device(pre, o_pre)
    eng.follow_vote_resps_device(real, o_real)
    eng.follow_promote_device(o_real["result"], d_lead, o_hand)
    eng.sync()
    for g in winners:
        assert nodes[g].record(M.Rec(M.PREVOTE, term=6, frm=1))[0] == M.REQUESTS and nodes[g].record(M.Rec(M.VOTE, term=6, frm=1))[0] == M.WON
    status, term = o_hand["status"].cpu().numpy(), o_hand["term"].cpu().numpy().view(np.uint64)
    assert [(int(status[g]), int(term[g])) for g in winners] == [(H.DONE, 6)] * 4
    final = rig.read_lead()
    assert [int(final["cur_term"][Lg]) for Lg in leads] == [6] * 4 and [int(final["term_hi"][Lg]) for Lg in leads] == [4] * 4
    rig.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. state rules
# ---------------------------------------------------------------------------------------------------------------------
def test_mirror_engine_device_inflights_and_state_rules(rg):
    """On an engine with a host mirror the dense form with a dev_lead column answers RG_ERR_STATE, without one it runs, and the
    sparse form deposes; an engine with device Inflights runs the dense road; before rg_follow_elect_enable, and where the clock's
    CHECK_QUORUM differs from the arena gate's, both forms answer RG_ERR_STATE."""
    rig, cfg, done = vote_rig(rg, False)
    E, eng = rig.E, rig.eng
    lead_state = rig.read_lead()
    eng.set_peers(200, [1, 2, 3], 2)
    lead_map = {c.g: c.L for c in done}
    recs = sorted((c.g, G.Msg(G.VOTE, int(lead_state["cur_term"][c.L]) + 3, 12, index=int(lead_state["term_hi"][c.L]) + 1, log_term=int(lead_state["cur_term"][c.L]) + 1))
                  for c in done)
    with pytest.raises(rg.EngineError) as ei:
        dense_vote(eng, E, rig.stride, rig.n, recs, lead=lead_map)
    assert ei.value.code == E.ERR["STATE"] and "host mirror" in str(ei.value)
    snap = snapshot(rig)
    plain = [(50, G.Msg(G.PREVOTE, 7, 12, index=1, log_term=1))]
    got, counts, _ = dense_vote(eng, E, rig.stride, rig.n, plain)  # dev_lead NULL: allowed
    assert counts[0] == 1 and got[50][:2] == (F.NONE, G.G_VOTE_GRANT) and same_snapshot(snapshot(rig), snap)
    want, want_arena, want_lead, want_cells = model_round(rig, cfg, snap, recs, lead_map)
    assert sparse_answers(eng.follow_vote(vote_recs(E, recs, lead_map))) == [want[g] for g, _ in recs]
    assert all(a[2] & V.EV_DEPOSED for a in want.values()) and rig.arena() == want_arena and clock_cells(rig, range(rig.G)) == want_cells
    rig.close()
    # ---- device Inflights ----
    rig, cfg, done = vote_rig(rg, True, max_inflight=4)
    lead_state = rig.read_lead()
    rig.eng.checkpoint()
    snap = snapshot(rig)
    lead_map = {c.g: c.L for c in done}
    recs = sorted((c.g, G.Msg(G.VOTE, int(lead_state["cur_term"][c.L]) + 1, 12, index=int(lead_state["term_hi"][c.L]) + 1, log_term=int(lead_state["cur_term"][c.L]) + 1, force=True))
                  for c in done)
    want = check_round(rig, cfg, snap, recs, lead_map)
    assert all(a[2] & V.EV_DEPOSED for a in want.values())
    rig.close()
    # ---- the state rules ----
    bare = Rig(rg, 3, elect=False)
    for call in (lambda: bare.eng.follow_vote(vote_recs(bare.E, plain)), lambda: dense_vote(bare.eng, bare.E, bare.stride, bare.n, plain)):
        with pytest.raises(rg.EngineError) as ei:
            call()
        assert ei.value.code == bare.E.ERR["STATE"] and "rg_follow_elect_enable first" in str(ei.value)
    bare.close()
    mixed, _, _ = promoted_rig(rg)  # the arena's gate without CHECK_QUORUM, the leader's clock with it
    for call in (lambda: mixed.eng.follow_vote(vote_recs(mixed.E, plain)), lambda: dense_vote(mixed.eng, mixed.E, mixed.stride, mixed.n, plain)):
        with pytest.raises(rg.EngineError) as ei:
            call()
        assert ei.value.code == mixed.E.ERR["STATE"] and "one Config" in str(ei.value)
    mixed.close()


def test_the_count_words_outlive_a_log_term_tick_of_an_engine_with_device_inflights(rg):
    """The count words stay what the vote call left until the next vote call (rgv_follow_vote_counts hands out their device address
    for that): the pre-pass of a dense log-term tick on an engine with device Inflights clears and copies its hint word, which lies
    in the same scratch block of the engine -- it must not be one of them."""
    from test_follow_gate_gpu import device_u64
    rig, cfg, done = vote_rig(rg, True, max_inflight=4)
    E, eng = rig.E, rig.eng
    plain = [(50, G.Msg(G.PREVOTE, 7, 12, index=1, log_term=1)), (60, G.Msg(G.PREVOTE, 7, 12, index=1, log_term=1))]
    got, counts, _ = dense_vote(eng, E, rig.stride, rig.n, plain)
    before = device_u64(eng.follow_vote_counts(), 6)
    assert before[0] == counts[0] == 2 and tuple(before[:5]) == tuple(counts)
    msgs = rg.MsgBuffers(rig.G, rig.P, eng.stride)  # an empty tick that carries a log-term column
    msgs.m_logterm = np.zeros((rig.P, eng.stride), dtype=np.uint64)
    eng.tick(msgs)
    assert device_u64(eng.follow_vote_counts(), 6) == before
    rig.close()
