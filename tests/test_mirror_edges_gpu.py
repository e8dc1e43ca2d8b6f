"""GPU: the host mirror's term gate and its elections on every road a flush can take, against tests/mirror_model.py (the host
half, written from INTEGRATION.md section 2) and the oracle (the device half). Everything is an integer: every comparison is
exact. After each flush: read_state() (fuzz.diff_states), RG_COL_CUR_TERM, results(), ingested_results() -- the group set and
the values -- against model and oracle; then the model's gate is probed on the engine (mirror_model.probe_and_answer): a
response at the registered term is queued, one at term + 1 answers RG_ERR_HIGHER_TERM, one at term - 1 is dropped with RG_OK
and its group stays out of the next flush's result list."""
import numpy as np
import pytest

import fuzz
import mirror_model as M
import oracle_lib as O
import sendstage

pytestmark = pytest.mark.gpu

MSG_APPEND_RESPONSE, MSG_HEARTBEAT_RESPONSE = 4, 9  # eraftpb::MessageType


def code_of(fn, *a, **kw):
    try:
        fn(*a, **kw)
        return M.OK
    except RuntimeError as e:  # raft_rs_amd.EngineError
        return e.code


def full_compare(rg, eng, model, res, what):
    G, P = model.G, model.P
    st = model.state()
    got = eng.read_state()
    diffs = fuzz.diff_states(st, got, G, P)
    assert not diffs, (what, diffs[:5])
    assert np.array_equal(eng.read_column(rg.COL.CUR_TERM), st["cur_term"]), (what, "RG_COL_CUR_TERM")
    assert np.array_equal(got["out"], res.gout), (what, np.nonzero(got["out"] != res.gout)[0][:5])
    commit, out = eng.results()
    assert np.array_equal(commit, st["commit"]) and np.array_equal(out, res.gout), (what, "results()")
    groups, c2, o2 = eng.ingested_results()
    order = np.argsort(groups)
    assert np.array_equal(groups[order], res.dirty), (what, "the groups of ingested_results()", len(groups), len(res.dirty))
    d = res.dirty.astype(np.int64)
    assert np.array_equal(c2[order], st["commit"][d]) and np.array_equal(o2[order], res.gout[d]), (what, "ingested_results()")


def make_flush(rg, eng, model, send=None, seen=None):
    """flush(tag): the engine's flush (rg_flush_send with send = (max_entries, skip_bcast_commit)), the model's, the whole
    comparison. With device Inflights also the work items, and after the road's flush and the one behind it the windows."""
    seen = {} if seen is None else seen

    def flush(tag):
        served = eng.mailbox_stats()[0]
        if send:
            eng.flush_send(send[0], skip_bcast_commit=send[1])
        else:
            eng.flush()
        seen["served"] = eng.mailbox_stats()[0] - served
        res = model.flush()
        if send:
            from test_sendstage_gpu import apply_snapshots
            want = model.cl.send_stage_soa(res.gout, send[0], skip_bcast_commit=send[1])
            items = sendstage.compare_items(eng.send_items(), want)
            seen["items"] = seen.get("items", 0) + len(items)
            apply_snapshots(rg, eng, model.cl, model.state(), items)
        full_compare(rg, eng, model, res, tag)
        if send and not tag.startswith(("first", "warm", "sparse")):
            meta, ring = eng.read_inflights()
            sendstage.compare_rings(model.cl, meta, ring, model.state(), eng.max_inflight)
            seen.setdefault("rings", []).append((meta, ring))
        return res

    return flush


def plain_state(rg, G, P, terms, snapshot_cell=None):
    """Every peer in Replicate at match 5 of a log 1..10, the leader on slot 0, a cur_term per group."""
    st = O.add_term_table(O.alloc_state(G, P))
    st["cfg"][:] = rg.cfg_make((1 << P) - 1, self_slot=0)
    st["term_lo"][:], st["term_hi"][:], st["commit"][:] = 1, 10, 5
    st["match"][:, :G], st["next"][:, :G], st["pr_commit"][:, :G] = 5, 11, 5
    st["match"][0, :G] = 10
    st["pflags"][:, :P] = rg.PF.REPLICATE | rg.PF.RECENT_ACTIVE
    st["cur_term"][:] = terms
    if snapshot_cell:
        g, s = snapshot_cell
        st["pflags"][g, s] = O.SNAPSHOT | rg.PF.RECENT_ACTIVE
        st["pend_snap"][s, g], st["next"][s, g] = 20, 6
    return st


def encoded(rg, kind, from_, term, index=0, commit=0, reject=False, reject_hint=0):
    """One response as protobuf bytes, built by the project's own encoder (rg_encode_message)."""
    f = {"msg_type": kind, "from": from_, "to": 1, "term": term, "commit": commit}
    if kind == MSG_APPEND_RESPONSE:
        f.update(index=index, reject=int(reject), reject_hint=reject_hint)
    return rg.engine.encode_message(f)


# ---- A ------------------------------------------------------------------------------------------------
def test_gate_order_table(rg):
    """Peer lookup, term gate, own-id drop, slot busy -- in this order, for rg_step, rg_step_heartbeat_response and
    rg_step_bytes with both message kinds; senders: an unknown id, id 0, the leader's own id, a known peer; terms: above,
    equal, below, 0. A reject from the own id (its REJECT bit is RG_MF_BECOME_LEADER, its hint would be the new term) queues
    nothing: after the flush nothing of its group has moved and the group is in no result list."""
    G, P = 4, 3
    terms = [5, 6, 8, 11]
    st = plain_state(rg, G, P, terms)
    model = M.Mirror(st)
    eng = rg.Engine(G, P)
    eng.load_state(st)
    both = M.Both(model, eng)
    for g in range(G):
        both.ok("set_peers", g, M.ids_of(model, g), terms[g])
    flush = make_flush(rg, eng, model)
    before = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in model.state().items()}

    def send(kind, g, from_, term, reject):
        """call kind `kind` on the engine, the same message on the model -> the code both gave"""
        hint = terms[g] + 50 if reject else 0
        if kind in ("step", "bytes_append"):
            want = model.step(g, from_, term, 7, commit=5, reject=reject, reject_hint=hint)
        else:
            want = model.step_heartbeat_response(g, from_, term, 5)
        if kind == "step":
            got = code_of(eng.step, g, from_, term, 7, commit=5, reject=reject, reject_hint=hint)
        elif kind == "heartbeat":
            got = code_of(eng.step_heartbeat_response, g, from_, term, 5)
        elif kind == "bytes_append":
            got = code_of(eng.step_bytes, g, encoded(rg, MSG_APPEND_RESPONSE, from_, term, 7, 5, reject, hint))
        else:
            got = code_of(eng.step_bytes, g, encoded(rg, MSG_HEARTBEAT_RESPONSE, from_, term, commit=5))
        assert got == want, (kind, g, from_, term, "engine", got, "model", want)
        return got

    kinds = ["step", "heartbeat", "bytes_append", "bytes_heartbeat"]  # (one group each: the queued cells do not meet)
    cells = 0
    for g, kind in enumerate(kinds):
        t, own = terms[g], M.peer_id(g, 0)
        for term in (t + 2, t, t - 1, 0):
            for from_ in (999, 0, M.peer_id((g + 1) % G, 1)):  # unknown, illegal, another group's peer
                assert send(kind, g, from_, term, False) == M.PEER_NOT_FOUND, (kind, from_, term)
            for reject in (False, True):
                assert send(kind, g, own, term, reject) == (M.HIGHER_TERM if term > t else M.OK), (kind, term, reject)
            cells += 5
    assert cells == 4 * 4 * 5
    assert not model.queue
    res = flush("own-id and unknown senders")  # nothing was queued: nothing moves, no group is listed
    assert len(res.dirty) == 0 and not res.gout.any()
    assert not fuzz.diff_states(before, eng.read_state(), G, P) and len(eng.ingested_results()[0]) == 0
    assert eng.read_column(rg.COL.CUR_TERM).tolist() == terms
    for g, kind in enumerate(kinds):
        t = terms[g]
        assert send(kind, g, M.peer_id(g, 1), t + 2, False) == M.HIGHER_TERM
        assert send(kind, g, M.peer_id(g, 1), t - 1, False) == M.OK   # dropped
        assert send(kind, g, M.peer_id(g, 1), t, False) == M.OK       # queued
        assert send(kind, g, M.peer_id(g, 2), 0, False) == M.OK       # term 0: no gate, queued
        assert send(kind, g, M.peer_id(g, 1), t - 1, False) == M.OK   # the gate comes before the busy rule
        assert send(kind, g, M.peer_id(g, 1), 0, False) == M.SLOT_BUSY
        assert send(kind, g, M.peer_id(g, 2), t, False) == M.SLOT_BUSY
        assert sorted(model.queue[g]) == [1, 2]
    res = flush("known peers")
    assert res.dirty.tolist() == [0, 1, 2, 3] and res.n_records == 8
    assert int(model.st["match"][1, 0]) == 7 and int(model.st["match"][2, 2]) == 7  # (the accepts were applied)
    eng.close()


# ---- B ------------------------------------------------------------------------------------------------
def test_busy_rules_leave_the_queue_as_it_was(rg):
    """Every busy rule, and after every refused call a flush gives exactly what the model's untouched queue gives."""
    G, P = 8, 5
    terms = [5, 6, 7, 8, 9, 10, 11, 12]
    st = plain_state(rg, G, P, terms, snapshot_cell=(7, 2))
    model = M.Mirror(st)
    eng = rg.Engine(G, P)
    eng.load_state(st)
    both = M.Both(model, eng)
    flush = make_flush(rg, eng, model)
    pid = M.peer_id
    # before rg_set_peers: RG_ERR_STATE everywhere, also for a registration the engine refuses (n > P)
    assert both.call("set_peers", 0, [pid(0, s) for s in range(P + 1)], 5) == M.INVALID_ARG
    for name, args in (("step", (0, pid(0, 1), 5, 7)), ("step_heartbeat_response", (0, pid(0, 1), 5)), ("local_append", (0, 11)),
                       ("local_persisted", (0, 10)), ("local_become_leader", (0, 9)), ("mark_sent", (0, pid(0, 1))),
                       ("report_unreachable", (0, pid(0, 1))), ("report_snapshot", (0, pid(0, 1), False))):
        assert both.call(name, *args) == M.STATE, name
    assert code_of(eng.flush) == M.STATE and model.flush() == M.STATE
    both.ok("set_peers", 0, [pid(0, 0), pid(0, 1), pid(0, 2)], terms[0])  # n < P: slots 3 and 4 have no id
    for g in range(1, G):
        both.ok("set_peers", g, M.ids_of(model, g), terms[g])
    for from_ in (pid(0, 3), pid(0, 4), 0):
        assert both.call("step", 0, from_, terms[0], 7) == M.PEER_NOT_FOUND
        assert both.call("mark_sent", 0, from_) == M.PEER_NOT_FOUND
        assert both.call("report_unreachable", 0, from_) == M.OK  # "no progress available": ignored
    both.ok("step", 0, pid(0, 2), terms[0], 8)
    assert flush("n < P").dirty.tolist() == [0]

    # a second event on a slot, in both orders; rg_mark_sent beside a queued response is allowed
    both.ok("step", 1, pid(1, 1), terms[1], 9, commit=5)
    assert both.call("step_heartbeat_response", 1, pid(1, 1), terms[1], 9) == M.SLOT_BUSY
    both.ok("mark_sent", 1, pid(1, 1))
    both.ok("step_heartbeat_response", 2, pid(2, 3), terms[2], 4)
    assert both.call("step", 2, pid(2, 3), terms[2], 10, commit=9) == M.SLOT_BUSY
    both.ok("mark_sent", 2, pid(2, 3))
    both.ok("mark_sent", 2, pid(2, 4))
    both.ok("step", 2, pid(2, 4), terms[2], 6)  # (and a response beside a queued mark)
    # rg_report_*: busy while the group has traffic queued, also for a slot that carries none
    assert both.call("report_unreachable", 1, pid(1, 2)) == M.SLOT_BUSY
    assert both.call("report_snapshot", 2, pid(2, 1), True) == M.SLOT_BUSY
    assert both.call("report_unreachable", 1, 424242) == M.OK  # (the peer lookup comes first)
    res = flush("second event on a slot")
    assert res.dirty.tolist() == [1, 2] and res.n_records == 3
    assert int(model.st["match"][1, 1]) == 9 and int(model.st["match"][3, 2]) == 5, "the FIRST event of each slot was applied"

    # rg_local_persisted twice: refused; rg_local_append twice: the newest last index counts
    both.ok("local_persisted", 3, 10)
    assert both.call("local_persisted", 3, 9) == M.SLOT_BUSY
    both.ok("local_append", 4, 12)
    both.ok("local_append", 4, 14)
    both.ok("local_persisted", 4, 13)
    assert both.call("local_persisted", 4, 14) == M.SLOT_BUSY
    res = flush("local events twice")
    assert res.dirty.tolist() == [3, 4] and int(model.st["term_hi"][4]) == 14 and int(model.st["match"][0, 4]) == 13

    # rg_local_become_leader: not at or below the registered term; not with anything of the group queued -- a response,
    # a sent mark, a proposal, another election
    for g, queued in ((3, ("step", (3, pid(3, 1), terms[3], 8))), (4, ("mark_sent", (4, pid(4, 2)))), (5, ("local_append", (5, 11))),
                      (6, ("local_become_leader", (6, terms[6] + 1)))):
        assert both.call("local_become_leader", g, terms[g]) == M.INVALID_ARG
        assert both.call("local_become_leader", g, terms[g] - 1) == M.INVALID_ARG
        both.ok(queued[0], *queued[1])
        assert both.call("local_become_leader", g, terms[g] + 3) == M.SLOT_BUSY, g
    assert both.call("local_become_leader", 6, terms[6] + 1) == M.INVALID_ARG  # (the gate moved when the election was queued)
    assert model.terms[6] == terms[6] + 1 and model.terms[3] == terms[3]
    both.ok("step", 6, pid(6, 1), terms[6] + 1, 11)  # a response of the new term behind the election
    assert both.call("step", 6, pid(6, 2), terms[6] + 2, 11) == M.HIGHER_TERM
    res = flush("elections against queued events")
    assert res.dirty.tolist() == [3, 4, 5, 6] and res.accepted == [6] and not res.refused
    assert model.cur_term(6) == terms[6] + 1 and [model.cur_term(g) for g in (3, 4, 5)] == [terms[g] for g in (3, 4, 5)]

    # rg_report_* on clean groups: applied (ro_handle_unreachable / ro_handle_snapshot_status)
    both.ok("report_unreachable", 1, pid(1, 3))
    both.ok("report_snapshot", 7, pid(7, 2), False)
    both.ok("report_snapshot", 7, pid(7, 1), True)  # not in Snapshot: ignored
    st_now = model.state()
    assert int(st_now["pflags"][1, 3]) & 3 == O.PROBE and int(st_now["pflags"][7, 2]) & 3 == O.PROBE
    assert int(st_now["pend_snap"][2, 7]) == 0
    diffs = fuzz.diff_states(st_now, eng.read_state(), G, P)
    assert not diffs, diffs[:5]
    res = flush("nothing queued")
    assert len(res.dirty) == 0
    assert both.codes["step", M.SLOT_BUSY] >= 1 and both.codes["step_heartbeat_response", M.SLOT_BUSY] >= 1
    eng.close()


# ---- C ------------------------------------------------------------------------------------------------
def mailbox_first(rg, eng, both, flush, seen, host_inflights=True):
    """The resident workgroup takes a small flush only behind a SPARSE one (the result words of a dense tick need a
    memset on the stream): start it, then one sparse flush of ordinary traffic."""
    def before(rng):
        eng.mailbox_start()
        for g in rng.choice(both.model.G, size=20, replace=False):
            M.ordinary(both, rng, int(g), False, host_inflights)
        flush("sparse flush before the mailbox's")
        seen["rings"] = []
    return before


@pytest.mark.parametrize("road", list(M.ROADS))
def test_elections_on_every_road(rg, road):
    """Accepted and refused elections in the same flush on each road a flush can take -- the one-launch flush (<= 256 =
    RG_INGEST_BLOCK records), the list flush out of pinned memory (<= 1024 = RG_ZEROCOPY_MAX groups) and copied (above, up to
    16384 = RG_ROUNDTRIP_MAX records), the three-call sequence (above that), the dense tick (half of G or more groups dirty:
    rg_flush_impl) and the resident mailbox workgroup. Groups of four kinds: (a) an election the device accepts, (b) one it
    refuses (above the registered term, not above RG_COL_CUR_TERM), (c) an election with proposals, the persisted index and the
    peers' responses of the new term behind it, accepted and refused, (d) ordinary traffic. The counts come from the oracle's
    result words (mirror_model.check_caps / check_road_shape). Then the gate probe and the second flush: the refused groups'
    peers answer at the old term, the accepted groups' at the new one, and all of it is applied."""
    assert list(M.ROADS) == ["one_launch", "pinned_list", "copied_list", "three_call", "dense", "mailbox"]
    G, P = M.ROADS[road][:2]
    st = M.make_state(77, G, P)
    model = M.Mirror(st)
    eng = rg.Engine(G, P)
    eng.load_state(st)
    both = M.Both(model, eng)
    seen = {}
    flush = make_flush(rg, eng, model, seen=seen)
    served = []

    def flush_road(tag):
        res = flush(tag)
        if tag == road:
            served.append(seen["served"])
        return res

    before = mailbox_first(rg, eng, both, flush, seen) if road == "mailbox" else None
    kinds, res, res2 = M.drive_road(both, road, flush_road, seed=100 + len(road), before_road=before)
    assert served == [1 if road == "mailbox" else 0], "the resident workgroup serves the mailbox road's flush and no other"
    assert both.codes["step", M.HIGHER_TERM] >= 48 and both.codes["step", M.SLOT_BUSY] >= 32
    eng.close()


# ---- D ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("road", ["one_launch", "pinned_list", "dense", "mailbox"])
def test_elections_on_every_road_with_device_inflights(rg, road):
    """The same with the Inflights on the device (max_inflight = 3) and the send stage riding along (rg_flush_send): inside
    the one launch, behind the list tick, as k_tick_send on the dense road, inside the mailbox request. Work items, Progress
    columns and windows against the oracle; an accepted election empties the windows, a refused one leaves them
    bit-identical."""
    G, P = M.ROADS[road][:2]
    cap, max_entries = 3, 1
    st = M.make_state(77, G, P)
    model = M.Mirror(st, max_inflight=cap)
    eng = rg.Engine(G, P, max_inflight=cap)
    eng.load_state(st)
    both = M.Both(model, eng)
    seen = {}
    flush = make_flush(rg, eng, model, send=(max_entries, False), seen=seen)
    served, rings0 = [], []

    def flush_road(tag):
        res = flush(tag)
        if tag == road:
            served.append(seen["served"])
        return res

    first = mailbox_first(rg, eng, both, flush, seen, host_inflights=False) if road == "mailbox" else None

    def before(rng):
        if first:
            first(rng)
        seen["rings"] = []
        rings0.append(eng.read_inflights())

    kinds, res, res2 = M.drive_road(both, road, flush_road, seed=100 + len(road), host_inflights=False, before_road=before)
    assert served == [1 if road == "mailbox" else 0]
    assert seen["items"] > G, "the send stage had work"
    (meta0, ring0), (meta1, ring1) = rings0[0], seen["rings"][0]
    count0, count1 = meta0 >> 16, meta1 >> 16
    # (a): the election is alone in its group -- every peer is in Probe afterwards, which keeps no window
    elected, alone = np.array(kinds["a"]), np.array(kinds["b"])
    assert count0[:, elected].sum() >= 8 and count0[:, alone].sum() >= 8, "windows with something in them before the flush"
    assert not count1[:P, elected].any(), "Raft::reset: every window of a group that became leader is empty"
    # (b): the refused election is alone in its group -- nothing of the group's windows may move
    assert np.array_equal(meta0[:, alone], meta1[:, alone]) and np.array_equal(ring0[alone], ring1[alone])
    eng.close()


# ---- E ------------------------------------------------------------------------------------------------
def test_permutation_moves_ids_and_gates_together(rg):
    """rg_permute_groups: position i answers to old group perm[i]'s peer ids AND its term, and an election at position i
    is judged against perm[i]'s RG_COL_CUR_TERM. Refused (RG_ERR_SLOT_BUSY) while an election is queued, which still settles."""
    G, P = 3000, 5
    rng = np.random.default_rng(9)
    st = M.make_state(78, G, P)
    model = M.Mirror(st)
    eng = rg.Engine(G, P)
    eng.load_state(st)
    both = M.Both(model, eng)
    flush = make_flush(rg, eng, model)
    M.register_all(both)
    M.first_round(both)
    assert len(flush("first round").accepted) == G
    order = rng.permutation(G)
    perm = np.empty(G, dtype=np.uint64)
    perm[order] = np.roll(order, -1)  # ONE cycle of length G: no fixed point, no pair swapped (perm is not its own inverse)
    assert (perm != np.arange(G)).all() and (perm[perm.astype(np.int64)] != np.arange(G)).all()
    # queued elections -- one the device will accept, one it will refuse -- bar the permutation, and settle afterwards
    x, y = int(order[0]), int(order[1])
    both.ok("set_peers", y, M.ids_of(model, y), model.cur_term(y) - 2)
    both.ok("local_become_leader", x, model.cur_term(x) + 1)
    both.ok("local_become_leader", y, model.cur_term(y))
    assert model.permute(perm) == M.SLOT_BUSY and code_of(eng.permute_groups, perm) == M.SLOT_BUSY
    res = flush("elections behind a refused permutation")
    assert res.accepted == [x] and res.refused == [y]
    M.probe_and_answer(both, rng, {"touched": [x, y], "registered": {x: model.cur_term(x) - 1, y: model.cur_term(y) - 2}}, res)
    flush("answers")
    old_terms, old_cur = list(model.terms), [model.cur_term(g) for g in range(G)]
    assert len(set(old_terms)) >= 7
    assert model.permute(perm) == M.OK
    eng.permute_groups(perm)
    assert not fuzz.diff_states(model.state(), eng.read_state(), G, P)
    assert np.array_equal(eng.read_column(rg.COL.CUR_TERM), model.st["cur_term"])
    moved = 0
    for i in range(G):
        o = int(perm[i])
        assert model.terms[i] == old_terms[o] and model.peers[i][:P] == M.ids_of(model, o) and model.cur_term(i) == old_cur[o]
        moved += old_terms[o] != old_terms[i]
        t, pid = model.terms[i], M.peer_id(o, (model.self_slot[i] + 1) % P)
        assert both.call("step", i, pid, t + 1, 3) == M.HIGHER_TERM
        assert both.call("step", i, pid, t - 1, 3) == M.OK  # dropped
        assert both.call("step", i, M.peer_id(i, 1), t, 3) == M.PEER_NOT_FOUND  # the ids this position had before
        if i % 3 == 0:
            both.ok("step", i, pid, t, model.last_index(i), commit=model.committed(i))
    assert moved > G // 2, "most positions took another term"
    res = flush("responses at the permuted gates")
    assert len(res.dirty) == G // 3
    # elections at the new positions, judged against the CUR_TERM that moved there
    sample = [int(g) for g in rng.choice(G, size=64, replace=False)]
    registered = {}
    for k, i in enumerate(sample):
        cur = model.cur_term(i)
        if k % 2:
            both.ok("set_peers", i, M.ids_of(model, int(perm[i])), cur - 2)
            both.ok("local_become_leader", i, cur)
        else:
            both.ok("local_become_leader", i, cur + 1)
        registered[i] = model.elections[-1][1]
    res = flush("elections after the permutation")
    assert sorted(res.accepted) == sorted(sample[0::2]) and sorted(res.refused) == sorted(sample[1::2])
    listed = M.probe_and_answer(both, rng, {"touched": sample, "registered": registered}, res)
    assert flush("answers after the permutation").dirty.tolist() == listed
    eng.close()


# ---- F ------------------------------------------------------------------------------------------------
def test_checkpoint_restore_leaves_the_gate_behind(rg):
    """rg_restore brings RG_COL_CUR_TERM back and NOT the host's gate (the mirror's tables are not in the image). What an
    un-re-registered group does with a response at the restored term: dropped, RG_OK, nothing queued. The documented
    recovery: rg_set_peers at the restored term, then the same election is accepted again."""
    G, P = 64, 3
    st = M.make_state(79, G, P)
    model = M.Mirror(st)
    eng = rg.Engine(G, P)
    eng.load_state(st)
    both = M.Both(model, eng)
    flush = make_flush(rg, eng, model)
    M.register_all(both)
    M.first_round(both)
    flush("first round")
    eng.checkpoint()
    image = model.snapshot()
    restored = [model.cur_term(g) for g in range(G)]
    assert model.terms == restored
    for g in range(G):
        both.ok("local_become_leader", g, restored[g] + 1)
    assert len(flush("elections after the checkpoint").accepted) == G
    eng.restore()
    model.restore(image)
    assert not fuzz.diff_states(model.state(), eng.read_state(), G, P)
    assert eng.read_column(rg.COL.CUR_TERM).tolist() == restored, "the device's term is the checkpoint's"
    assert model.terms == [t + 1 for t in restored], "the host's gate is not"
    for g in range(G):
        pid = M.peer_id(g, (model.self_slot[g] + 1) % P)
        assert both.call("step", g, pid, restored[g], model.last_index(g)) == M.OK  # below the gate: dropped
        assert both.call("step_heartbeat_response", g, pid, restored[g]) == M.OK
        assert both.call("local_become_leader", g, restored[g] + 1) == M.INVALID_ARG  # not above the gate the host kept
    assert not model.queue
    assert len(flush("dropped responses").dirty) == 0
    again = list(range(0, G, 2))
    for g in again:
        both.ok("set_peers", g, M.ids_of(model, g), restored[g])
        both.ok("local_become_leader", g, restored[g] + 1)
    res = flush("the same elections after re-registration")
    assert sorted(res.accepted) == again and not res.refused
    M.probe_and_answer(both, np.random.default_rng(1), {"touched": list(range(G)), "registered": dict(zip(again, [restored[g] for g in again]))}, res)
    flush("answers")
    eng.close()


# ---- G ------------------------------------------------------------------------------------------------
class BytesEngine:
    """An engine whose responses all arrive as protobuf bytes (rg_step_bytes), built by rg_encode_message."""

    def __init__(self, rg, eng):
        self._rg, self._eng = rg, eng

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def step(self, g, from_, term, index, commit=0, reject=False, reject_hint=0, request_snapshot=0, ins_full=False, log_term=0):
        f = {"msg_type": MSG_APPEND_RESPONSE, "from": from_, "to": 1, "term": term, "index": index, "commit": commit,
             "reject": int(reject), "reject_hint": reject_hint, "request_snapshot": request_snapshot, "log_term": log_term}
        self._eng.step_bytes(g, self._rg.engine.encode_message(f), ins_full=ins_full)

    def step_heartbeat_response(self, g, from_, term, commit=0, ins_full=False):
        f = {"msg_type": MSG_HEARTBEAT_RESPONSE, "from": from_, "to": 1, "term": term, "commit": commit}
        self._eng.step_bytes(g, self._rg.engine.encode_message(f), ins_full=ins_full)


def test_step_bytes_equals_step_through_the_gate(rg):
    """The one-launch road of test_elections_on_every_road with every response fed as encoded bytes: the same codes, and
    after every flush results and state identical to the rg_step form."""
    G, P = M.ROADS["one_launch"][:2]
    logs = []
    for as_bytes in (False, True):
        st = M.make_state(77, G, P)
        model = M.Mirror(st)
        eng = rg.Engine(G, P)
        eng.load_state(st)
        both = M.Both(model, BytesEngine(rg, eng) if as_bytes else eng)
        plain = make_flush(rg, eng, model)
        log = []

        def flush(tag):
            res = plain(tag)
            groups, commit, out = eng.ingested_results()
            order = np.argsort(groups)
            log.append((tag, groups[order], commit[order], out[order], eng.results(), eng.read_state()))
            return res

        M.drive_road(both, "one_launch", flush, seed=100 + len("one_launch"))
        logs.append((log, both.codes))
        eng.close()
    (a, codes_a), (b, codes_b) = logs
    assert codes_a == codes_b and len(a) == len(b) == 5
    for (tag, g1, c1, o1, r1, s1), (_, g2, c2, o2, r2, s2) in zip(a, b):
        assert np.array_equal(g1, g2) and np.array_equal(c1, c2) and np.array_equal(o1, o2), tag
        assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1]), tag
        assert not fuzz.diff_states(s1, s2, G, P, present_only=False) and np.array_equal(s1["out"], s2["out"]), tag
