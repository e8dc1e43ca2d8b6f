"""GPU: random SEQUENCES of entry points against the oracle -- dense ticks, sparse ticks (three-call and one-call),
the RawNode::step mirror with dense and sparse flushes, rg_recompute, checkpoint/restore -- checking the state
columns, RG_COL_OUT and the compact results after every step. Catches host-side bookkeeping slips (which result
words are stale, which caches are valid) that single-path tests cannot see."""
import os

import numpy as np
import pytest

import fuzz
import oracle_lib as O

pytestmark = pytest.mark.gpu
TERM = 5


def records(msgs, groups, P, rng):
    from raft_rs_amd.engine import WIRE_DTYPE
    recs = []
    for g in groups:
        for p in range(P):
            f = int(msgs["m_flags"][g, p])
            if f:
                recs.append((g, msgs["m_index"][p, g], msgs["m_commit"][p, g], msgs["m_hint"][p, g],
                             msgs["m_rs"][p, g], 0, p, f, 0))
    arr = np.array(recs, dtype=WIRE_DTYPE)
    rng.shuffle(arr)
    return arr


def mirror_steps(rg, eng, msgs, groups, P, self_slot, term=TERM):
    """Feed one tick's events of `groups` through the message-at-a-time mirror. term: Message.term of the responses (0: a
    local message, the mirror's term gate is skipped). RG_MF_BECOME_LEADER on the leader's slot -- alone there: the election
    goes in before anything else of its group -- is rg_local_become_leader at the term in m_hint."""
    MF = rg.MF
    for g in groups:
        g = int(g)
        if int(msgs["m_flags"][g, self_slot[g]]) == MF.BECOME_LEADER:
            eng.local_become_leader(g, int(msgs["m_hint"][self_slot[g], g]))
        for p in range(P):
            f = int(msgs["m_flags"][g, p])
            if not f:
                continue
            if p == self_slot[g]:
                if f == MF.BECOME_LEADER:
                    continue
                if f & MF.APPEND:
                    eng.local_append(g, int(msgs["m_commit"][p, g]))
                if f & MF.VALID:
                    eng.local_persisted(g, int(msgs["m_index"][p, g]))
                continue
            if f & MF.SENT:
                eng.mark_sent(g, p + 1)
            if f & MF.HEARTBEAT:
                eng.step_heartbeat_response(g, p + 1, term, int(msgs["m_commit"][p, g]), bool(f & MF.INS_FULL))
            elif f & MF.VALID:
                eng.step(g, p + 1, term, int(msgs["m_index"][p, g]), commit=int(msgs["m_commit"][p, g]),
                         reject=bool(f & MF.REJECT), reject_hint=int(msgs["m_hint"][p, g]),
                         request_snapshot=int(msgs["m_rs"][p, g]) if f & MF.HAS_RS else 0, ins_full=bool(f & MF.INS_FULL))


def clean_for_mirror(msgs, P, self_slot):
    """The mirror has no way to express meaningless combinations the raw columns allow: keep what it can say."""
    f = msgs["m_flags"]
    G = f.shape[0]
    for p in range(P):
        col = f[:, p]
        is_self = self_slot == p
        col[is_self] &= 0x21  # VALID | APPEND on the leader's own slot
        hb = (col & 0x40) != 0
        col[hb & ~is_self] &= 0x40 | 0x10 | 0x08  # HEARTBEAT (+SENT, INS_FULL)
        rest = ~hb & ~is_self
        only_mod = rest & ((col & 0x01) == 0)
        col[only_mod] &= 0x10  # without VALID only SENT means anything
        f[:, p] = col
    # request_snapshot value 0 with HAS_RS cannot be expressed either
    for p in range(P):
        has = (f[:, p] & 0x04) != 0
        zero = msgs["m_rs"][p, :G] == 0
        f[has & zero, p] &= np.uint8(~0x04 & 0xff)


def local_messages(rg, eng, cl, rng, G, P, mirror_ok=True):
    """RawNode::report_unreachable / report_snapshot between two steps of a sequence, through one of the three forms
    (records, one byte per group, the mirror by peer id), to the engine and to the oracle alike."""
    E = rg.engine
    form = rng.choice(["records", "dense", "mirror"] if mirror_ok else ["records", "dense"])
    if form == "records":
        events = fuzz.random_progress_events(rng, G, P, int(rng.integers(1, 60)))
        eng.progress_events(events)
    elif form == "dense":
        kind = int(rng.integers(1, 4))
        slot1 = np.where(rng.random(G) < 0.1, rng.integers(1, P + 1, size=G), 0).astype(np.uint8)
        eng.progress_event_dense(kind, slot1)
        events = [(int(g), int(slot1[g]) - 1, kind) for g in np.nonzero(slot1)[0]]
    else:
        events = []
        for _ in range(int(rng.integers(1, 12))):
            g, s, kind = int(rng.integers(0, G)), int(rng.integers(0, P)), int(rng.integers(1, 4))
            if kind == E.EV_UNREACHABLE:
                eng.report_unreachable(g, s + 1)
            else:
                eng.report_snapshot(g, s + 1, kind == E.EV_SNAPSHOT_FAILURE)
            events.append((g, s, kind))
    for g, s, kind in events:
        if g >= G or s >= P:
            continue
        if kind == 1:
            cl.L.ro_handle_unreachable(cl.h, g, s + 1)
        else:
            cl.L.ro_handle_snapshot_status(cl.h, g, s + 1, kind == 3)
    return form


# (RG_SOAK_SEEDS=n adds n more seeded cases here as well, P = 1..8 by the seed: an ad hoc soak, see below)
@pytest.mark.parametrize("seed,P", [(1, 3), (2, 5), (3, 7)] + [(200 + i, 1 + i % 8) for i in range(int(os.environ.get("RG_SOAK_SEEDS", "0")))])
def test_random_api_sequences_match_the_oracle(rg, seed, P):
    rng = np.random.default_rng(4200 + seed)
    G = 1500
    st = O.alloc_state(G, P)
    st["cfg"][:] = fuzz.random_cfg(rng, G, P)
    fuzz.random_state(rng, st, small_values=True)
    self_slot = ((st["cfg"] >> 16) & 7).astype(np.int64)
    eng = rg.Engine(G, P)
    eng.load_state(st)
    for g in range(G):
        eng.set_peers(g, list(range(1, P + 1)), TERM)
    cl = O.Cluster(G)
    cl.load_soa(st, term=TERM)
    msgs = O.alloc_msgs(G, P)
    del msgs["m_logterm"]
    mb = rg.MsgBuffers(G, P, eng.stride)
    gout = np.zeros(G, dtype=np.uint32)
    ckpt = None
    ops_seen = set()
    for step in range(70):
        cl.store_soa(st)
        op = rng.choice(["dense", "sparse3", "sparse1", "mirror_sparse", "mirror_dense", "recompute", "checkpoint",
                         "restore"], p=[0.15, 0.17, 0.17, 0.17, 0.1, 0.08, 0.08, 0.08])
        if op == "restore" and ckpt is None:
            op = "checkpoint"
        ops_seen.add(op)
        touched = None
        if op == "checkpoint":
            eng.checkpoint()
            ckpt = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
            continue
        if op == "restore":
            eng.restore()
            st = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in ckpt.items()}
            cl = O.Cluster(G)
            cl.load_soa(st, term=TERM)
            got = eng.read_state()
            assert not fuzz.diff_states(st, got, G, P), (step, op)
            continue
        if rng.random() < 0.3:  # local messages between the steps: MsgUnreachable / MsgSnapStatus
            ops_seen.add("local:" + local_messages(rg, eng, cl, rng, G, P))
            cl.store_soa(st)  # (the tick's messages are generated for the state the events left)
        if op == "recompute":
            eng.recompute()
            for g in range(G):
                gout[g] = 1 if cl.maybe_commit(g) else 0
        else:
            fuzz.random_msgs(rng, st, msgs)
            if op in ("sparse3", "sparse1", "mirror_sparse"):
                touched = np.sort(rng.choice(G, size=int(rng.integers(1, G // 3)), replace=False))
                keep = np.zeros(G, dtype=bool)
                keep[touched] = True
                msgs["m_flags"][~keep] = 0
            if op.startswith("mirror"):
                clean_for_mirror(msgs, P, self_slot)
            if op == "dense":
                for k in ("m_index", "m_commit", "m_hint", "m_rs", "m_flags"):
                    getattr(mb, k)[...] = msgs[k]
                eng.tick(mb)
            elif op == "sparse3":
                assert eng.ingest(records(msgs, touched, P, rng)) == 0
                eng.tick_ingested()
            elif op == "sparse1":
                n, dup = eng.ingest_tick(records(msgs, touched, P, rng))
                assert dup == 0
            else:
                mirror_steps(rg, eng, msgs, touched if touched is not None else range(G), P, self_slot)
                eng.flush()
            gout[:] = 0
            cl.tick_soa(msgs, gout)
        got = eng.read_state()
        cl.store_soa(st)
        diffs = fuzz.diff_states(st, got, G, P)
        assert not diffs, (step, op, diffs[:5])
        assert (got["out"] == gout).all(), (step, op, np.nonzero(got["out"] != gout)[0][:5])
        commit, out = eng.results()
        assert (commit == st["commit"]).all() and (out == gout).all(), (step, op)
        if op in ("sparse3", "sparse1", "mirror_sparse", "mirror_dense"):
            with_events = np.nonzero(msgs["m_flags"].any(axis=1))[0]
            groups, c2, o2 = eng.ingested_results()
            order = np.argsort(groups)
            assert (groups[order] == with_events).all(), (step, op)
            assert (c2[order] == st["commit"][with_events]).all() and (o2[order] == gout[with_events]).all(), (step, op)
    assert len(ops_seen) >= 9 and any(o.startswith("local:") for o in ops_seen), ops_seen
    eng.close()


# RG_SOAK_SEEDS=n adds n more seeded cases (P, window depth and mailbox use derived from the seed): an ad hoc soak
_SEND_CASES = [(11, 3, 2, False), (12, 5, 4, False), (13, 5, 3, True)] + [
    (100 + i, 2 + i % 7, 1 + (i * 5) % 9, i % 2 == 0) for i in range(int(os.environ.get("RG_SOAK_SEEDS", "0")))]


@pytest.mark.parametrize("seed,P,cap,mailbox", _SEND_CASES)
def test_random_api_sequences_with_the_send_stage(rg, seed, P, cap, mailbox):
    """The same idea with the Inflights on the device: after every kind of tick the send stage (separately or inside
    rg_flush_send) must produce the oracle's send decisions, Progress columns and window contents."""
    import sendstage
    from test_sendstage_gpu import apply_snapshots
    rng = np.random.default_rng(4300 + seed)
    G = 1200
    st = O.add_term_table(O.alloc_state(G, P))
    st["cfg"][:] = fuzz.random_cfg(rng, G, P)
    fuzz.random_state(rng, st, small_values=True)
    fuzz.random_term_table(rng, st, TERM)
    sendstage.mark_pending_conf(rng, st)
    self_slot = ((st["cfg"] >> 16) & 7).astype(np.int64)
    eng = rg.Engine(G, P, max_inflight=cap)
    eng.load_state(st)
    for g in range(G):
        eng.set_peers(g, list(range(1, P + 1)), TERM)
    if mailbox:  # small rg_flush_send batches go through the resident workgroup; everything else makes it step aside
        eng.mailbox_start()
    cl = O.Cluster(G)
    cl.load_soa(st, term=TERM, max_inflight=cap)
    cl.set_own_inflights(True)
    msgs = O.alloc_msgs(G, P)
    msgs["m_logterm"][...] = 0
    mb = rg.MsgBuffers(G, P, eng.stride)
    gout = np.zeros(G, dtype=np.uint32)
    n_items = 0
    ops_seen = set()
    for step in range(70):
        cl.store_soa(st)
        op = rng.choice(["dense", "dense_send", "sparse3", "sparse1", "mirror_sparse", "mirror_flush_send", "mirror_dense",
                         "mirror_small_flush_send", "recompute"])
        ops_seen.add(op)
        max_entries, skip = int(rng.integers(0, 4)), bool(rng.integers(0, 2))
        staged = False
        touched = None
        if rng.random() < 0.3:  # local messages between the steps (a state change resets the device window)
            ops_seen.add("local:" + local_messages(rg, eng, cl, rng, G, P))
            cl.store_soa(st)
        if op == "recompute":
            eng.recompute()
            for g in range(G):
                gout[g] = 1 if cl.maybe_commit(g) else 0
        else:
            fuzz.random_msgs(rng, st, msgs, sent_p=0.0, heartbeat_p=0.2)
            sendstage.prepare_msgs(msgs)
            if op not in ("dense", "dense_send", "mirror_dense"):
                # (mirror_small_flush_send: few enough records for the ONE-launch flush with the stage inside, k_flush_small_send)
                hi = 40 if op == "mirror_small_flush_send" else G // 3
                touched = np.sort(rng.choice(G, size=int(rng.integers(1, hi)), replace=False))
                keep = np.zeros(G, dtype=bool)
                keep[touched] = True
                msgs["m_flags"][~keep] = 0
            if op.startswith("mirror"):
                clean_for_mirror(msgs, P, self_slot)
            if op in ("dense", "dense_send"):
                for k in ("m_index", "m_commit", "m_hint", "m_rs", "m_flags"):
                    getattr(mb, k)[...] = msgs[k]
                if op == "dense_send":  # the tick and its stage as ONE launch (rg_tick_send)
                    eng.tick_send(mb, max_entries, skip_bcast_commit=skip)
                    staged = True
                else:
                    eng.tick(mb)
            elif op == "sparse3":
                assert eng.ingest(records(msgs, touched, P, rng)) == 0
                eng.tick_ingested()
            elif op == "sparse1":
                assert eng.ingest_tick(records(msgs, touched, P, rng))[1] == 0
            else:
                mirror_steps(rg, eng, msgs, touched if touched is not None else range(G), P, self_slot)
                if op in ("mirror_flush_send", "mirror_small_flush_send") or (op == "mirror_dense" and rng.random() < 0.5):
                    eng.flush_send(max_entries, skip_bcast_commit=skip)
                    staged = True
                else:
                    eng.flush()
            gout[:] = 0
            cl.tick_soa(msgs, gout)
        if not staged:
            eng.send_appends(max_entries, skip_bcast_commit=skip)
        items = sendstage.compare_items(eng.send_items(), cl.send_stage_soa(gout, max_entries, skip_bcast_commit=skip))
        n_items += len(items)
        apply_snapshots(rg, eng, cl, st, items)
        got = eng.read_state()
        cl.store_soa(st)
        diffs = fuzz.diff_states(st, got, G, P)
        assert not diffs, (step, op, diffs[:5])
        meta, ring = eng.read_inflights()
        sendstage.compare_rings(cl, meta, ring, st, cap)
    assert n_items > 2000 and {"dense_send", "mirror_small_flush_send"} <= ops_seen, (n_items, ops_seen)
    assert any(o.startswith("local:") for o in ops_seen), ops_seen
    if mailbox:
        assert eng.mailbox_stats()[0] > 0, "no flush was served by the resident workgroup"
    eng.close()


def _to_device(torch, msgs, with_logterm):
    keys = ("m_index", "m_commit", "m_hint", "m_rs", "m_flags")
    cols = [torch.from_numpy(np.ascontiguousarray(msgs[k]).view(np.uint8 if k == "m_flags" else np.int64).copy()).cuda()
            for k in keys]
    if with_logterm:  # (a log-term column without log-term rejects: the tick takes the single-tick road inside a fused call)
        cols.append(torch.zeros_like(cols[0]))
    return cols


@pytest.mark.parametrize("seed,P", [(21, 3), (22, 5)])
def test_random_api_sequences_with_publication(rg, seed, P):
    """Random sequences of entry points on an engine that publishes its commit indices (RCCL at world size 1): dense ticks from
    host and device buffers, fused calls with and without log-term ticks, sparse ticks, mirror flushes, rg_recompute,
    rg_set_config, checkpoint / restore, rg_load_column(COMMIT) and rg_permute_groups, the state checked against the oracle
    after every call, and a publication after about a third of the calls. After every publication the replica equals the commit
    column -- except inside a loss window (include/raftgroups.h: rg_restore, a reloaded commit column, rg_permute_groups mark
    the slice lost): the replica may be inexact for at most 2 x ring_ticks publications after the loss, and the one after those
    at the latest is the loss's one full publication (the check point after the one that folds the lost slice)."""
    import torch
    from raft_rs_amd import engine as E
    COL = rg.COL
    rng = np.random.default_rng(4500 + seed)
    G, RING = 1500, 3
    st = O.alloc_state(G, P)
    st["cfg"][:] = fuzz.random_cfg(rng, G, P)
    fuzz.random_state(rng, st, small_values=True)
    self_slot = ((st["cfg"] >> 16) & 7).astype(np.int64)
    eng = rg.Engine(G, P)
    eng.load_state(st)
    for g in range(G):
        eng.set_peers(g, list(range(1, P + 1)), TERM)
    cl = O.Cluster(G)
    cl.load_soa(st, term=TERM)
    eng.comm_init(0, 1, unique_id=E.comm_unique_id(), ring_ticks=RING)
    msgs = O.alloc_msgs(G, P)
    del msgs["m_logterm"]
    mb = rg.MsgBuffers(G, P, eng.stride)
    gout = np.zeros(G, dtype=np.uint32)
    out_t = torch.zeros((8, G), dtype=torch.int32, device="cuda")
    ckpt, window = None, None  # window: [publications since the loss, this one included; full publications before it]
    ops_seen, windows_closed, exact_checks = set(), 0, 0
    LOSS = ("restore", "load_commit", "permute")

    def reload_oracle():
        nonlocal cl
        cl = O.Cluster(G)
        cl.load_soa(st, term=TERM)

    def publish():
        nonlocal window, windows_closed, exact_checks
        eng.publish_commit()
        fulls = eng.publish_stats()["full_publications"]
        exact = np.array_equal(eng.published_commit(0), eng.read_column(COL.COMMIT))
        if window is None:
            assert exact and fulls == full_base[0], (step, op, fulls, full_base)
            exact_checks += 1
            return
        window[0] += 1
        assert fulls <= window[1] + 1, (step, "more than one full publication for one loss", fulls, window)
        if fulls == window[1] + 1:
            assert exact and window[0] <= 2 * RING + 1, (step, window, exact)
            full_base[0] = fulls
            window, windows_closed = None, windows_closed + 1
        else:
            assert window[0] <= 2 * RING, (step, "the loss window did not close", window)

    full_base = [eng.publish_stats()["full_publications"]]
    assert full_base[0] == 1
    for step in range(90):
        cl.store_soa(st)
        op = rng.choice(["dense", "device", "fused", "fused_lt", "sparse3", "sparse1", "mirror_sparse", "mirror_dense", "recompute",
                         "set_config", "checkpoint", "restore", "load_commit", "permute"],
                        p=[0.1, 0.1, 0.08, 0.1, 0.08, 0.08, 0.08, 0.06, 0.06, 0.06, 0.05, 0.05, 0.05, 0.05])
        if op == "restore" and ckpt is None:
            op = "checkpoint"
        if op in LOSS and window is not None:
            op = "dense"  # (one loss at a time: each window is checked for its own full publication)
        ops_seen.add(op)
        if op == "checkpoint":
            eng.checkpoint()
            ckpt = ({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}, self_slot.copy())
        elif op == "restore":
            eng.restore()
            st = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in ckpt[0].items()}
            self_slot = ckpt[1].copy()
            reload_oracle()
        elif op == "load_commit":
            # a host reloads the commit column (here: some groups raised to their last index, the rest as they are)
            c = st["commit"].copy()
            up = rng.choice(G, size=40, replace=False)
            c[up] = np.maximum(c[up], np.minimum(st["term_hi"][up], c[up] + 3))
            eng.load_column(COL.COMMIT, c)
            st["commit"][:] = c
            reload_oracle()
        elif op == "permute":
            perm = rng.permutation(G).astype(np.uint64)
            eng.permute_groups(perm)
            p = perm.astype(np.int64)
            for k in ("match", "next", "pr_commit", "pend_snap", "pend_rs", "gid"):
                st[k][:, :G] = st[k][:, p]
            for k in ("pflags", "commit", "term_lo", "term_hi", "cfg"):
                st[k][:] = st[k][p]
            self_slot = self_slot[p]
            ckpt = None  # (rg_permute_groups drops the checkpoint: it images the old placement)
            reload_oracle()
        elif op == "set_config":
            for g in rng.choice(G, size=5, replace=False):
                w = int(fuzz.random_cfg(rng, 1, P)[0])
                eng.set_config(int(g), w)
                st["cfg"][g] = w
                self_slot[g] = (w >> 16) & 7
            reload_oracle()
        elif op == "recompute":
            eng.recompute()
            for g in range(G):
                gout[g] = 1 if cl.maybe_commit(g) else 0
        elif op in ("fused", "fused_lt"):
            T = int(rng.integers(1, 5))
            kinds = ["plain"] * T
            if op == "fused_lt":
                kinds[int(rng.integers(0, T))] = "lt"
            dev = []
            for t in range(T):
                cl.store_soa(st)
                fuzz.random_msgs(rng, st, msgs)
                gout[:] = 0
                cl.tick_soa(msgs, gout)
                dev.append(_to_device(torch, msgs, kinds[t] == "lt"))
            assert eng.tick_device_fused([[c.data_ptr() for c in d] for d in dev], out_t.data_ptr()) == T
            eng.sync()
        else:
            fuzz.random_msgs(rng, st, msgs)
            touched = None
            if op in ("sparse3", "sparse1", "mirror_sparse"):
                touched = np.sort(rng.choice(G, size=int(rng.integers(1, G // 3)), replace=False))
                keep = np.zeros(G, dtype=bool)
                keep[touched] = True
                msgs["m_flags"][~keep] = 0
            if op.startswith("mirror"):
                clean_for_mirror(msgs, P, self_slot)
            if op == "dense":
                for k in ("m_index", "m_commit", "m_hint", "m_rs", "m_flags"):
                    getattr(mb, k)[...] = msgs[k]
                eng.tick(mb)
            elif op == "device":
                d = _to_device(torch, msgs, False)
                eng.tick_device(*[c.data_ptr() for c in d])
                eng.sync()
            elif op == "sparse3":
                assert eng.ingest(records(msgs, touched, P, rng)) == 0
                eng.tick_ingested()
            elif op == "sparse1":
                assert eng.ingest_tick(records(msgs, touched, P, rng))[1] == 0
            else:
                mirror_steps(rg, eng, msgs, touched if touched is not None else range(G), P, self_slot)
                eng.flush()
            gout[:] = 0
            cl.tick_soa(msgs, gout)
        if op in LOSS:
            window = [0, full_base[0]]
        if op not in ("checkpoint",):
            got = eng.read_state()
            cl.store_soa(st)
            diffs = fuzz.diff_states(st, got, G, P)
            assert not diffs, (step, op, diffs[:5])
            if op not in LOSS + ("set_config",):
                assert (got["out"] == gout).all(), (step, op, np.nonzero(got["out"] != gout)[0][:5])
        if rng.random() < 1 / 3:
            publish()
    for _ in range(2 * RING + 1):  # (a window still open at the end must close as well)
        if window is None:
            break
        op = "final"
        publish()
    assert window is None
    assert windows_closed >= 2 and exact_checks >= 5, (windows_closed, exact_checks)
    assert {"fused_lt", "permute", "load_commit", "restore", "mirror_dense", "recompute"} <= ops_seen, ops_seen
    eng.close()


@pytest.mark.parametrize("seed,P", [(31, 3), (34, 5)])
def test_random_api_sequences_with_read_index(rg, seed, P):
    """ReadIndex behind every road that moves what it reads (RG_COL_COMMIT, RG_COL_TERM_LO, RG_COL_CUR_TERM, RG_COL_CFG): dense
    ticks from host and device buffers, fused calls with and without log-term ticks, sparse ticks, mirror flushes -- large,
    and small ones the resident mailbox workgroup serves --, rg_recompute, rg_set_config followed by the re-check,
    checkpoint / restore, rg_load_column(COMMIT) and rg_permute_groups, elections on every road that ticks. After EVERY call:
    a batch of read requests, then sparse or dense acks, straight behind the call on the engine's stream and before anything
    is read back; statuses, queues and (every few steps) the drained list against tests/readonly_model.py, whose commit,
    term_lo, term and cfg are the ORACLE's after that call -- never the engine's columns --, and then the state itself
    against the oracle."""
    import copy
    import torch
    import readonly_model as M
    from test_read_index_gpu import ReadChecker
    COL, MF = rg.COL, rg.MF
    rng = np.random.default_rng(4600 + seed)
    G, DEPTH, STEPS = 600, 2, 60
    st = O.add_term_table(O.alloc_state(G, P))
    st["cfg"][:] = fuzz.random_cfg(rng, G, P)
    fuzz.random_state(rng, st, small_values=True)
    fuzz.random_term_table(rng, st, TERM, max_runs=2)  # (room for the elections: no reject is handed back to the host)
    self_slot = ((st["cfg"] >> 16) & 7).astype(np.int64)
    eng = rg.Engine(G, P)
    eng.load_state(st)
    for g in range(G):
        eng.set_peers(g, list(range(1, P + 1)), TERM)
    eng.mailbox_start()
    eng.read_index_enable(DEPTH)
    cl = O.Cluster(G)
    cl.load_soa(st, term=TERM)
    msgs = O.alloc_msgs(G, P)
    del msgs["m_logterm"]
    mb = rg.MsgBuffers(G, P, eng.stride)
    gout = np.zeros(G, dtype=np.uint32)
    out_t = torch.zeros((8, G), dtype=torch.int32, device="cuda")
    rd = ReadChecker(eng, M.Shard(st["cfg"], DEPTH), rng, P, DEPTH, G)
    ckpt = None
    ops_seen, seen, drained, elected = set(), set(), 0, 0
    served_before_read = []  # steps whose flush the resident workgroup served (the read calls follow it at once)

    def reload_oracle():
        nonlocal cl
        cl = O.Cluster(G)
        cl.load_soa(st, term=TERM)

    def model_follows_the_oracle():
        for g, grp in enumerate(rd.model.groups):
            grp.cfg, grp.commit, grp.term_lo = int(st["cfg"][g]), int(st["commit"][g]), int(st["term_lo"][g])
            grp.set_term(int(st["cur_term"][g]))

    def reads(step):
        nonlocal seen
        seen |= set(rd.requests(rd.random_requests(150), lease=(step % 10 == 9)))
        if step % 3 != 2:
            rd.acks(rd.random_sparse_acks(250))
        else:
            rd.acks_dense(rd.random_dense_cols(0.5))
        rd.check_queues()

    def check_state(step, op, check_out):
        got = eng.read_state()
        cl.store_soa(st)
        diffs = fuzz.diff_states(st, got, G, P)
        assert not diffs, (step, op, diffs[:5])
        assert (eng.read_column(COL.CUR_TERM) == st["cur_term"]).all(), (step, op)
        if check_out:
            assert (got["out"] == gout).all(), (step, op, np.nonzero(got["out"] != gout)[0][:5])

    def one_tick(step, op, sub=0):
        """one tick of random messages through the road `op`; the oracle takes the same messages"""
        nonlocal elected
        term = TERM + 1 + 2 * step + sub  # (above every term a group can have: the elections are well-formed)
        fuzz.random_msgs(rng, st, msgs, elect_p=0.0 if op.startswith("mirror") else 0.04, elect_term=term)
        touched = None
        if op in ("sparse3", "sparse1", "mirror_sparse", "mirror_small"):
            hi = 30 if op == "mirror_small" else G // 3  # (mirror_small: <= 256 records, what the resident workgroup takes)
            touched = np.sort(rng.choice(G, size=int(rng.integers(1, hi)), replace=False))
            keep = np.zeros(G, dtype=bool)
            keep[touched] = True
            msgs["m_flags"][~keep] = 0
        if op.startswith("mirror"):
            clean_for_mirror(msgs, P, self_slot)
            for g in (touched if touched is not None else range(G)):
                if rng.random() < 0.08:  # rg_local_become_leader: the election alone on the leader's slot
                    msgs["m_flags"][g, self_slot[g]] = MF.BECOME_LEADER
                    msgs["m_hint"][self_slot[g], g] = term
        keep_alive = None
        if op == "dense":
            for k in ("m_index", "m_commit", "m_hint", "m_rs", "m_flags"):
                getattr(mb, k)[...] = msgs[k]
            eng.tick(mb)
        elif op == "device":
            keep_alive = _to_device(torch, msgs, False)
            torch.cuda.synchronize()
            eng.tick_device(*[c.data_ptr() for c in keep_alive])
        elif op == "sparse3":
            assert eng.ingest(records(msgs, touched, P, rng)) == 0
            eng.tick_ingested()
        elif op == "sparse1":
            assert eng.ingest_tick(records(msgs, touched, P, rng))[1] == 0
        else:
            mirror_steps(rg, eng, msgs, touched if touched is not None else range(G), P, self_slot, term=0)
            served = eng.mailbox_stats()[0]
            eng.flush()
            if eng.mailbox_stats()[0] > served:
                served_before_read.append(step)
        gout[:] = 0
        cl.tick_soa(msgs, gout)
        cl.store_soa(st)
        elected += int(((gout & 0x10) != 0).sum())
        return keep_alive

    for step in range(STEPS):
        cl.store_soa(st)
        op = rng.choice(["dense", "device", "fused", "fused_lt", "sparse3", "sparse1", "mirror_sparse", "mirror_small", "mirror_dense",
                         "recompute", "set_config", "checkpoint", "restore", "load_commit", "permute"],
                        p=[0.08, 0.08, 0.07, 0.07, 0.08, 0.08, 0.07, 0.12, 0.05, 0.05, 0.06, 0.05, 0.05, 0.05, 0.04])
        if op == "restore" and ckpt is None:
            op = "checkpoint"
        ops_seen.add(op)
        check_out, keep_alive = True, None
        if op == "checkpoint":
            eng.checkpoint()
            ckpt = ({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}, self_slot.copy(),
                    copy.deepcopy(rd.model.groups))
            check_out = False
        elif op == "restore":
            eng.restore()
            st = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in ckpt[0].items()}
            self_slot = ckpt[1].copy()
            rd.model.groups = copy.deepcopy(ckpt[2])  # (the queues of the checkpoint; the undrained list stays)
            reload_oracle()
            check_out = False
        elif op == "load_commit":
            c = st["commit"].copy()
            up = rng.choice(G, size=40, replace=False)
            c[up] = np.maximum(c[up], np.minimum(st["term_hi"][up], c[up] + 3))
            eng.load_column(COL.COMMIT, c)
            st["commit"][:] = c
            reload_oracle()
            check_out = False
        elif op == "permute":
            drained += rd.check_states()  # (the list's `group` fields name the old positions: drain first)
            perm = rng.permutation(G).astype(np.uint64)
            eng.permute_groups(perm)
            p = perm.astype(np.int64)
            for k in ("match", "next", "pr_commit", "pend_snap", "pend_rs", "gid", "run_first", "run_term"):
                st[k][:, :G] = st[k][:, p]
            for k in ("pflags", "commit", "term_lo", "term_hi", "cfg", "dummy_index", "dummy_term", "cur_term"):
                st[k][:] = st[k][p]
            self_slot = self_slot[p]
            rd.model.groups = [rd.model.groups[int(i)] for i in p]
            ckpt = None  # (rg_permute_groups drops the checkpoint: it images the old placement)
            reload_oracle()
            check_out = False
        elif op == "set_config":
            changed = [int(g) for g in rng.choice(G, size=8, replace=False)]
            for g in changed:
                w = int(fuzz.random_cfg(rng, 1, P)[0])
                if rng.random() < 0.5:  # the quorum shrinks to the leader alone: what the re-check is for
                    s = int(self_slot[g])
                    w = (1 << s) | (s << 16) | (int(st["cfg"][g]) & 0xff000000) | (1 << (24 + s))
                eng.set_config(g, w)
                st["cfg"][g] = w
                self_slot[g] = (w >> 16) & 7
            reload_oracle()
            model_follows_the_oracle()
            rd.acks([(g, 0, 0, M.ACK_LAST_SELF) for g in changed])  # post_conf_change
            check_out = False
        elif op == "recompute":
            eng.recompute()
            for g in range(G):
                gout[g] = 1 if cl.maybe_commit(g) else 0
            cl.store_soa(st)
        elif op in ("fused", "fused_lt"):
            T = int(rng.integers(1, 5))
            kinds = ["plain"] * T
            if op == "fused_lt":
                kinds[int(rng.integers(0, T))] = "lt"
            keep_alive = []
            for t in range(T):
                fuzz.random_msgs(rng, st, msgs, elect_p=0.02, elect_term=TERM + 1 + 2 * step)
                if t:  # (one election per group and call: the term of a second one would not be above the first's)
                    for s in range(P):
                        msgs["m_flags"][:, s] &= np.where(self_slot == s, 0xff & ~MF.BECOME_LEADER, 0xff).astype(np.uint8)
                gout[:] = 0
                cl.tick_soa(msgs, gout)
                cl.store_soa(st)
                elected += int(((gout & 0x10) != 0).sum())
                keep_alive.append(_to_device(torch, msgs, kinds[t] == "lt"))
            torch.cuda.synchronize()
            assert eng.tick_device_fused([[c.data_ptr() for c in d] for d in keep_alive], out_t.data_ptr()) == T
        elif op == "mirror_small":
            one_tick(step, op)  # (the first makes the engine's last tick a sparse one; the second is the mailbox's to serve)
            model_follows_the_oracle()
            reads(step)
            check_state(step, op, True)
            one_tick(step, op, sub=1)
        else:
            keep_alive = one_tick(step, op)
        model_follows_the_oracle()
        reads(step)
        check_state(step, op, check_out)
        del keep_alive
        if step % 4 == 3 or step == STEPS - 1:
            drained += rd.check_states()
    assert ops_seen == {"dense", "device", "fused", "fused_lt", "sparse3", "sparse1", "mirror_sparse", "mirror_small", "mirror_dense",
                        "recompute", "set_config", "checkpoint", "restore", "load_commit", "permute"}, ops_seen
    assert seen == {M.NOT_READY, M.READY, M.QUEUED, M.DUPLICATE, M.FULL}, seen
    assert drained > 300 and elected > 20, (drained, elected)
    served, launches = eng.mailbox_stats()
    assert len(served_before_read) >= 2 and served >= 2 and launches >= 2, (served_before_read, served, launches)
    eng.close()
