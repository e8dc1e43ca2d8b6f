"""GPU: every launcher of the per-slot-count launcher table (RgTickLaunch, csrc/rg_tick_kernels.h) and every launch that goes
through rg_with_p, at EVERY slot count 1..8, against the oracle.

The host reaches the kernels instantiated for P slots through one table per P; the one thing that can go wrong there is a slot
count wired to another slot count's launcher. A kernel compiled for another P assumes another column stride per lane, so one
full workgroup plus a ragged one (G = 300) shows it: every case below compares everything with the oracle, exactly as the
suites of the single paths do (whose helpers it borrows), for 2-3 ticks.
"""
import numpy as np
import pytest

import fuzz
import oracle_lib as O
import sendstage
import test_api_sequences_gpu as A
import test_parity_gpu as PG
from test_sendstage_gpu import apply_snapshots, check as check_send_state

pytestmark = pytest.mark.gpu

G = 300
SLOTS = list(range(1, 9))
KEYS = ("m_index", "m_commit", "m_hint", "m_rs", "m_flags")


def full_cfg(rg, P):
    return rg.cfg_make((1 << P) - 1, 0, 0)


def dense_state(rg, rng, P, cfg=None, term=None, **cfg_kw):
    """A random state of G groups whose every block of 64 names all P slots (no block below P: the plain lane kernel runs)."""
    st = O.alloc_state(G, P)
    if term is not None:
        st = O.add_term_table(st)
    st["cfg"][:] = fuzz.random_cfg(rng, G, P, **cfg_kw) if cfg is None else cfg
    if cfg is None and not cfg_kw.get("group_commit_frac"):
        st["cfg"][::64] = full_cfg(rg, P)
    fuzz.random_state(rng, st, small_values=True, with_gids=bool(cfg_kw.get("group_commit_frac")))
    if term is not None:
        fuzz.random_term_table(rng, st, term)
    return st


def run_dense(rg, P, seed, label, kernel, streaming=None, offset_bits=None, cfg=None, cfg_kw=None, **engine_kw):
    rng = np.random.default_rng(seed + P)
    st = dense_state(rg, rng, P, cfg=cfg(rng) if cfg else None, **(cfg_kw or {}))
    eng = rg.Engine(G, P, **engine_kw)
    eng.load_state(st)
    PG._run_against_oracle(rg, eng, st, rng, 3, f"{label} P={P}", reject_p=0.2, heartbeat_p=0.1)
    info = eng.device_info()
    assert info["last_tick_kernel"] == kernel, info
    if streaming is not None:
        assert info["last_tick_streaming"] == streaming, info
    if offset_bits is not None:
        assert info["last_tick_offset_bits"] == offset_bits, info
    eng.close()


@pytest.mark.parametrize("policy,streaming", [("PLAIN", 0), ("STREAM_MSGS", 1), ("STREAM_ALL", 2)])
@pytest.mark.parametrize("n_slots", SLOTS)
def test_dense_tick_cached_and_streamed(rg, n_slots, policy, streaming):
    run_dense(rg, n_slots, 31000, f"dense {policy}", "k_tick_lane", streaming=streaming, offset_bits=32,
              cache_policy=getattr(rg.CACHE, policy))


@pytest.mark.parametrize("n_slots", SLOTS)
def test_dense_tick_resident_range(rg, n_slots):
    """k_tick_split: the first 256 groups' state stays in the cache, the ragged rest is streamed -- both bodies in the launch"""
    run_dense(rg, n_slots, 31100, "dense resident", "k_tick_split", streaming=2, offset_bits=32,
              cache_policy=rg.CACHE.RESIDENT, cache_resident_groups=256)


@pytest.mark.parametrize("n_slots", SLOTS)
def test_dense_tick_64bit_offsets(rg, n_slots):
    run_dense(rg, n_slots, 31200, "dense ix64", "k_tick_lane", offset_bits=64, flags=rg.CFGF.IX64)


@pytest.mark.parametrize("n_slots", SLOTS)
def test_dense_tick_group_commit(rg, n_slots):
    rng = np.random.default_rng(31300 + n_slots)
    st = dense_state(rg, rng, n_slots, group_commit_frac=0.6)
    assert ((st["cfg"] >> 19) & 1).any()
    eng = rg.Engine(G, n_slots)
    eng.load_state(st)
    cl = PG.oracle_from_state(st)
    mci, used = eng.maximal_committed_index(with_flag=True)
    for g in range(G):
        v, f = cl.mci(g)
        assert mci[g] == v and bool(used[g]) == f, (g, mci[g], v, used[g], f)
    PG._run_against_oracle(rg, eng, st, rng, 3, f"group commit P={n_slots}", reject_p=0.2)
    info = eng.device_info()
    assert info["last_tick_kernel"] == "k_tick_lane" and info["last_tick_streaming"] == 0, info
    eng.close()


def class_placed(rg, P):
    """The first two blocks name 3 slots at most, the rest up to P (and every block of the rest names slot P - 1)."""
    def cfg(rng):
        c = fuzz.class_placed_cfg(rng, [(128, 3), (G - 128, P)], P, missing_progress_frac=0.05)
        c[128::64] = full_cfg(rg, P)
        return c
    return cfg


@pytest.mark.parametrize("n_slots", [p for p in SLOTS if p >= 4])
def test_class_placed_shard(rg, n_slots):
    run_dense(rg, n_slots, 31400, "classes", "k_tick_classes", streaming=0, offset_bits=32, cfg=class_placed(rg, n_slots),
              cache_policy=rg.CACHE.PLAIN)


def send_engine(rg, rng, P, cap, term):
    st = dense_state(rg, rng, P, term=term, missing_progress_frac=0.05)
    sendstage.mark_pending_conf(rng, st)
    eng = rg.Engine(G, P, max_inflight=cap)
    eng.load_state(st)
    cl = O.Cluster(G)
    cl.load_soa(st, term=term, max_inflight=cap)
    cl.set_own_inflights(True)
    return st, eng, cl


def send_msgs(rng, cl, st, msgs, touched=None):
    cl.store_soa(st)
    fuzz.random_msgs(rng, st, msgs, sent_p=0.0, heartbeat_p=0.2)
    sendstage.prepare_msgs(msgs)
    if touched is not None:
        keep = np.zeros(G, dtype=bool)
        keep[touched] = True
        msgs["m_flags"][~keep] = 0


def check_stage(rg, eng, cl, st, gout, cap, max_entries, skip, what):
    items = sendstage.compare_items(eng.send_items(), cl.send_stage_soa(gout, max_entries, skip_bcast_commit=skip))
    apply_snapshots(rg, eng, cl, st, items)
    check_send_state(rg, eng, cl, st, cap, what)
    return len(items)


@pytest.mark.parametrize("n_slots", SLOTS)
def test_tick_plus_send_stage_in_one_launch(rg, n_slots):
    rng = np.random.default_rng(31500 + n_slots)
    cap, max_entries = 4, 2
    st, eng, cl = send_engine(rg, rng, n_slots, cap, term=6)
    msgs, mb, gout = O.alloc_msgs(G, n_slots), rg.MsgBuffers(G, n_slots, eng.stride), np.zeros(G, dtype=np.uint32)
    n_items = 0
    for t in range(3):
        send_msgs(rng, cl, st, msgs)
        for k in KEYS:
            getattr(mb, k)[...] = msgs[k]
        eng.tick_send(mb, max_entries, skip_bcast_commit=t == 1)
        assert eng.device_info()["last_tick_kernel"] == "k_tick_send"
        cl.tick_soa(msgs, gout)
        _, out = eng.results()
        assert (out == gout).all(), (t, np.nonzero(out != gout)[0][:5])
        n_items += check_stage(rg, eng, cl, st, gout, cap, max_entries, t == 1, f"tick_send P={n_slots} tick {t}")
    assert n_items > 0 or n_slots == 1
    eng.close()


@pytest.mark.parametrize("n_slots", SLOTS)
def test_two_launch_send_dense_and_over_the_list(rg, n_slots):
    """rg_tick + rg_send_appends (the dense stage, work items into the columns), then rg_ingest_tick + rg_send_appends (the
    stage over the list of touched groups)."""
    rng = np.random.default_rng(31600 + n_slots)
    cap, max_entries = 4, 2
    st, eng, cl = send_engine(rg, rng, n_slots, cap, term=6)
    msgs, mb, gout = O.alloc_msgs(G, n_slots), rg.MsgBuffers(G, n_slots, eng.stride), np.zeros(G, dtype=np.uint32)
    msgs["m_logterm"][...] = 0
    n_items = 0
    for t in range(3):
        touched = None if t != 1 else np.sort(rng.choice(G, size=20, replace=False))
        send_msgs(rng, cl, st, msgs, touched)
        if touched is None:
            for k in KEYS:
                getattr(mb, k)[...] = msgs[k]
            eng.tick(mb)
        else:
            n, dup = eng.ingest_tick(A.records(msgs, touched, n_slots, rng))
            assert dup == 0 and n == int(msgs["m_flags"].any(axis=1).sum())
        gout[:] = 0
        cl.tick_soa(msgs, gout)
        eng.send_appends(max_entries)
        n_items += check_stage(rg, eng, cl, st, gout, cap, max_entries, False, f"two launches P={n_slots} tick {t}")
    assert n_items > 0 or n_slots == 1
    eng.close()


@pytest.mark.parametrize("n_slots", SLOTS)
def test_fused_ticks(rg, n_slots):
    import torch
    rng = np.random.default_rng(31700 + n_slots)
    T = 3
    st = dense_state(rg, rng, n_slots)
    seq, fus = rg.Engine(G, n_slots), rg.Engine(G, n_slots)
    seq.load_state(st)
    fus.load_state(st)
    cl = PG.oracle_from_state(st)
    msgs, gout = O.alloc_msgs(G, n_slots), np.zeros(G, dtype=np.uint32)
    del msgs["m_logterm"]
    dev, want_out, want_commit = [], [], []
    for t in range(T):
        cl.store_soa(st)
        fuzz.random_msgs(rng, st, msgs, reject_p=0.2)
        dev.append(A._to_device(torch, msgs, False))
        seq.tick_device(*[c.data_ptr() for c in dev[-1]])
        cl.tick_soa(msgs, gout)
        PG.assert_same(seq, cl, st, gout, f"sequential P={n_slots} tick {t}")
        want_out.append(gout.copy())
        want_commit.append(st["commit"].copy())
    out_t = torch.zeros((T, G), dtype=torch.int32, device="cuda")
    commit_t = torch.zeros((T, G), dtype=torch.int64, device="cuda")
    assert fus.tick_device_fused([[c.data_ptr() for c in d] for d in dev], out_t.data_ptr(), commit_t.data_ptr()) == T
    fus.sync()
    ot, ct = out_t.cpu().numpy().view(np.uint32), commit_t.cpu().numpy().view(np.uint64)
    for t in range(T):
        assert (ot[t] == want_out[t]).all() and (ct[t] == want_commit[t]).all(), t
    PG.assert_same(fus, cl, st, gout, f"fused P={n_slots}")
    a, b = seq.read_state(), fus.read_state()
    for k in fuzz.STATE_KEYS + ("out",):
        assert (a[k] == b[k]).all(), k
    seq.close()
    fus.close()


@pytest.mark.parametrize("n_slots", SLOTS)
def test_ingest_paths(rg, n_slots):
    """rg_ingest + rg_tick_ingested (k_tick_list) and the one-call rg_ingest_tick (one small launch), about 20 records each."""
    rng = np.random.default_rng(31800 + n_slots)
    st = dense_state(rg, rng, n_slots)
    eng = rg.Engine(G, n_slots)
    eng.load_state(st)
    cl = PG.oracle_from_state(st)
    msgs, gout = O.alloc_msgs(G, n_slots), np.zeros(G, dtype=np.uint32)
    for t in range(3):
        cl.store_soa(st)
        fuzz.random_msgs(rng, st, msgs)
        touched = np.sort(rng.choice(G, size=max(4, 20 // n_slots), replace=False))
        keep = np.zeros(G, dtype=bool)
        keep[touched] = True
        msgs["m_flags"][~keep] = 0
        recs = A.records(msgs, touched, n_slots, rng)
        with_events = np.nonzero(msgs["m_flags"].any(axis=1))[0]
        if t == 1:
            assert eng.ingest_tick(recs) == (len(with_events), 0)
        else:
            assert eng.ingest(recs) == 0
            assert eng.tick_ingested() == len(with_events)
        gout[:] = 0
        cl.tick_soa(msgs, gout)
        groups, commit, out = eng.ingested_results()
        order = np.argsort(groups)
        cl.store_soa(st)
        assert (groups[order] == with_events).all()
        assert (commit[order] == st["commit"][with_events]).all() and (out[order] == gout[with_events]).all()
        PG.assert_same(eng, cl, st, gout, f"ingest P={n_slots} tick {t}")
    eng.close()


@pytest.mark.parametrize("form", ["flush", "flush_send", "mailbox", "mailbox_send"])
@pytest.mark.parametrize("n_slots", SLOTS)
def test_host_mirror_small_flushes(rg, n_slots, form):
    """RawNode::step through the host mirror, three rounds of steps and one small flush each: the one-launch flush, the same with
    the send stage inside (rg_flush_send, device Inflights), and both served by the resident workgroup (rg_mailbox_start)."""
    rng = np.random.default_rng(31900 + n_slots)
    send, mailbox = form.endswith("send"), form.startswith("mailbox")
    cap, max_entries = 4, 2
    if send:
        st, eng, cl = send_engine(rg, rng, n_slots, cap, term=A.TERM)
    else:
        st = dense_state(rg, rng, n_slots)
        eng = rg.Engine(G, n_slots)
        eng.load_state(st)
        cl = O.Cluster(G)
        cl.load_soa(st, term=A.TERM)
    self_slot = ((st["cfg"] >> 16) & 7).astype(np.int64)
    for g in range(G):
        eng.set_peers(g, list(range(1, n_slots + 1)), A.TERM)
    if mailbox:
        eng.mailbox_start()
    msgs, gout = O.alloc_msgs(G, n_slots), np.zeros(G, dtype=np.uint32)
    msgs["m_logterm"][...] = 0
    for t in range(3):
        touched = np.sort(rng.choice(G, size=12, replace=False))
        if send:
            send_msgs(rng, cl, st, msgs, touched)
        else:
            cl.store_soa(st)
            fuzz.random_msgs(rng, st, msgs)
            keep = np.zeros(G, dtype=bool)
            keep[touched] = True
            msgs["m_flags"][~keep] = 0
        A.clean_for_mirror(msgs, n_slots, self_slot)
        A.mirror_steps(rg, eng, msgs, touched, n_slots, self_slot)
        if send:
            eng.flush_send(max_entries)
        else:
            eng.flush()
        gout[:] = 0
        cl.tick_soa(msgs, gout)
        with_events = np.nonzero(msgs["m_flags"].any(axis=1))[0]
        groups, commit, out = eng.ingested_results()
        order = np.argsort(groups)
        assert (groups[order] == with_events).all(), t
        assert (out[order] == gout[with_events]).all(), t
        if send:
            check_stage(rg, eng, cl, st, gout, cap, max_entries, False, f"{form} P={n_slots} round {t}")
        else:
            PG.assert_same(eng, cl, st, gout, f"{form} P={n_slots} round {t}")
        assert (commit[order] == st["commit"][with_events]).all(), t
    if mailbox:
        assert eng.mailbox_stats()[0] >= 1, "no flush was served by the resident workgroup"
        eng.mailbox_stop()
    eng.close()


@pytest.mark.parametrize("variant", ["VARIANT_DEFAULT", "VARIANT_LANE", "VARIANT_COOP"])
@pytest.mark.parametrize("n_slots", SLOTS)
def test_recompute(rg, n_slots, variant):
    rng = np.random.default_rng(32000 + n_slots)
    st = dense_state(rg, rng, n_slots)
    st["commit"][:] = st["commit"] // 2  # leave room to commit
    eng = rg.Engine(G, n_slots, variant=getattr(rg, variant))
    eng.load_state(st)
    cl = PG.oracle_from_state(st)
    mci = eng.maximal_committed_index()
    assert (mci == np.array([cl.mci(g)[0] for g in range(G)], dtype=np.uint64)).all()
    eng.recompute()
    gout = np.array([1 if cl.maybe_commit(g) else 0 for g in range(G)], dtype=np.uint32)
    PG.assert_same(eng, cl, st, gout, f"recompute P={n_slots} {variant}")
    eng.close()


def ride_case(rg, path):
    """engine arguments, the kernel that runs, publications' events per dense tick that ride on its packet"""
    return {"lane": (dict(cache_policy=rg.CACHE.PLAIN), "k_tick_lane", 1),
            "split": (dict(cache_policy=rg.CACHE.RESIDENT, cache_resident_groups=256), "k_tick_split", 1),
            "classes": (dict(cache_policy=rg.CACHE.PLAIN), "k_tick_classes", 1),
            "lds": (dict(variant=rg.VARIANT_LDS), "k_tick_lds", 0)}[path]


@pytest.mark.parametrize("n_slots,path", [(p, k) for p in SLOTS for k in ("lane", "split", "classes", "lds") if k != "classes" or p >= 4])
def test_publication_event_rides_on_the_tick_packet(rg, n_slots, path):
    """A one-rank communicator: the publication's event goes out on the dispatch packet of the lane, split and class kernels
    (events_on_tick_packets grows by one per dense tick), not on the LDS variant's; the replica equals the commit column after
    every publication, and the state the oracle's."""
    import torch
    from raft_rs_amd import engine as E
    engine_kw, kernel, rides = ride_case(rg, path)
    rng = np.random.default_rng(32100 + n_slots)
    st = dense_state(rg, rng, n_slots, cfg=class_placed(rg, n_slots)(rng) if path == "classes" else None)
    eng = rg.Engine(G, n_slots, **engine_kw)
    eng.load_state(st)
    eng.comm_init(0, 1, unique_id=E.comm_unique_id(), ring_ticks=2)
    cl = PG.oracle_from_state(st)
    msgs, gout = O.alloc_msgs(G, n_slots), np.zeros(G, dtype=np.uint32)
    del msgs["m_logterm"]
    moved = 0
    for t in range(3):
        cl.store_soa(st)
        before = st["commit"].copy()
        fuzz.random_msgs(rng, st, msgs)
        d = A._to_device(torch, msgs, False)
        n0 = eng.publish_stats()["events_on_tick_packets"]
        eng.tick_device(*[c.data_ptr() for c in d])
        eng.publish_commit()
        assert eng.publish_stats()["events_on_tick_packets"] == n0 + rides, (t, path)
        assert eng.device_info()["last_tick_kernel"] == kernel
        assert np.array_equal(eng.published_commit(0), eng.read_column(rg.COL.COMMIT)), t
        cl.tick_soa(msgs, gout)
        PG.assert_same(eng, cl, st, gout, f"publication {path} P={n_slots} tick {t}")
        moved += int((st["commit"] != before).sum())
    assert moved > 0
    eng.comm_destroy()
    eng.close()
