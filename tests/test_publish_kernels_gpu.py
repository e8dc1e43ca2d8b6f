"""GPU: the publication slice every commit-storing kernel writes, kernel by kernel, against the host twin.

Each case runs one engine at world size 1 behind a callback transport that copies the slice it is handed (dev_send) to the
host. After every publication interval the slice is compared with rg_pub_accumulate_host(commit at the interval's start,
commit now) in canonical form (tests/pubcheck.py), its decoded advance with the commit column, and the replica with the commit
column. The traffic is the synthetic workload with crafted acks on every third group (and the last one): advances of 0 to
2^32 + 3, bytes that cross 255 only on the second or third tick of an interval. A twin engine takes the same ticks one at a
time (rg_tick_device), so every path must also leave the commit column the twin leaves.

Dense cases assert which kernel ran (rg_device_info: last_tick_kernel / last_tick_offset_bits / last_tick_streaming): a silent
fallback to another kernel does not count as coverage."""
import numpy as np
import pytest

import pubcheck
from raft_rs_amd.engine import COL

pytestmark = pytest.mark.gpu


class Dev:
    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (int(ptr), False), "version": 2}


class Publisher:
    """rg_comm_init(0, 1) with a host transport that keeps a copy of every slice it moves."""

    def __init__(self, eng, cap):
        import torch
        from raft_rs_amd import engine as E
        self.torch, self.E = torch, E
        self.eng, self.G, self.cap = eng, eng.n_groups, cap
        self.bytes = E.pub_bytes_per_rank(self.G, cap)
        assert self.bytes == pubcheck.layout(self.G, cap)[2]
        self.slices = []
        eng.comm_init(0, 1, transport=self._allgather, ring_ticks=4, overflow_slots=cap)
        self.c0 = eng.read_column(COL.COMMIT)
        assert np.array_equal(eng.published_commit(0), self.c0)

    def _allgather(self, dev_send, dev_recv, nbytes, stream):
        torch = self.torch
        torch.cuda.synchronize()
        buf = torch.as_tensor(Dev(dev_send, nbytes), device="cuda").cpu()
        torch.as_tensor(Dev(dev_recv, nbytes), device="cuda").copy_(buf.cuda())  # (world 1: the gathered buffer is the slice)
        torch.cuda.synchronize()
        self.slices.append(buf.numpy().copy())
        return 0

    def publish_and_check(self, what):
        n0 = len(self.slices)
        self.eng.publish_commit()
        assert len(self.slices) == n0 + 1 and len(self.slices[-1]) == self.bytes, (what, "not a delta publication")
        sl = self.slices[-1]
        c1 = self.eng.read_column(COL.COMMIT)
        want = pubcheck.new_slice(self.G, self.cap)
        self.E.pub_accumulate_host(self.c0, c1, want, self.cap)
        pubcheck.assert_same_slice(sl, want, self.G, self.cap, what)
        adv = pubcheck.decode(sl, self.G, self.cap)
        bad = np.nonzero(adv != c1 - self.c0)[0]
        assert bad.size == 0, (what, "decoded advance", bad[:5], adv[bad[:5]], (c1 - self.c0)[bad[:5]])
        rep = self.eng.published_commit(0)
        bad = np.nonzero(rep != c1)[0]
        assert bad.size == 0, (what, "replica", bad[:5], rep[bad[:5]], c1[bad[:5]])
        moved = c1 - self.c0
        self.c0 = c1
        return moved


def craft(eng, twin, P, wl, gc, groups, base=1000):
    """Overwrite `groups` of both engines with the crafted state of pubcheck.crafted_state (leader in slot 0, all P voting)."""
    st = eng.read_state()
    cs = pubcheck.crafted_state(eng.n_groups, P, base, gc)
    for k in ("match", "next", "pr_commit", "pend_snap", "pend_rs", "gid"):
        st[k][:, groups] = cs[k][:, groups]
    for k in ("pflags", "commit", "term_lo", "term_hi", "cfg"):
        st[k][groups] = cs[k][groups]
    for e in (eng, twin):
        e.load_state(st)


class Traffic:
    """Ticks of workload `wl`, with crafted acks on `groups`, generated and applied one at a time on the twin engine."""

    def __init__(self, rg, twin, P, wl, groups, sparse=False, gc=False, classes=False, device_sends=False):
        import torch
        self.rg, self.torch, self.twin, self.P, self.wl, self.groups = rg, torch, twin, P, wl, groups
        self.sparse, self.gc, self.classes, self.k, self.seen = sparse, gc, classes, 0, set()
        self.device_sends = device_sends  # (engines with device Inflights: no SENT / INS_FULL events from the host)

    def tick(self, adv):
        """adv: u64[len(groups)] advances of the crafted groups. Returns the device columns (m_index, m_commit, m_hint, m_rs,
        m_flags) and the host copies."""
        torch, twin, P, g = self.torch, self.twin, self.P, self.groups
        cols = [torch.zeros((P, twin.stride), dtype=torch.int64, device="cuda") for _ in range(4)]
        flags = torch.zeros((twin.n_groups, 8), dtype=torch.uint8, device="cuda")
        if not self.sparse:
            twin.workload_gen(self.wl, self.k, *[c.data_ptr() for c in cols], flags.data_ptr(), sorted_classes=self.classes,
                              group_commit=self.gc)
        self.k += 1
        h = {k: c.cpu().numpy().view(np.uint64).copy() for k, c in zip(("m_index", "m_commit", "m_hint", "m_rs"), cols)}
        h["m_flags"] = flags.cpu().numpy().copy()
        if self.device_sends:
            h["m_flags"] &= np.uint8(~(self.rg.MF.SENT | self.rg.MF.INS_FULL) & 0xff)
        commit = twin.read_column(COL.COMMIT)[g]
        target = commit + adv
        for k in ("m_index", "m_commit", "m_hint", "m_rs"):
            h[k][:, g] = 0
        h["m_flags"][g, :] = 0
        moved = target != commit
        for p in range(P):
            h["m_index"][p, g] = target
            h["m_commit"][p, g] = target if p == 0 else commit
            h["m_flags"][g, p] = np.where(moved, self.rg.MF.VALID | (self.rg.MF.APPEND if p == 0 else 0), 0)
        for c, k in zip(cols, ("m_index", "m_commit", "m_hint", "m_rs")):
            c.copy_(torch.from_numpy(h[k].view(np.int64)))
        flags.copy_(torch.from_numpy(h["m_flags"]))
        twin.tick_device(*[c.data_ptr() for c in cols], flags.data_ptr())
        after = twin.read_column(COL.COMMIT)[g]
        assert (after == target).all(), ("the crafted advances did not commit", np.nonzero(after != target)[0][:5])
        self.seen.update(int(a) for a in np.unique(adv))
        return cols + [flags], h


def records(h, groups, P):
    """The crafted groups' messages of one tick as wire records (slot order inside a group: the leader's append first)."""
    from raft_rs_amd.engine import WIRE_DTYPE
    gs = np.repeat(groups, P)
    ps = np.tile(np.arange(P), len(groups))
    keep = h["m_flags"][gs, ps] != 0
    gs, ps = gs[keep], ps[keep]
    rec = np.zeros(len(gs), dtype=WIRE_DTYPE)
    rec["group"], rec["slot"], rec["flags"] = gs, ps, h["m_flags"][gs, ps]
    rec["index"], rec["commit"] = h["m_index"][ps, gs], h["m_commit"][ps, gs]
    return rec


INTERVALS = (1, 2, 3, 3)


def run_case(rg, eng, twin, P, wl, apply, groups, expect=None, sparse=False, gc=False, classes=False, base=1000,
             intervals=INTERVALS, fused=False, device_sends=False):
    """Publication intervals of `intervals` ticks each; apply(ticks) runs them on `eng` (fused: all of one interval at
    once; otherwise tick by tick)."""
    craft(eng, twin, P, wl, gc, groups, base)
    pub = Publisher(eng, 3 * eng.n_groups)  # (a list long enough for every crafted group: no slice is lost)
    tr = Traffic(rg, twin, P, wl, groups, sparse=sparse, gc=gc, classes=classes, device_sends=device_sends)
    moved_big = 0
    for i, T in enumerate(intervals):
        adv = pubcheck.pattern_advances(len(groups), T, seed=i)
        ticks = []
        for t in range(T):
            ticks.append(tr.tick(adv[t]))
            if not fused:
                apply([ticks[-1]])
        if fused:
            apply(ticks)
        c = eng.read_column(COL.COMMIT)
        assert np.array_equal(c, twin.read_column(COL.COMMIT)), (i, "commit column differs from the twin's")
        if expect is not None:
            info = eng.device_info()
            assert {k: info[k] for k in expect} == expect, info
        moved = pub.publish_and_check((i, T))
        moved_big += int((moved > 255).sum())
    assert set(pubcheck.EDGES) <= tr.seen, tr.seen
    assert moved_big > len(groups) // 5, moved_big
    return pub


def crafted_groups(G, step=3):
    g = np.arange(0, G, step, dtype=np.int64)
    return g if g[-1] == G - 1 else np.append(g, G - 1)


def dense(eng):
    return lambda ticks: [eng.tick_device(*[c.data_ptr() for c in cols]) for cols, _ in ticks]


G0 = 20_000 + 13


@pytest.mark.parametrize("policy,bits,streaming", [("PLAIN", 32, 0), ("STREAM_MSGS", 32, 1), ("STREAM_ALL", 32, 2), ("PLAIN", 64, 0),
                                                   ("STREAM_MSGS", 64, 1), ("STREAM_ALL", 64, 2)])
def test_lane_kernel_slices(rg, policy, bits, streaming):
    """k_tick_lane and its streamed twins, with 32-bit cell offsets and RG_CFGF_IX64's 64-bit ones (near the top of the
    index range for the latter)."""
    P, wl = 5, 2
    flags = rg.CFGF.IX64 if bits == 64 else 0
    eng = rg.Engine(G0, P, cache_policy=getattr(rg.CACHE, policy), flags=flags)
    twin = rg.Engine(G0, P)
    for e in (eng, twin):
        e.workload_init(wl)
    run_case(rg, eng, twin, P, wl, dense(eng), crafted_groups(G0), base=2**62 if bits == 64 else 1000,
             expect={"last_tick_kernel": "k_tick_lane", "last_tick_offset_bits": bits, "last_tick_streaming": streaming})
    eng.close()
    twin.close()


def test_split_kernel_slices(rg):
    """k_tick_split: a resident head of 4096 groups, the rest streamed, in one launch."""
    P, wl = 5, 2
    eng = rg.Engine(G0, P, cache_policy=rg.CACHE.RESIDENT, cache_resident_groups=4096)
    twin = rg.Engine(G0, P)
    for e in (eng, twin):
        e.workload_init(wl)
    assert 0 < eng.device_info()["resident_groups"] < G0 // 2, eng.device_info()
    run_case(rg, eng, twin, P, wl, dense(eng), crafted_groups(G0),
             expect={"last_tick_kernel": "k_tick_split", "last_tick_offset_bits": 32, "last_tick_streaming": 2})
    eng.close()
    twin.close()


def test_classes_kernel_slices(rg):
    """k_tick_classes: workload 5 placed by size class (3, 5, 7 peers) in a 7-slot engine; the crafted groups lie in the
    7-peer range (crafting a group gives it all seven voters)."""
    P, wl = 7, 5
    eng, twin = rg.Engine(G0, P), rg.Engine(G0, P)
    for e in (eng, twin):
        e.workload_init(wl, sorted_classes=True)
    cls = eng.size_classes()
    assert [q for _, _, q in cls] == [3, 5, 7], cls
    first7 = cls[2][0]
    groups = np.arange(first7, G0, 2, dtype=np.int64)
    groups = groups if groups[-1] == G0 - 1 else np.append(groups, G0 - 1)
    run_case(rg, eng, twin, P, wl, dense(eng), groups, classes=True,
             expect={"last_tick_kernel": "k_tick_classes", "last_tick_offset_bits": 32})
    eng.close()
    twin.close()


@pytest.mark.parametrize("variant,kernel", [("VARIANT_LDS", "k_tick_lds"), ("VARIANT_LDS_DMA", "k_tick_lds"),
                                            ("VARIANT_COMPACT", "k_tick_compact")])
def test_lds_and_compact_kernel_slices(rg, variant, kernel):
    P, wl = 5, 2
    eng = rg.Engine(G0, P, variant=getattr(rg, variant))
    twin = rg.Engine(G0, P)
    for e in (eng, twin):
        e.workload_init(wl)
    run_case(rg, eng, twin, P, wl, dense(eng), crafted_groups(G0), expect={"last_tick_kernel": kernel, "last_tick_streaming": 0})
    eng.close()
    twin.close()


def test_group_commit_kernel_slices(rg):
    """The group-commit instantiation of k_tick_lane (some group has ProgressTracker.group_commit)."""
    P, wl = 5, 2
    eng, twin = rg.Engine(G0, P), rg.Engine(G0, P)
    for e in (eng, twin):
        e.workload_init(wl, group_commit=True)
    run_case(rg, eng, twin, P, wl, dense(eng), crafted_groups(G0), gc=True,
             expect={"last_tick_kernel": "k_tick_lane", "last_tick_offset_bits": 32, "last_tick_streaming": 0})
    eng.close()
    twin.close()


@pytest.mark.parametrize("form", ["device", "host"])
def test_tick_send_kernel_slices(rg, form):
    """k_tick_send: rg_tick_device_send and the host-buffer rg_tick_send."""
    P, wl = 5, 2
    eng, twin = rg.Engine(G0, P, max_inflight=8), rg.Engine(G0, P, max_inflight=8)
    for e in (eng, twin):
        e.workload_init(wl)
    mb = rg.MsgBuffers(G0, P, eng.stride)

    def apply(ticks):
        for cols, h in ticks:
            if form == "device":
                eng.tick_device_send(*[c.data_ptr() for c in cols])
            else:
                for k in ("m_index", "m_commit", "m_hint", "m_rs", "m_flags"):
                    getattr(mb, k)[...] = h[k]
                eng.tick_send(mb)

    run_case(rg, eng, twin, P, wl, apply, crafted_groups(G0), device_sends=True,
             expect={"last_tick_kernel": "k_tick_send", "last_tick_offset_bits": 32})
    eng.close()
    twin.close()


@pytest.mark.parametrize("gc", [False, True])
@pytest.mark.parametrize("T", [1, 3, 8])
def test_fused_kernel_slices(rg, T, gc):
    """k_tick_fused over T ticks per publication interval: the launch's summed advance lands in the byte once."""
    P, wl = 5, 2
    eng, twin = rg.Engine(G0, P), rg.Engine(G0, P)
    for e in (eng, twin):
        e.workload_init(wl, group_commit=gc)
    import torch
    out_t = torch.zeros((8, G0), dtype=torch.int32, device="cuda")

    def apply(ticks):
        assert eng.tick_device_fused([[c.data_ptr() for c in cols] for cols, _ in ticks], out_t.data_ptr()) == len(ticks)

    run_case(rg, eng, twin, P, wl, apply, crafted_groups(G0), gc=gc, fused=True, intervals=(T, T, T))
    eng.close()
    twin.close()


@pytest.mark.parametrize("form", ["ingest_tick", "ingest_then_tick_ingested"])
def test_sparse_tick_slices(rg, form):
    """The sparse path: rg_ingest_tick, and rg_ingest + rg_tick_ingested, over the crafted groups' records only."""
    P, wl = 3, 2
    eng, twin = rg.Engine(G0, P), rg.Engine(G0, P)
    for e in (eng, twin):
        e.workload_init(wl)
    groups = crafted_groups(G0, step=7)

    def apply(ticks):
        for _, h in ticks:
            rec = records(h, groups, P)
            if form == "ingest_tick":
                n, dup = eng.ingest_tick(rec)
                assert dup == 0
            else:
                assert eng.ingest(rec) == 0
                eng.tick_ingested()

    run_case(rg, eng, twin, P, wl, apply, groups, sparse=True)
    eng.close()
    twin.close()


@pytest.mark.parametrize("mode", ["small", "small_send", "dense"])
def test_mirror_flush_slices(rg, mode):
    """The host mirror (rg_step ... rg_flush): a small batch in ONE launch (k_flush_small; with a send request
    k_flush_small_send) and a flush with most groups dirty (the dense tick)."""
    P, TERM = 3, 5
    G = 1024 + 5 if mode == "dense" else G0
    ins = 8 if mode == "small_send" else 0
    eng, twin = rg.Engine(G, P, max_inflight=ins), rg.Engine(G, P, max_inflight=ins)
    for e in (eng, twin):
        e.workload_init(2)
    groups = crafted_groups(G, step=1) if mode == "dense" else np.sort(np.append(np.arange(5, G, G // 60)[:60], G - 1))
    for g in groups:
        eng.set_peers(int(g), [11, 12, 13], TERM)

    def apply(ticks):
        for _, h in ticks:
            for g in groups:
                g = int(g)
                if not h["m_flags"][g, 0]:
                    continue
                x, c = int(h["m_index"][0, g]), int(h["m_commit"][1, g])
                eng.local_append(g, x)
                eng.local_persisted(g, x)
                for p in range(1, P):
                    eng.step(g, 11 + p, TERM, x, commit=c)
            if mode == "small_send":
                eng.flush_send()
            else:
                eng.flush()

    run_case(rg, eng, twin, P, 2, apply, groups, sparse=True, base=1000)
    eng.close()
    twin.close()


@pytest.mark.parametrize("variant", ["VARIANT_DEFAULT", "VARIANT_COOP"])
def test_recompute_slices(rg, variant):
    """rg_recompute (k_recompute; VARIANT_COOP: k_recompute_coop) after the leaders of the crafted groups appended alone and
    their configuration shrank to the leader: the commit index jumps to the leader's match."""
    from raft_rs_amd.engine import COL
    P, wl = 3, 2
    eng, twin = rg.Engine(G0, P, variant=getattr(rg, variant)), rg.Engine(G0, P)
    for e in (eng, twin):
        e.workload_init(wl)
    groups = crafted_groups(G0, step=11)
    craft(eng, twin, P, wl, False, groups)
    pub = Publisher(eng, 3 * G0)
    seen = set()
    for i, T in enumerate(INTERVALS):
        adv = pubcheck.pattern_advances(len(groups), T, seed=i)
        for t in range(T):
            commit = eng.read_column(COL.COMMIT)[groups]
            target = commit + adv[t]
            seen.update(int(a) for a in np.unique(adv[t]))
            mb = rg.MsgBuffers(G0, P, eng.stride)
            moved = target != commit
            mb.m_index[0, groups] = target
            mb.m_commit[0, groups] = target
            mb.m_flags[groups, 0] = np.where(moved, rg.MF.VALID | rg.MF.APPEND, 0)
            for e in (eng, twin):
                e.tick(mb)  # the leader alone: match[0] = target, no quorum yet
                assert (e.read_column(COL.COMMIT)[groups] == commit).all()
                for g in groups[moved]:
                    e.set_config(int(g), rg.cfg_make(0b001, present=0b111))
                e.recompute()
                for g in groups[moved]:  # (back to three voters, all acked up to the old commit: the next step starts alike)
                    e.set_config(int(g), rg.cfg_make(0b111))
            got = eng.read_column(COL.COMMIT)
            assert (got[groups] == target).all(), (i, t)
            assert np.array_equal(got, twin.read_column(COL.COMMIT))
        pub.publish_and_check((variant, i))
    assert set(pubcheck.EDGES) <= seen, seen
    eng.close()
    twin.close()
