"""GPU: write-behind launches of the dense tick's read mirror (k_tick_mirror_wb, k_mirror_settle: raft_rs_amd/csrc/rg_mirror.h) against
an engine created without the mirror (RG_CFGF_NO_READ_MIRROR) and against the oracle: a streak of rg_tick_device calls with nothing
between them, then ONE of the calls that must find the two columns current -- and the calls that must not end the streak."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fuzz
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WB_AFTER = int(re.search(r"#define RG_MIRROR_WB_AFTER (\d+)",
                         open(os.path.join(ROOT, "raft_rs_amd", "csrc", "rg_mirror_host.h")).read()).group(1))
TERM = 4
SHAPES = [(65, 3), (193, 5), (193, 3), (65, 5)]
MSG_KEYS = ("m_index", "m_commit", "m_hint", "m_rs", "m_flags")


class Streak:
    """A mirror-on engine, its mirror-less twin and the oracle over one pre-generated stream (the workload generator's, made on the
    host from the oracle's columns, so that nothing has to look at the engines between ticks); every tick's messages on the device."""

    def __init__(self, rg, G, P, ticks, cache_policy=None, plant=None):
        import torch
        from raft_rs_amd import engine as E
        self.rg, self.G, self.P = rg, G, P
        kw = {} if cache_policy is None else {"cache_policy": cache_policy}
        self.on = rg.Engine(G, P, device=0, flags=rg.CFGF.NO_SIZE_CLASSES, **kw)
        self.off = rg.Engine(G, P, device=0, flags=rg.CFGF.NO_SIZE_CLASSES | rg.CFGF.NO_READ_MIRROR, **kw)
        self.on.workload_init(rg.WL_MAJORITY)
        st = self.on.read_state()
        if plant:
            plant(st)
            self.on.load_state(st)
        self.off.load_state(st)
        self.st = st
        self.cl = O.Cluster(G)
        self.cl.load_soa(st, term=TERM - 1)
        self.gout = np.zeros(G, dtype=np.uint32)
        self.msgs = rg.MsgBuffers(G, P, self.on.stride)
        self.dev = []
        for t in range(ticks):  # the oracle runs ahead: tick t's messages come from its state after tick t - 1
            self.cl.store_soa(st)
            E.workload_gen_host(st, self.msgs, rg.WL_MAJORITY, t)
            self.dev.append([torch.from_numpy(np.ascontiguousarray(getattr(self.msgs, k)).view(np.uint8 if k == "m_flags" else np.int64).copy()).cuda()
                             for k in MSG_KEYS])
            self.cl.tick_soa(self.msgs.as_dict(), self.gout)
        self.cl.store_soa(st)
        self.t = 0

    def ptrs(self, t):
        return [d.data_ptr() for d in self.dev[t]]

    def ticks(self, n, engines=None):
        for _ in range(n):
            for e in engines or (self.on, self.off):
                e.tick_device(*self.ptrs(self.t))
            self.t += 1

    def compare(self, out=True, oracle=True):
        a, b = self.on.read_state(), self.off.read_state()
        diffs = fuzz.diff_states(a, b, self.G, self.P, present_only=False)
        assert not diffs, ("mirror on / off", diffs[:5])
        if out:
            assert (a["out"] == b["out"]).all()
        if oracle:
            assert self.t == len(self.dev)
            diffs = fuzz.diff_states(self.st, a, self.G, self.P)
            assert not diffs, ("oracle", diffs[:5])
            if out:
                assert (a["out"] == self.gout).all()
                for e in (self.on, self.off):
                    commit, o = e.results()
                    assert (commit == self.st["commit"]).all() and (o == self.gout).all()

    def close(self):
        self.on.close()
        self.off.close()


def streak_stats(s, n):
    st = s.on.mirror_stats()
    assert (st["build_launches"], st["packed_launches"], st["valid"], st["off"]) == (1, n - 1, 1, 0), st


# ---- the settle triggers, one per case: each finds the columns behind after WB_AFTER + 4 back-to-back ticks ----------------------
def trig_enter(rg, s):
    s.on.checkpoint()  # RG_ENTER


def trig_set_stream(rg, s):
    for e in (s.on, s.off):
        e.set_stream(0)  # (the ticks ran on a side stream: the settle runs there, before the engine moves)


def trig_read_match(rg, s):
    assert (s.on.read_column(rg.COL.MATCH) == s.off.read_column(rg.COL.MATCH)).all()
    assert s.on.mirror_stats()["valid"] == 1  # a KEEP call that settles leaves the plane


def trig_read_pr_commit(rg, s):
    assert (s.on.read_column(rg.COL.PR_COMMIT) == s.off.read_column(rg.COL.PR_COMMIT)).all()
    assert s.on.mirror_stats()["valid"] == 1


def trig_workload_gen(rg, s):
    """The generator reads st.match: what it makes from a settled engine is what it makes from the mirror-less one."""
    import torch
    got = []
    for e in (s.on, s.off):
        cols = [torch.zeros((s.P, e.stride), dtype=torch.int64, device="cuda") for _ in range(4)]
        flags = torch.zeros((s.G, 8), dtype=torch.uint8, device="cuda")
        e.workload_gen(rg.WL_MAJORITY, s.t, *[c.data_ptr() for c in cols], flags.data_ptr())
        e.sync()
        got.append([c.cpu().numpy() for c in cols] + [flags.cpu().numpy()])
    for x, y in zip(got[0][:4], got[1][:4]):
        assert (x[:, :s.G] == y[:, :s.G]).all()
    assert (got[0][4] == got[1][4]).all()
    assert s.on.mirror_stats()["valid"] == 1


def trig_column_ptr(rg, s):
    assert s.on.column_ptr(rg.COL.MATCH)
    assert s.on.mirror_stats()["off"] == 1


def trig_flush(rg, s):
    """The sparse flush (its by-hand invalidation): one AppendResponse through rg_step + rg_flush on both engines."""
    g = s.G - 1
    w = int(s.st["cfg"][g])
    slot = next(x for x in range(s.P) if x != ((w >> 16) & 7) and (w >> (24 + x)) & 1)
    for e in (s.on, s.off):
        e.step(g, slot + 1, TERM, int(min(int(s.st["term_hi"][g]), int(s.st["match"][slot, g]) + 1)))
        e.flush()


def trig_fused(rg, s):
    import torch
    for e in (s.on, s.off):
        out_t = torch.zeros((1, s.G), dtype=torch.int32, device="cuda")
        assert e.tick_device_fused([s.ptrs(s.t - 1)], out_t.data_ptr()) == 1  # (the last tick's messages again: stale acks)
        e.sync()


def ack_records(rg, s, groups):
    """One AppendResponse per listed group, from a follower, one entry ahead of its matched (the oracle's state is the engines')."""
    a = np.zeros(len(groups), dtype=rg.engine.WIRE_DTYPE)
    for k, g in enumerate(groups):
        w = int(s.st["cfg"][g])
        slot = next(x for x in range(s.P) if x != ((w >> 16) & 7) and (w >> (24 + x)) & 1)
        a[k]["group"], a[k]["slot"], a[k]["flags"] = g, slot, fuzz.MF_VALID
        a[k]["index"] = int(min(int(s.st["term_hi"][g]), int(s.st["match"][slot, g]) + 1))
        a[k]["commit"] = int(s.st["commit"][g])
    return a


def trig_list_tick(rg, s):
    """A list tick (k_tick_list): rg_ingest + rg_tick_ingested over a few groups of different waves."""
    groups = sorted({0, s.G // 2, s.G - 1})
    for e in (s.on, s.off):
        e.ingest(ack_records(rg, s, groups))
        assert e.tick_ingested() == len(groups)


def trig_ingest_tick(rg, s):
    """... and the one-trip road of the same tick (rg_ingest_tick: the sparse round trip's by-hand invalidation)."""
    groups = sorted({1 % s.G, s.G - 1})
    for e in (s.on, s.off):
        assert e.ingest_tick(ack_records(rg, s, groups))[0] == len(groups)


def trig_group_commit(rg, s):
    """A group-commit tick: one group switches ProgressTracker.group_commit on (rg_set_config), and the next dense tick runs the
    group-commit instantiation of k_tick_lane, which reads and writes the columns (the last tick's messages again: stale acks)."""
    g = s.G // 2
    for e in (s.on, s.off):
        e.set_config(g, int(s.st["cfg"][g]) | 0x80000)  # RG_CFG_GROUP_COMMIT
        e.tick_device(*s.ptrs(s.t - 1))
        e.sync()
    st = s.on.mirror_stats()
    assert st["valid"] == 0 and st["build_launches"] == 1, st  # (not a mirror launch)


# Tick + send (rg_tick_device_send, k_tick_send) is NOT a case: rg_send_check refuses it on an engine created with max_inflight == 0,
# and an engine with device Inflights keeps no mirror (rg_create), so no engine can hold columns behind a plane and run that plan.
# The plans of rg_tick_impl that are no mirror launch and CAN follow a streak without an RG_ENTER in between are the escape watch's
# return to k_tick_lane and a captured tick: both have tests of their own below.
TRIGGERS = {"list_tick": trig_list_tick, "ingest_tick": trig_ingest_tick, "group_commit": trig_group_commit, "enter": trig_enter, "set_stream": trig_set_stream, "read_match": trig_read_match, "read_pr_commit": trig_read_pr_commit,
            "workload_gen": trig_workload_gen, "column_ptr": trig_column_ptr, "flush": trig_flush, "fused": trig_fused}
ORACLE_TOO = {"enter", "set_stream", "read_match", "read_pr_commit", "workload_gen", "column_ptr"}


@pytest.mark.gpu
@pytest.mark.parametrize("trigger", sorted(TRIGGERS))
@pytest.mark.parametrize("G,P", SHAPES)
def test_a_streak_then_one_settle_trigger(rg, G, P, trigger):
    import torch
    n = WB_AFTER + 4
    s = Streak(rg, G, P, n)
    if trigger == "set_stream":
        side = torch.cuda.Stream()
        for e in (s.on, s.off):
            e.set_stream(side.cuda_stream)
    if trigger == "flush":
        for e in (s.on, s.off):
            for g in range(G):
                e.set_peers(g, list(range(1, P + 1)), TERM)
    s.ticks(n)
    streak_stats(s, n)
    TRIGGERS[trigger](rg, s)
    torch.cuda.synchronize()
    keep_out = trigger in ORACLE_TOO
    s.compare(out=keep_out, oracle=keep_out)
    s.close()


def raw_match(rg, s):
    """RG_COL_MATCH of the mirror-on engine as it stands in device memory, copied WITHOUT an entry point that settles: the column's
    address from RG_COL_NEXT's (rg_column_ptr of that column leaves the mirror alone) and the distance the mirror-less engine of the
    same shape has between the two; rg_sync in front, which keeps the streak."""
    import torch
    delta = s.off.column_ptr(rg.COL.NEXT) - s.off.column_ptr(rg.COL.MATCH)
    src = s.on.column_ptr(rg.COL.NEXT) - delta
    assert s.on.mirror_stats()["off"] == 0
    s.on.sync()

    class View:  # (a torch view over the arena: no copy is enqueued on the engine's stream, no entry point is called)
        __cuda_array_interface__ = {"shape": (s.P, s.on.stride), "typestr": "<i8", "data": (src, False), "version": 2}

    torch.cuda.synchronize()
    out = torch.as_tensor(View(), device="cuda").cpu().numpy().view(np.uint64)
    return out[:, :s.G]


@pytest.mark.gpu
@pytest.mark.parametrize("G,P", [(193, 5), (65, 3)])
def test_the_write_behind_kernel_is_what_a_streak_runs(rg, G, P):
    """rgr_mirror_stats counts both kinds of packed launch as one, so look at the memory: up to the last write-through launch the
    match column in device memory is the mirror-less engine's; after write-behind launches on this steady stream it is not (no
    wave stores an escape, so no cell was written: the column still holds what the last write-through launch left); and the
    first call that looks finds it settled."""
    if WB_AFTER == 0:
        pytest.skip("write-behind never engages in this build")
    n = WB_AFTER + 4
    s = Streak(rg, G, P, n)
    s.ticks(WB_AFTER + 1)  # build + WB_AFTER write-through launches
    s.off.sync()
    through = raw_match(rg, s)
    assert (through == s.off.read_column(rg.COL.MATCH)[:, :G]).all()
    s.ticks(3)
    s.off.sync()
    behind = raw_match(rg, s)
    ref = s.off.read_column(rg.COL.MATCH)[:, :G]
    assert (behind == through).all(), "a write-behind launch stored match cells on a steady stream"
    assert (behind != ref).sum() >= G, int((behind != ref).sum())  # (every group's followers acked in those three ticks)
    streak_stats(s, n)
    assert (s.on.read_column(rg.COL.MATCH)[:, :G] == ref).all()  # settled
    assert (raw_match(rg, s) == ref).all()
    s.compare()
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("G,P", SHAPES)
def test_a_fused_launch_behind_log_term_ticks_of_the_same_call(rg, G, P):
    """ONE rg_tick_device_fused call: WB_AFTER + 2 ticks that carry a log-term column (each runs as a single tick behind its
    pre-pass -- build, WB_AFTER write-through, one write-behind launch) and then a plain tick, which k_tick_fused runs on the
    columns: the call has to settle them in between, there is no entry point left to do it."""
    import torch
    n = WB_AFTER + 3
    assert n <= 8  # RG_MAX_FUSE
    s = Streak(rg, G, P, n)
    logterm = torch.zeros((P, s.on.stride), dtype=torch.int64, device="cuda")  # (no message has RG_MF_HAS_LOGTERM: the column only routes the tick)
    ticks = [s.ptrs(t) + [logterm.data_ptr()] for t in range(n - 1)] + [s.ptrs(n - 1)]
    outs = []
    for e in (s.on, s.off):
        out_t = torch.zeros((n, G), dtype=torch.int32, device="cuda")
        assert e.tick_device_fused(ticks, out_t.data_ptr()) == n
        e.sync()
        outs.append(out_t.cpu().numpy())
    s.t = n
    st = s.on.mirror_stats()
    assert (st["build_launches"], st["packed_launches"], st["valid"]) == (1, WB_AFTER + 1, 0), st
    assert (outs[0] == outs[1]).all()
    s.compare(out=False)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("G,P", SHAPES)
def test_results_between_ticks_neither_settle_nor_end_the_streak(rg, G, P):
    n = WB_AFTER + 6
    s = Streak(rg, G, P, n)
    s.ticks(WB_AFTER + 3)
    for e in (s.on, s.off):
        commit, out = e.results()
        e.result_counts()
        e.sync()
        e.device_info()
        e.read_column(rg.COL.NEXT)
    assert (s.on.results()[0] == s.off.results()[0]).all() and (s.on.results()[1] == s.off.results()[1]).all()
    s.ticks(3)
    streak_stats(s, n)
    s.compare()
    s.close()


@pytest.mark.gpu
def test_streamed_messages_take_the_write_behind_kernel_too(rg):
    """NTM = 1: the policy forced (RG_CACHE_STREAM_MSGS), the second pair of instantiations."""
    n = WB_AFTER + 4
    s = Streak(rg, 193, 5, n, cache_policy=rg.CACHE.STREAM_MSGS)
    s.ticks(n)
    info = s.on.device_info()
    assert info["last_tick_streaming"] == 1 and info["last_tick_kernel"] == rg.KERNEL.NAMES[rg.KERNEL.LANE], info
    streak_stats(s, n)
    s.compare()
    s.close()


@pytest.mark.gpu
def test_the_escape_watch_settles_when_it_goes_back_to_the_plain_kernel(rg):
    """A follower in lane 0 of three of the four waves reports a commit index far above the leader's (committed_index > commit: an
    escape that stays): after RG_MIRROR_WINDOW launches the engine switches to k_tick_lane for good -- behind a settle, because
    the cells of the one steady wave are behind the plane by then."""
    G, P, n = 193, 5, 40

    def plant(st):
        for wave in range(3):
            g = 64 * wave
            w = int(st["cfg"][g])
            slot = next(x for x in range(P) if x != ((w >> 16) & 7) and (w >> (24 + x)) & 1)
            st["pr_commit"][slot, g] = int(st["commit"][g]) + 1_000_000

    s = Streak(rg, G, P, n, plant=plant)
    s.ticks(31)
    s.on.sync()  # (lets the pinned count catch up with the launches, as any host that looks at results does; no settle, no new streak)
    s.ticks(n - 31)
    for e in (s.on, s.off):
        e.sync()
    st = s.on.mirror_stats()
    assert st["off"] == 2 and st["valid"] == 0 and st["build_launches"] == 1 and 31 <= st["packed_launches"] < n - 1, st
    s.compare()
    s.close()


PROBE = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import raft_rs_amd as rg
G, P, K1, M = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), 3
T = K1 + M
side = torch.cuda.Stream()
eng = rg.Engine(G, P, flags=rg.CFGF.NO_SIZE_CLASSES)          # eager write-behind ticks, then captured ones
ref = rg.Engine(G, P, flags=rg.CFGF.NO_SIZE_CLASSES | rg.CFGF.NO_READ_MIRROR)   # the same ticks, all eager
for e in (eng, ref):
    e.set_stream(side.cuda_stream)
    e.workload_init(rg.WL_MAJORITY)
    e.checkpoint()
cols = [torch.empty((T, P, eng.stride), dtype=torch.int64, device="cuda") for _ in range(4)]
flags = torch.empty((T, G, 8), dtype=torch.uint8, device="cuda")
ptrs = lambda t: [c[t].data_ptr() for c in cols] + [flags[t].data_ptr()]
for t in range(T):   # the stream, made once by the reference engine
    ref.workload_gen(rg.WL_MAJORITY, t, *ptrs(t))
    ref.tick_device(*ptrs(t))
ref.restore()
ref.sync()
for t in range(K1):
    eng.tick_device(*ptrs(t))
s = eng.mirror_stats()
assert (s["build_launches"], s["packed_launches"], s["valid"], s["off"]) == (1, K1 - 1, 1, 0), s
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph, stream=side):
    for t in range(K1, T):          # no entry point in between: the first of them finds the columns behind
        eng.tick_device(*ptrs(t))
s = eng.mirror_stats()
assert (s["build_launches"], s["packed_launches"]) == (1, K1 - 1) and s["off"] == 1 and s["valid"] == 0, s
graph.replay()
graph.replay()                      # (the same messages again: stale acks -- the eager engine gets them too)
torch.cuda.synchronize()
for t in range(K1):
    ref.tick_device(*ptrs(t))
for rep in range(2):
    for t in range(K1, T):
        ref.tick_device(*ptrs(t))
ref.sync()
a, b = eng.read_state(), ref.read_state()
for k in ("match", "next", "pr_commit", "commit", "pflags", "term_lo", "term_hi", "cfg", "out"):
    assert np.array_equal(a[k], b[k]), k
ca, cb = eng.results(), ref.results()
assert np.array_equal(ca[0], cb[0]) and np.array_equal(ca[1], cb[1])
graph.replay()                      # ... and once more behind an entry point that has settled: the captured settle is a no-op
torch.cuda.synchronize()
for t in range(K1, T):
    ref.tick_device(*ptrs(t))
ref.sync()
a, b = eng.read_state(), ref.read_state()
for k in ("match", "next", "pr_commit", "commit", "pflags"):
    assert np.array_equal(a[k], b[k]), k
print("MIRROR_WB_GRAPH_OK")
"""


@pytest.mark.gpu
@pytest.mark.parametrize("G,P", [(193, 5), (65, 3)])
def test_ticks_captured_behind_a_write_behind_streak_replay_any_number_of_times(tmp_path, G, P):
    """Modelled on PROBE of tests/test_mirror_gpu.py (torch.cuda.graph drives the capture, in a process of its own): the captured
    settle decodes the plane only when write-behind launches ran since the last settle."""
    script = tmp_path / "mirror_wb_graph_probe.py"
    script.write_text(PROBE)
    r = subprocess.run([sys.executable, str(script), ROOT, str(G), str(P), str(WB_AFTER + 3)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "MIRROR_WB_GRAPH_OK" in r.stdout, r.stdout
