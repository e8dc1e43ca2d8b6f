"""GPU: the dense tick's read mirror (k_tick_mirror, raft_rs_amd/csrc/rg_mirror.h) against an engine created without it
(RG_CFGF_NO_READ_MIRROR) and against the oracle; every way the mirror is dropped; the launches it must never take."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fuzz
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = (1, 63, 64, 65, 193)
SLOTS = (3, 5, 7)
TERM = 4


def make(rg, G, P, mirror=True, **kw):
    """An engine on the plain lane kernel (no size classes: a small shard of config 5 would otherwise run k_tick_classes)."""
    flags = rg.CFGF.NO_SIZE_CLASSES | (0 if mirror else rg.CFGF.NO_READ_MIRROR)
    eng = rg.Engine(G, P, device=0, flags=flags)
    # 3 and 5 slots: BASELINE config 2; 7 slots: config 5 (replica sets of 3 / 5 / 7 in one engine: absent slots, elections, rejects)
    eng.workload_init(rg.WL_MAJORITY if P < 7 else rg.WL_MIXED, **kw)
    return eng


def workload(rg, P):
    return rg.WL_MAJORITY if P < 7 else rg.WL_MIXED


def oracle_of(st, G):
    cl = O.Cluster(G)
    cl.load_soa(st, term=TERM - 1)
    return cl


def tick_all(rg, engines, cl, st, msgs, gout, P, t, **kw):
    """One tick of the generated stream on every engine and on the oracle; every column and result word compared."""
    from raft_rs_amd import engine as E
    G = st["n_groups"]
    cl.store_soa(st)
    E.workload_gen_host(st, msgs, workload(rg, P), t, **kw)
    for eng in engines:
        eng.tick(msgs)
    cl.tick_soa(msgs.as_dict(), gout)
    cl.store_soa(st)
    for eng in engines:
        got = eng.read_state()
        diffs = fuzz.diff_states(st, got, G, P)
        assert not diffs, (t, diffs[:5])
        assert (got["out"] == gout).all(), t
    if len(engines) == 2:  # ... and the two engines cell for cell, slots without a Progress included
        a, b = engines[0].read_state(), engines[1].read_state()
        assert not fuzz.diff_states(a, b, G, P, present_only=False)
        assert (a["out"] == b["out"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("P", SLOTS)
@pytest.mark.parametrize("G", GROUPS)
def test_packed_ticks_equal_the_plain_engine_and_the_oracle(rg, G, P):
    on, off = make(rg, G, P), make(rg, G, P, mirror=False)
    assert on.mirror_stats()["present"] == 1 and on.mirror_stats()["plane_bytes"] == 4 * P * on.stride
    assert off.mirror_stats() == {"packed_launches": 0, "build_launches": 0, "plane_bytes": 0, "present": 0, "valid": 0, "off": 0}
    st = on.read_state()
    cl = oracle_of(st, G)
    msgs, gout = rg.MsgBuffers(G, P, on.stride), np.zeros(G, dtype=np.uint32)
    for t in range(4):
        tick_all(rg, (on, off), cl, st, msgs, gout, P, t)
        info = on.device_info()
        assert info["last_tick_kernel"] == rg.KERNEL.NAMES[rg.KERNEL.LANE] and info["last_tick_streaming"] == 0
    commit, out = on.results()
    assert (commit == st["commit"]).all()
    s = on.mirror_stats()
    assert (s["build_launches"], s["packed_launches"], s["valid"], s["off"]) == (1, 3, 1, 0), s
    s = off.mirror_stats()
    assert (s["build_launches"], s["packed_launches"]) == (0, 0), s
    on.close()
    off.close()


def follower(st, g):
    """A slot of group g that has a Progress and is not the leader's own."""
    w = int(st["cfg"][g])
    return next(s for s in range(st["n_slots"]) if s != ((w >> 16) & 7) and (w >> (24 + s)) & 1)


def op_write_column(rg, eng, st):
    m = eng.read_column(rg.COL.MATCH)
    m[:, :st["n_groups"]] = np.where(m[:, :st["n_groups"]] > 2, m[:, :st["n_groups"]] - 2, m[:, :st["n_groups"]])
    eng.load_column(rg.COL.MATCH, m)


def op_set_progress(rg, eng, st):
    G = st["n_groups"]
    eng.write_cells([{"group": g, "slot": follower(st, g), "match": int(max(1, int(st["match"][follower(st, g), g]) - 1)), "pr_commit": 0}
                     for g in range(0, G, 2)])


def op_recompute(rg, eng, st):
    eng.recompute()


def op_step_flush(rg, eng, st):
    g = st["n_groups"] - 1
    s = follower(st, g)  # (peer ids are slot + 1; one record of many groups: the sparse road, k_tick_list)
    eng.step(g, s + 1, TERM, int(min(int(st["term_hi"][g]), int(st["match"][s, g]) + 1)))
    eng.flush()


def op_restore(rg, eng, st):
    eng.restore()


def op_conf_change(rg, eng, st):
    w = int(st["cfg"][0])
    self_slot = (w >> 16) & 7
    victim = next(s for s in range(st["n_slots"]) if s != self_slot and (w >> s) & 1)
    eng.set_config(0, w & ~(1 << victim))  # a voter of the incoming majority becomes a learner


def op_progress_event(rg, eng, st):
    from raft_rs_amd import engine as E
    eng.progress_events([(g, follower(st, g), E.EV_UNREACHABLE) for g in range(0, st["n_groups"], 3)])


OPS = {"write_column": op_write_column, "set_progress": op_set_progress, "recompute": op_recompute, "step_flush": op_step_flush,
       "restore": op_restore, "conf_change": op_conf_change, "progress_event": op_progress_event}


@pytest.mark.gpu
@pytest.mark.parametrize("G,P", [(193, 5), (65, 3), (64, 7), (63, 5)])
def test_every_outside_write_drops_the_mirror(rg, G, P):
    """Between packed ticks, one each of the calls that change what the plane caches (or might): the next tick is a build tick, and it
    computes from the columns as they stand -- the oracle, reloaded from the engine's columns after the call, agrees cell for cell."""
    eng = make(rg, G, P)
    for g in range(G):  # the host mirror of RawNode::step (peer ids 1..P in slot order) for the step + flush case
        eng.set_peers(g, list(range(1, P + 1)), TERM)
    st = eng.read_state()
    cl = oracle_of(st, G)
    msgs, gout = rg.MsgBuffers(G, P, eng.stride), np.zeros(G, dtype=np.uint32)
    t = 0
    for _ in range(2):
        tick_all(rg, (eng,), cl, st, msgs, gout, P, t)
        t += 1
    eng.checkpoint()  # (an entry point like any other: the tick behind it builds)
    tick_all(rg, (eng,), cl, st, msgs, gout, P, t)
    t += 1
    s0 = eng.mirror_stats()
    assert (s0["build_launches"], s0["packed_launches"]) == (2, 1), s0
    for name, op in OPS.items():
        tick_all(rg, (eng,), cl, st, msgs, gout, P, t)  # a packed tick in front of every call
        t += 1
        before = eng.mirror_stats()
        assert before["valid"] == 1 and before["packed_launches"] == s0["packed_launches"] + 1, (name, before)
        op(rg, eng, st)
        assert eng.mirror_stats()["valid"] == 0, name
        st = eng.read_state()
        cl = oracle_of(st, G)
        tick_all(rg, (eng,), cl, st, msgs, gout, P, t)
        t += 1
        s1 = eng.mirror_stats()
        assert (s1["build_launches"], s1["packed_launches"]) == (s0["build_launches"] + 1, before["packed_launches"]), (name, s0, s1)
        s0 = s1
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("G,P", [(193, 5), (65, 7), (1, 3)])
def test_read_only_calls_keep_the_mirror(rg, G, P):
    eng = make(rg, G, P)
    st = eng.read_state()
    cl = oracle_of(st, G)
    msgs, gout = rg.MsgBuffers(G, P, eng.stride), np.zeros(G, dtype=np.uint32)
    tick_all(rg, (eng,), cl, st, msgs, gout, P, 0)
    eng.results()
    eng.result_counts()
    eng.sync()
    eng.device_info()
    eng.read_column(rg.COL.NEXT)
    assert eng.mirror_stats()["valid"] == 1
    tick_all(rg, (eng,), cl, st, msgs, gout, P, 1)
    assert eng.mirror_stats()["packed_launches"] == 1
    eng.column_ptr(rg.COL.NEXT)
    assert eng.mirror_stats()["off"] == 0
    eng.column_ptr(rg.COL.MATCH)  # whoever holds this pointer writes the column without an entry point: off for good
    s = eng.mirror_stats()
    assert s["off"] == 1 and s["valid"] == 0
    tick_all(rg, (eng,), cl, st, msgs, gout, P, 2)
    s = eng.mirror_stats()
    assert (s["build_launches"], s["packed_launches"]) == (1, 1), s
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("G,P", [(193, 5), (64, 3), (65, 7)])
def test_group_commit_never_takes_the_mirror_kernel(rg, G, P):
    eng = make(rg, G, P)
    st = eng.read_state()
    w = int(st["cfg"][G // 2]) | 0x80000  # RG_CFG_GROUP_COMMIT on in ONE group
    eng.set_config(G // 2, w)
    st = eng.read_state()
    cl = oracle_of(st, G)
    msgs, gout = rg.MsgBuffers(G, P, eng.stride), np.zeros(G, dtype=np.uint32)
    for t in range(3):
        tick_all(rg, (eng,), cl, st, msgs, gout, P, t)
    s = eng.mirror_stats()
    assert s["present"] == 1 and (s["build_launches"], s["packed_launches"], s["valid"]) == (0, 0, 0), s
    eng.close()


@pytest.mark.gpu
def test_a_shard_whose_waves_escape_goes_back_to_the_plain_kernel(rg):
    """Config 5 in one 7-slot engine: most waves hold a fresh leader's follower or a probing peer, i.e. an escape. The engine's
    escape watch (a count the kernel keeps, read without a synchronisation every 32 mirror launches) switches the mirror off for
    good: rgr_mirror_info.off bit 1, no packed launch afterwards, and the columns equal a mirror-less engine's throughout."""
    import torch
    G, P, K = 4096, 7, 100
    on, off = make(rg, G, P), make(rg, G, P, mirror=False)
    cols = [torch.empty((P, on.stride), dtype=torch.int64, device="cuda") for _ in range(4)]
    flags = torch.empty((G, 8), dtype=torch.uint8, device="cuda")
    ptrs = [c.data_ptr() for c in cols] + [flags.data_ptr()]
    for t in range(K):
        on.workload_gen(rg.WL_MIXED, t, *ptrs)
        on.tick_device(*ptrs)
        off.tick_device(*ptrs)
        if t % 33 == 32:
            on.sync()  # (lets the pinned count catch up with the launches, as any host that looks at results does)
    on.sync()
    off.sync()
    s = on.mirror_stats()
    assert s["off"] == 2 and s["valid"] == 0 and s["build_launches"] == 1 and 31 <= s["packed_launches"] < K - 1, s
    a, b = on.read_state(), off.read_state()
    assert not fuzz.diff_states(a, b, G, P, present_only=False)
    assert (a["out"] == b["out"]).all()
    on.close()
    off.close()


PROBE = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import raft_rs_amd as rg
G, P, K = int(sys.argv[2]), int(sys.argv[3]), 6
side = torch.cuda.Stream()
eng = rg.Engine(G, P, flags=rg.CFGF.NO_SIZE_CLASSES)
eng.set_stream(side.cuda_stream)
eng.workload_init(rg.WL_MAJORITY)
cols = [torch.empty((K, P, eng.stride), dtype=torch.int64, device="cuda") for _ in range(4)]
flags = torch.empty((K, G, 8), dtype=torch.uint8, device="cuda")
ptrs = lambda t: [c[t].data_ptr() for c in cols] + [flags[t].data_ptr()]
eng.checkpoint()
for t in range(K):
    eng.workload_gen(rg.WL_MAJORITY, t, *ptrs(t))
    eng.tick_device(*ptrs(t))
eng.sync()
ref, ref_state = eng.results(), eng.read_state()
s = eng.mirror_stats()
assert (s["build_launches"], s["packed_launches"]) == (1, K - 1), s   # eager: the generator keeps the mirror
eng.restore()
eng.sync()
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph, stream=side):
    for t in range(K):
        eng.tick_device(*ptrs(t))
s2 = eng.mirror_stats()
assert (s2["build_launches"], s2["packed_launches"]) == (1, K - 1) and s2["off"] == 1 and s2["valid"] == 0, s2   # captured: never
for rep in range(2):   # the graph replays behind the engine's back: every launch in it must stand on the columns alone
    eng.restore()
    eng.sync()
    graph.replay()
    torch.cuda.synchronize()
    c, o = eng.results()
    assert np.array_equal(c, ref[0]) and np.array_equal(o, ref[1])
    st = eng.read_state()
    for k in ("match", "next", "pr_commit", "commit", "pflags"):
        assert np.array_equal(st[k], ref_state[k]), k
for t in range(2):   # ... and an eager tick afterwards stays off the mirror for good
    eng.tick_device(*ptrs(t))
eng.sync()
s3 = eng.mirror_stats()
assert (s3["build_launches"], s3["packed_launches"]) == (1, K - 1), s3
print("MIRROR_GRAPH_OK")
"""


@pytest.mark.gpu
@pytest.mark.parametrize("G,P", [(193, 5), (65, 3)])
def test_captured_ticks_never_take_the_mirror_kernel(tmp_path, G, P):
    """The approach of tests/test_graph_capture_gpu.py (torch.cuda.graph drives the capture, in a process of its own): a captured
    tick runs k_tick_lane, and because the graph can be replayed without any entry point the mirror is off for good afterwards."""
    script = tmp_path / "mirror_graph_probe.py"
    script.write_text(PROBE)
    r = subprocess.run([sys.executable, str(script), ROOT, str(G), str(P)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "MIRROR_GRAPH_OK" in r.stdout, r.stdout
