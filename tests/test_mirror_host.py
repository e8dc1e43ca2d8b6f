"""CPU-only: the dense tick's read mirror (raft_rs_amd/csrc/rg_mirror.h) on the host twin tests/host_check/mirror_twin.hip.

(1) the packed word at its edges; (2) two roads over one random stream -- (a) rg_load_group / tick / rg_store_group, (b) build once,
then packed -- leave every column and every result word equal after every tick, and every field of the plane that is not the escape
decodes to its column cell; (3) the share of escaped fields on the benchmark's stream; (4) the rgr_* exports are the header's, bound
and generated."""
import ctypes as C
import copy
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fuzz
import oracle_lib as O
from test_host_check import msg_ptrs, state_ptrs

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_check", "mirror_twin.hip")
LIB = os.path.join(HERE, "host_check", "libmirror_twin.so")
CSRC = os.path.join(ROOT, "raft_rs_amd", "csrc")
MT_ESC, PC_ESC = 0x8000, 0xFFFF
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def twin():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("rg_mirror.h", "rg_group.h", "rg_common.h", "rg_tick_kernels.h", "rg_send.h", "rg_publish.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call([hipcc, "-O3", "-std=c++17", "-shared", "-fPIC", "--offload-arch=gfx950", "-Wno-pass-failed", SRC, "-o", LIB])
    L = C.CDLL(LIB)
    L.rg_mirror_twin_tick.restype = C.c_int
    L.rg_mirror_twin_tick.argtypes = [C.c_uint, C.c_ulong, C.c_ulong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.rg_mirror_twin_encode.restype = C.c_uint
    L.rg_mirror_twin_encode.argtypes = [C.c_ulong] * 3
    for f in (L.rg_mirror_twin_match, L.rg_mirror_twin_prc):
        f.restype = C.c_ulong
        f.argtypes = [C.c_uint, C.c_ulong]
    return L


def model_word(mt, pc, c):
    """The issue's definition, in Python integers: differences in 64-bit wrap-around arithmetic, then range-checked."""
    dm = (mt - c) & M64
    sm = dm - (1 << 64) if dm >> 63 else dm
    lo = (sm & 0xFFFF) if -32767 <= sm <= 32767 else MT_ESC
    dp = (c - pc) & M64
    hi = dp if dp <= 65534 else PC_ESC
    return lo | (hi << 16)


EDGES = (0, 1, 32766, 32767, 32768, 65534, 65535, 65536)
BASES = (0, 1, 70000, (1 << 32) - 1, 1 << 32, (1 << 32) + 70000, (1 << 63) - 1, 1 << 63, M64 - 1, M64)


def test_word_edges(twin):
    seen = set()
    for c in BASES:
        vals = {(c + s * d) & M64 for d in EDGES for s in (1, -1)} | {0, (1 << 32) - 1, 1 << 32, (1 << 63) - 1, M64}
        for mt in vals:
            for pc in vals:
                w = twin.rg_mirror_twin_encode(mt, pc, c)
                assert w == model_word(mt, pc, c), (hex(mt), hex(pc), hex(c), hex(w))
                lo, hi = w & 0xFFFF, w >> 16
                if lo != MT_ESC:
                    assert twin.rg_mirror_twin_match(w, c) == mt
                if hi != PC_ESC:
                    assert twin.rg_mirror_twin_prc(w, c) == pc
                seen.add((lo == MT_ESC, hi == PC_ESC))
    assert len(seen) == 4
    # the last representable and the first escaped value on either side
    assert twin.rg_mirror_twin_encode(100000 + 32767, 100000, 100000) == 0x7FFF
    assert twin.rg_mirror_twin_encode(100000 - 32767, 100000, 100000) == 0x8001
    assert twin.rg_mirror_twin_encode(100000 + 32768, 100000, 100000) & 0xFFFF == MT_ESC
    assert twin.rg_mirror_twin_encode(100000 - 32768, 100000, 100000) & 0xFFFF == MT_ESC
    assert twin.rg_mirror_twin_encode(100000, 100000 - 65534, 100000) >> 16 == 0xFFFE
    assert twin.rg_mirror_twin_encode(100000, 100000 - 65535, 100000) >> 16 == PC_ESC
    assert twin.rg_mirror_twin_encode(100000, 100001, 100000) >> 16 == PC_ESC  # committed_index above commit


def new_plane(st):
    return np.full((st["n_slots"], st["stride"]), 0xDEADBEEF, dtype=np.uint32)  # (never read before a build tick wrote it)


def run(twin, st, msgs, out, pk, mode):
    rc = twin.rg_mirror_twin_tick(st["n_slots"], st["n_groups"], st["stride"], state_ptrs(st, out), msg_ptrs(msgs),
                                  pk.ctypes.data if pk is not None else None, mode)
    assert rc == 0


def check_plane(st, pk):
    """Wherever a field is not the escape the decoded word is the column cell; a slot WITHOUT a Progress holds the word 0 and never
    an escape (no tick looks at what it decodes to). -> (fields, escaped fields, blocks of 64 groups = waves that hold an escape)"""
    G, P = st["n_groups"], st["n_slots"]
    c = st["commit"][:G]
    present = (st["cfg"][:G] >> 24) & 0xFF
    esc = 0
    group_esc = np.zeros(G, dtype=bool)
    for p in range(P):
        w = pk[p, :G].astype(np.uint64)
        lo, hi = w & np.uint64(0xFFFF), w >> np.uint64(16)
        sext = np.where(lo >= 0x8000, lo.astype(np.int64) - 65536, lo.astype(np.int64)).astype(np.uint64)
        dec_mt, dec_pc = c + sext, c - hi  # (uint64 arithmetic wraps)
        has = ((present >> p) & 1).astype(bool)
        assert (w[~has] == 0).all(), (p, np.nonzero(~has & (w != 0))[0][:5])
        ok_mt = ~has | (lo == MT_ESC) | (dec_mt == st["match"][p, :G])
        ok_pc = ~has | (hi == PC_ESC) | (dec_pc == st["pr_commit"][p, :G])
        assert ok_mt.all(), (p, np.nonzero(~ok_mt)[0][:5])
        assert ok_pc.all(), (p, np.nonzero(~ok_pc)[0][:5])
        esc += int((lo == MT_ESC).sum()) + int((hi == PC_ESC).sum())
        group_esc |= (lo == MT_ESC) | (hi == PC_ESC)
    waves = sum(int(group_esc[b:b + 64].any()) for b in range(0, G, 64))
    return 2 * P * G, esc, waves


def plant_edges(rng, st, groups):
    """Groups whose cells sit at the edges of the word: match = commit +- EDGES, committed_index commit - EDGES and ABOVE commit,
    commits at 0, 2^32 - 1, 2^32 and 2^63 - 1 (wrap-around on either side)."""
    P = st["n_slots"]
    commits = [0, 5, (1 << 32) - 1, 1 << 32, (1 << 63) - 1, 3_000_000, 40_000, 65_535]
    for i, g in enumerate(groups):
        c = commits[i % len(commits)]
        st["commit"][g] = c
        hi = max(c, 1) + 70_000 if c < (1 << 62) else c  # last_index at or beyond everything planted below
        st["term_hi"][g] = min(hi, M64)
        st["term_lo"][g] = max(1, c - 3) if c else 1
        for p in range(P):
            d = EDGES[(i // len(commits) + p) % len(EDGES)]
            s = 1 if (i + p) & 1 else -1
            st["match"][p, g] = (c + s * d) & M64
            st["next"][p, g] = (int(st["match"][p, g]) + 1) & M64
            e = EDGES[(i + 2 * p) % len(EDGES)]
            st["pr_commit"][p, g] = (c - e) & M64 if (i + p) % 5 else (c + 1 + e) & M64  # every fifth: above commit


@pytest.mark.parametrize("P", [1, 3, 5, 7, 8])
def test_packed_road_equals_plain_road(twin, P):
    G, T, term = 257, 12, 5
    rng = np.random.default_rng(0xA11CE + P)
    a = O.add_term_table(O.alloc_state(G, P))
    a["cfg"][:] = fuzz.random_cfg(rng, G, P)
    fuzz.random_state(rng, a)
    fuzz.random_term_table(rng, a, term, max_runs=4)
    present = (a["cfg"] >> 24) & 0xFF
    for p in range(P):  # slots without a Progress hold arbitrary garbage in every column
        absent = np.nonzero(((present >> p) & 1) == 0)[0]
        for k in ("match", "next", "pr_commit"):
            a[k][p, absent] = rng.integers(0, 1 << 63, size=len(absent), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        # ... some of it within reach of the commit index
        near = absent[::3]
        a["match"][p, near] = a["commit"][near] + np.uint64(7)
        a["pr_commit"][p, near] = a["commit"][near] - np.minimum(a["commit"][near], np.uint64(3))
    edge_groups = list(range(3, G, 4))
    b = None
    out_a, out_b = np.zeros(G, dtype=np.uint32), np.zeros(G, dtype=np.uint32)
    msgs = O.alloc_msgs(G, P)
    pk = None
    fields = escaped = elected = 0
    seen_lo, seen_hi = set(), set()
    for t in range(T):
        planted = t % 4 == 0
        if planted:  # an outside write: both roads get the same cells, and road (b) rebuilds its plane
            plant_edges(rng, a, edge_groups)
            b = copy.deepcopy(a)
            pk = new_plane(b)
        fuzz.random_msgs(rng, a, msgs, elect_p=0.08, elect_term=term + 1 + t, reject_p=0.2)
        if planted:  # the planted groups sit this tick out, so that the build tick encodes the planted cells themselves
            msgs["m_flags"][edge_groups, :] = 0
        run(twin, a, msgs, out_a, None, 0)
        run(twin, b, msgs, out_b, pk, 1 if planted else 2)
        diffs = fuzz.diff_states(a, b, G, P, present_only=False)
        assert not diffs, (t, diffs[:5])
        assert (out_a == out_b).all(), (t, np.nonzero(out_a != out_b)[0][:5])
        for k in ("run_first", "run_term", "cur_term", "host_hint", "run_count"):
            assert (a[k] == b[k]).all(), (t, k)
        elected += int(((out_a & 0x10) != 0).sum())  # RG_OUT_BECAME_LEADER
        f, e, _ = check_plane(b, pk)
        fields, escaped = fields + f, escaped + e
        if planted:
            seen_lo |= set(np.unique(pk[:, edge_groups] & 0xFFFF).tolist())
            seen_hi |= set(np.unique(pk[:, edge_groups] >> 16).tolist())
    # the stream reached both sides of both edges, and the packed road served escapes from the columns
    assert {0x7FFF, 0x8001, MT_ESC, 0, 1} <= seen_lo and {0xFFFE, PC_ESC, 0, 1} <= seen_hi, (sorted(seen_lo)[:8], sorted(seen_hi)[-4:])
    assert 0 < escaped < fields and elected > 0


def test_escapes_are_rare_on_the_benchmark_stream(twin, rg):
    """The headline stream (workload 2, the benchmark's seed): under 0.1 % of the fields of the plane are escapes, so the packed
    road's dependent loads are noise. Measured: see the assertion message / profiles/mirror.txt."""
    from raft_rs_amd import engine as E
    G, P, T, seed = 4096, 5, 55, 0x5EED5EED
    st = O.alloc_state(G, P)
    E.workload_init_host(st, 2, seed=seed)
    msgs = E.MsgBuffers(G, P, st["stride"])
    out = np.zeros(G, dtype=np.uint32)
    pk = new_plane(st)
    fields = escaped = 0
    for t in range(T):
        E.workload_gen_host(st, msgs, 2, t, seed=seed)
        run(twin, st, msgs.as_dict(), out, pk, 1 if t == 0 else 2)
        f, e, _ = check_plane(st, pk)
        fields, escaped = fields + f, escaped + e
    share = escaped / fields
    print(f"escaped fields: {escaped} of {fields} = {share:.6%}")
    assert share < 0.001, (escaped, fields)


def test_the_mixed_workload_escapes_and_the_engine_is_told(twin, rg):
    """BASELINE config 5 (workload 5, replica sets of 3 / 5 / 7 in a 7-slot engine, leader-term rollover): slots without a Progress
    never escape, but a fresh leader's followers (matched = 0) and probing peers do, and with one such group in most 64-lane waves
    the packed road would re-read the columns nearly everywhere. That is what the engine's escape watch is for (rg_mirror.h:
    RG_MIRROR_WAVE_SHARE -- more than one wave in 8 over a window switches the mirror off): on this stream the share of waves
    that store an escape is far above that bound, on the headline stream (above) it is zero. Results stay equal all the same."""
    from raft_rs_amd import engine as E
    G, P, T, seed = 4096, 7, 40, 0x5EED5EED
    a = O.add_term_table(O.alloc_state(G, P))  # (a table of its own per road: an election writes the current term)
    E.workload_init_host(a, 5, seed=seed)
    b = copy.deepcopy(a)
    msgs = E.MsgBuffers(G, P, a["stride"])
    out_a, out_b = np.zeros(G, dtype=np.uint32), np.zeros(G, dtype=np.uint32)
    pk = new_plane(b)
    fields = escaped = waves = 0
    for t in range(T):
        E.workload_gen_host(a, msgs, 5, t, seed=seed)
        run(twin, a, msgs.as_dict(), out_a, None, 0)
        run(twin, b, msgs.as_dict(), out_b, pk, 1 if t == 0 else 2)
        assert not fuzz.diff_states(a, b, G, P, present_only=False), t
        assert (out_a == out_b).all(), t
        f, e, w = check_plane(b, pk)
        fields, escaped, waves = fields + f, escaped + e, waves + w
    share = waves / (T * (G // 64))
    print(f"workload 5 x 7 slots: escaped fields {escaped} of {fields} = {escaped / fields:.4%}; waves holding an escape {share:.1%}")
    src = open(os.path.join(CSRC, "rg_mirror.h")).read()
    bound = 1 / int(re.search(r"#define RG_MIRROR_WAVE_SHARE (\d+)u", src).group(1))
    assert share > 2 * bound, (share, bound)


def test_mirror_export_is_the_headers(rg):
    """include/raftgroups_mirror.h: its one entry point is exported as an OBJECT holding the function's address (rgr_mirror_stats, the
    only rgr_* symbol), so the library's exported FUNCTIONS are what the older headers declare; it is bound by the Python package
    and named by the generated Rust module; the flag is the header's."""
    from raft_rs_amd import engine as E
    hdr = open(os.path.join(ROOT, "include", "raftgroups_mirror.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert not re.findall(r"\b(rg\w?_\w+)\s*\([^()]*\)\s*;", plain)  # no function prototype
    assert re.findall(r"extern const (\w+) (rgr_\w+);", plain) == [("rgr_mirror_stats_fn", "rgr_mirror_stats")]
    nm = subprocess.run(["nm", "-D", "--defined-only", rg.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    rows = {l.split()[-1]: l.split()[-2] for l in nm.splitlines() if len(l.split()) >= 3}
    assert {k: v for k, v in rows.items() if k.startswith("rgr_")} in ({"rgr_mirror_stats": "D"}, {"rgr_mirror_stats": "R"})
    rs = open(os.path.join(ROOT, "bindings", "raftgroups_mirror.rs")).read()
    assert "pub static rgr_mirror_stats: unsafe extern \"C\" fn(h: *const RgEngine, info: *mut RgrMirrorInfo) -> i32;" in rs
    assert "pub const RGR_MIRROR_VERSION: u32 = %d;" % E.MIRROR_VERSION in rs
    assert C.sizeof(E.MirrorInfo) == 40
    core = open(os.path.join(ROOT, "include", "raftgroups.h")).read()
    assert int(re.search(r"#define RG_CFGF_NO_READ_MIRROR (0x[0-9a-f]+)u", core).group(1), 16) == E.CFGF.NO_READ_MIRROR == 0x8
    lib = rg.load_library()
    info = E.MirrorInfo()
    assert lib.rgr_mirror_stats_fn(None, C.byref(info)) == -1 and b"rgr_mirror_stats" in lib.rg_last_error()
    assert int(re.search(r"#define RGR_MIRROR_VERSION (\d+)u", hdr).group(1)) == E.MIRROR_VERSION
