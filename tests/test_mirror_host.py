"""CPU-only: the dense tick's read mirror (raft_rs_amd/csrc/rg_mirror.h) on the host twin tests/host_check/mirror_twin.hip.

(1) the packed word at its edges; (2) two roads over one random stream -- (a) rg_load_group / tick / rg_store_group, (b) build once,
then packed -- leave every column and every result word equal after every tick, and every field of the plane that is not the escape
decodes to its column cell; (3) the share of escaped fields on the benchmark's stream; (4) the rgr_* exports are the header's, bound
and generated; (5) the same roads with the twin's WAVE mode, in which a block of 64 groups takes the escape branch together as
the wave does on the device, and ONE escaping lane in a steady wave (readmirror.plant_wave) in both modes; (6) a word wrong by
one, in the slot that decides the commit index or in an acker's committed_index, shows in the columns: the packed tick computes
on the plane. The helpers shared with the GPU tests live in tests/readmirror.py."""
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
from readmirror import (EDGES, KINDS, M64, MT_ESC, PC_ESC, check_plane, deciding_acks, model_word, new_plane, plant_edges,
                        plant_wave, wave_groups)
from test_host_check import msg_ptrs, state_ptrs

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_check", "mirror_twin.hip")
LIB = os.path.join(HERE, "host_check", "libmirror_twin.so")
CSRC = os.path.join(ROOT, "raft_rs_amd", "csrc")


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


def run(twin, st, msgs, out, pk, mode):
    rc = twin.rg_mirror_twin_tick(st["n_slots"], st["n_groups"], st["stride"], state_ptrs(st, out), msg_ptrs(msgs),
                                  pk.ctypes.data if pk is not None else None, mode)
    assert rc == 0


@pytest.mark.parametrize("P", [1, 3, 5, 7, 8])
def test_packed_road_equals_plain_road(twin, P):
    packed_road_equals_plain_road(twin, P, 2)


def packed_road_equals_plain_road(twin, P, packed_mode):
    """packed_mode 2: every lane decides the escape branch for itself; 3: the block of 64 groups does (the device's wave)."""
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
        run(twin, b, msgs, out_b, pk, 1 if planted else packed_mode)
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


# ---- the device's wave semantics on the twin; one escaping lane; the comparison reads the plane ------------------------------
@pytest.mark.parametrize("P", [1, 3, 5, 7, 8])
def test_packed_road_equals_plain_road_decided_by_the_wave(twin, P):
    """The same two roads with the twin's WAVE mode: a block of 64 consecutive groups takes the escape branch of rg_load_group_pk
    together, as the wave does on the device (a lane without an escape then re-reads its cells because a neighbour has one)."""
    packed_road_equals_plain_road(twin, P, 3)


def steady_shard(rng, G, P, term):
    """Every wave steady (readmirror.plant_wave): the state the one-lane and the corrupted-plane tests start from."""
    st = O.add_term_table(O.alloc_state(G, P))
    st["cfg"][:] = fuzz.random_cfg(rng, G, P, transfer_frac=0.0)
    fuzz.random_state(rng, st)
    for w in range((G + 63) // 64):
        plant_wave(st, w, (), "mt_hi")
    fuzz.random_term_table(rng, st, term, max_runs=4)
    return st


def silence(msgs):
    msgs["m_flags"][...] = 0
    return msgs


@pytest.mark.parametrize("packed_mode", [2, 3])
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("P", [3, 5, 7])
def test_one_escaping_lane_in_a_steady_wave(twin, P, kind, packed_mode):
    """plant_wave: lanes {0}, {31}, {63}, {0, 63} of the first, a middle and the (partial) tail wave hold one escaping field, every
    other group of the shard is steady. Build tick without messages, a packed tick in which a silent voter's cell decides the
    commit index of every group of the planted wave and of one steady wave, two random ticks -- against the plain road."""
    term = 5
    for G, wave, lanes in ((257 + 64, 0, (0,)), (257 + 64, 2, (31,)), (257 + 64, 5, (0,)), (129, 1, (63,)), (129, 2, (0,)),
                           (65, 1, (0,)), (63, 0, (0, 62)), (257 + 64, 3, (0, 63)), (1, 0, (0,)), (63, 0, (31,)), (100, 1, (31,)), (100, 1, (0, 35)),
                           (128, 1, (0, 63)), (128, 1, (63,)), (257 + 64, 0, (0, 63))):
        rng = np.random.default_rng(G * 100 + wave * 10 + P)
        a = steady_shard(rng, G, P, term)
        planted = plant_wave(a, wave, lanes, kind)
        assert len(planted) == len(lanes)
        b = copy.deepcopy(a)
        pk = new_plane(b)
        msgs = silence(O.alloc_msgs(G, P))
        out_a, out_b = np.zeros(G, dtype=np.uint32), np.zeros(G, dtype=np.uint32)
        steady = (wave + 1) % ((G + 63) // 64)
        decided = 0
        for t in range(4):
            if t == 1:
                listed = sorted(set(wave_groups(a, wave)) | set(wave_groups(a, steady)))
                decided = len(deciding_acks(a, msgs, listed))
                before = a["commit"].copy()
            elif t > 1:
                fuzz.random_msgs(rng, a, msgs, elect_p=0.05, elect_term=term + t, reject_p=0.2)
            run(twin, a, msgs, out_a, None, 0)
            run(twin, b, msgs, out_b, pk, 1 if t == 0 else packed_mode)
            diffs = fuzz.diff_states(a, b, G, P, present_only=False)
            assert not diffs, (G, wave, lanes, t, diffs[:5])
            assert (out_a == out_b).all(), (G, wave, lanes, t)
            _, esc, waves = check_plane(b, pk)
            if t == 0:  # exactly the planted fields escape, in exactly one wave
                assert (esc, waves) == (len(lanes), 1), (G, wave, lanes, esc, waves)
                for g, p in planted:
                    w = int(pk[p, g])
                    assert ((w & 0xFFFF) == MT_ESC) != ((w >> 16) == PC_ESC)
            if t == 1:
                moved = int((a["commit"] > before).sum())
                assert moved == decided and (decided >= len(listed) // 4 or G == 1), (G, wave, decided, len(listed))


def corrupt(pk, cells, field, delta):
    """delta added to the low (0) or high (1) field of the listed (group, slot) words, where neither the old nor the new field
    is the escape and the field does not wrap. -> the cells that were changed."""
    done = []
    for g, s in cells:
        w = int(pk[s, g])
        lo, hi = w & 0xFFFF, w >> 16
        if field == 0:
            new = (lo + delta) & 0xFFFF
            if MT_ESC in (lo, new):
                continue
            pk[s, g] = new | (hi << 16)
        else:
            new = hi + delta
            if PC_ESC in (hi, new) or not 0 <= new < PC_ESC:
                continue
            pk[s, g] = lo | (new << 16)
        done.append((g, s))
    return done


def groups_that_differ(a, b, G, P):
    bad = np.zeros(G, dtype=bool)
    for k in fuzz.STATE_KEYS:
        x, y = a[k], b[k]
        if k == "pflags":
            bad |= (x[:G, :P] != y[:G, :P]).any(axis=1)
        elif x.ndim == 2:
            bad |= (x[:P, :G] != y[:P, :G]).any(axis=0)
        else:
            bad |= x[:G] != y[:G]
    return bad


@pytest.mark.parametrize("packed_mode", [2, 3])
@pytest.mark.parametrize("P", [2, 3, 5, 7, 8])
def test_a_corrupted_word_changes_what_the_tick_commits(twin, P, packed_mode):
    """The packed tick COMPUTES on the plane: after a build tick, the word of the slot whose `matched` decides the commit index
    (readmirror.deciding_acks) gets 1 added to, or taken from, its low field in half of the groups. Every such group then
    commits something else than the plain road, no other group differs in any column. This is what makes a comparison of a
    packed tick under deciding_acks meaningful: a wrongly decoded cell of a silent slot shows in `commit`."""
    G, term = 257, 5
    for delta in (1, -1):
        rng = np.random.default_rng(0xC0 + P)
        a = steady_shard(rng, G, P, term)
        b = copy.deepcopy(a)
        pk = new_plane(b)
        msgs = silence(O.alloc_msgs(G, P))
        out_a, out_b = np.zeros(G, dtype=np.uint32), np.zeros(G, dtype=np.uint32)
        run(twin, a, msgs, out_a, None, 0)
        run(twin, b, msgs, out_b, pk, 1)
        decided = deciding_acks(a, msgs, range(G))
        assert len(decided) >= G // 8, len(decided)  # (a floor on the construction: at two slots most groups have ONE voter)
        hit = corrupt(pk, decided[::2], 0, delta)
        assert len(hit) == len(decided[::2])  # (steady cells: no field near the escape)
        run(twin, a, msgs, out_a, None, 0)
        run(twin, b, msgs, out_b, pk, packed_mode)
        bad = groups_that_differ(a, b, G, P)
        hit_g = np.zeros(G, dtype=bool)
        hit_g[[g for g, _ in hit]] = True
        assert (a["commit"][hit_g] != b["commit"][hit_g]).all(), np.nonzero(hit_g & (a["commit"] == b["commit"]))[0][:5]
        assert not (bad & ~hit_g).any(), np.nonzero(bad & ~hit_g)[0][:5]
        assert (a["commit"][[g for g, _ in decided]] == [a["match"][s, g] for g, s in decided]).all()


@pytest.mark.parametrize("packed_mode", [2, 3])
@pytest.mark.parametrize("P", [2, 3, 5, 7, 8])
def test_a_corrupted_committed_index_reaches_its_column(twin, P, packed_mode):
    """The high field (commit - committed_index), in the words of the ACKERS of deciding_acks, 1 taken from it or added to it in
    half of the groups.

    Observable, and asserted for every corrupted cell and no other: the acks carry a Message.commit that is not above the
    acker's committed_index (0). Progress::update_committed then changes nothing, and since the tick rewrites the cells of every
    slot that had an event from its registers (RG_OPT_UNCOND_ST, the default build: whole lines instead of lane-masked stores),
    the decoded value itself lands in RG_COL_PR_COMMIT: one above or one below the plain road's cell.

    UNOBSERVABLE by the tick's arithmetic, named here and asserted as such so that the claim is checked rather than believed:
    the construction with Message.commit exactly one above the true committed_index. Decoded one higher, update_committed finds
    nothing to do -- but the store is NOT skipped, the slot had an event and is rewritten unconditionally with the decoded value,
    which is Message.commit, the right value. Decoded one lower, update_committed is a maximum and stores Message.commit. More
    generally a wrong committed_index below Message.commit never shows, and one of a slot WITHOUT an event is neither compared
    with anything nor stored (the leader's own cell is raised to the new commit index, which is above every representable
    committed_index): only a slot with an event whose Message.commit does not cover the error carries it into the column."""
    G, term = 257, 5
    for delta, above in ((-1, False), (1, False), (-1, True), (1, True)):
        rng = np.random.default_rng(0xC1 + P)
        a = steady_shard(rng, G, P, term)
        b = copy.deepcopy(a)
        pk = new_plane(b)
        msgs = silence(O.alloc_msgs(G, P))
        out_a, out_b = np.zeros(G, dtype=np.uint32), np.zeros(G, dtype=np.uint32)
        run(twin, a, msgs, out_a, None, 0)
        run(twin, b, msgs, out_b, pk, 1)
        decided = deciding_acks(a, msgs, range(G), m_commit_above=above)
        assert len(decided) >= G // 8
        ackers = [(g, s) for g, _ in decided[::2] for s in range(P) if msgs["m_flags"][g, s]]
        hit = corrupt(pk, ackers, 1, delta)
        assert len(hit) >= (3 * len(ackers)) // 4  # (committed_index == commit, field 0, cannot be reduced: 1 cell in 201)
        run(twin, a, msgs, out_a, None, 0)
        run(twin, b, msgs, out_b, pk, packed_mode)
        cell = np.zeros((P, a["stride"]), dtype=bool)
        for g, s in hit:
            cell[s, g] = True
        differs = a["pr_commit"] != b["pr_commit"]
        if above:
            assert not differs.any(), (delta, np.argwhere(differs)[:5])
        else:
            assert (differs == cell).all(), (delta, np.argwhere(differs != cell)[:5])
            assert all(int(b["pr_commit"][s, g]) == int(a["pr_commit"][s, g]) - delta for g, s in hit)
        a["pr_commit"][cell] = b["pr_commit"][cell]
        assert not fuzz.diff_states(a, b, G, P, present_only=False)
        assert (out_a == out_b).all()
