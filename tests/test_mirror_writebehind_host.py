"""CPU-only: the WRITE-BEHIND road of the dense tick's read mirror (raft_rs_amd/csrc/rg_mirror.h: k_tick_mirror_wb stores the packed
words and no longer the match / committed_index cells, k_mirror_settle writes the two columns back from the plane) as the host twin
tests/host_check/mirror_wb_twin.hip runs it, against the plain road; and the host state machine (rg_mirror_host.h), compiled alone."""
import copy
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fuzz
import oracle_lib as O
from readmirror import KINDS, MF_VALID, MT_ESC, PC_ESC, WAVE_COMMIT, absent_garbage, check_plane, new_plane, plant_wave
from test_host_check import msg_ptrs, state_ptrs

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "raft_rs_amd", "csrc")
SRC = os.path.join(HERE, "host_check", "mirror_wb_twin.hip")
LIB = os.path.join(HERE, "host_check", "libmirror_wb_twin.so")
STATE_SRC = os.path.join(HERE, "host_check", "mirror_wb_state.cpp")
STATE_BIN = os.path.join(HERE, "host_check", "mirror_wb_state")
WB_AFTER = int(re.search(r"#define RG_MIRROR_WB_AFTER (\d+)", open(os.path.join(CSRC, "rg_mirror_host.h")).read()).group(1))
PLAIN, BUILD, PACKED, PACKED_WB = 0, 1, 2, 3


@pytest.fixture(scope="module")
def twin():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("rg_mirror.h", "rg_mirror_host.h", "rg_group.h", "rg_common.h", "rg_tick_kernels.h", "rg_send.h", "rg_publish.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call([hipcc, "-O3", "-std=c++17", "-shared", "-fPIC", "--offload-arch=gfx950", "-Wno-pass-failed", SRC, "-o", LIB])
    L = C.CDLL(LIB)
    L.rg_mirror_wb_twin_tick.restype = C.c_int
    L.rg_mirror_wb_twin_tick.argtypes = [C.c_uint, C.c_ulong, C.c_ulong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint]
    L.rg_mirror_wb_twin_settle.restype = C.c_int
    L.rg_mirror_wb_twin_settle.argtypes = [C.c_uint, C.c_ulong, C.c_ulong, C.c_void_p, C.c_void_p, C.c_uint]
    return L


def run(twin, st, msgs, out, pk, mode, lanes=64):
    rc = twin.rg_mirror_wb_twin_tick(st["n_slots"], st["n_groups"], st["stride"], state_ptrs(st, out), msg_ptrs(msgs),
                                     pk.ctypes.data if pk is not None else None, mode, lanes)
    assert rc == 0


def settle(twin, st, out, pk, lanes=64):
    assert twin.rg_mirror_wb_twin_settle(st["n_slots"], st["n_groups"], st["stride"], state_ptrs(st, out), pk.ctypes.data, lanes) == 0


NOT_BEHIND = ("next", "pend_snap", "pend_rs", "pflags", "commit", "term_lo", "term_hi", "cfg", "run_first", "run_term", "cur_term",
              "host_hint", "run_count")


def same_but_the_two_columns(a, b, out_a, out_b, where):
    """Everything a write-behind launch still stores equals the plain road's after every tick."""
    for k in NOT_BEHIND:
        assert (a[k] == b[k]).all(), (where, k)
    assert (out_a == out_b).all(), (where, np.nonzero(out_a != out_b)[0][:5])


def same_state(a, b, out_a, out_b, where):
    G, P = a["n_groups"], a["n_slots"]
    diffs = fuzz.diff_states(a, b, G, P, present_only=False)
    assert not diffs, (where, diffs[:5])
    same_but_the_two_columns(a, b, out_a, out_b, where)


# ---- the base sequence ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [1, 64])
@pytest.mark.parametrize("G", [1, 63, 64, 65, 193])
@pytest.mark.parametrize("P", [1, 3, 5, 7, 8])
def test_a_streak_then_a_settle_equals_the_plain_road(twin, P, G, lanes):
    """build, WB_AFTER write-through ticks, 3 write-behind ticks, settle: the columns equal the plain road's bit for bit, slots
    without a Progress (which hold garbage) included. Random state and stream: escapes, elections and rejects in most waves."""
    term = 5
    rng = np.random.default_rng(0xBE41 + 1000 * P + G)
    a = O.add_term_table(O.alloc_state(G, P))
    a["cfg"][:] = fuzz.random_cfg(rng, G, P)
    fuzz.random_state(rng, a)
    fuzz.random_term_table(rng, a, term, max_runs=4)
    absent_garbage(rng, a)
    b = copy.deepcopy(a)
    pk = new_plane(b)
    out_a, out_b = np.zeros(G, dtype=np.uint32), np.zeros(G, dtype=np.uint32)
    msgs = O.alloc_msgs(G, P)
    modes = [BUILD] + [PACKED] * max(WB_AFTER, 1) + [PACKED_WB] * 3
    behind = 0
    for t, mode in enumerate(modes):
        fuzz.random_msgs(rng, a, msgs, elect_p=0.05, elect_term=term + 1 + t, reject_p=0.2)
        run(twin, a, msgs, out_a, None, PLAIN, lanes)
        run(twin, b, msgs, out_b, pk, mode, lanes)
        if mode == PACKED_WB:
            same_but_the_two_columns(a, b, out_a, out_b, (t, mode))
            behind += int((a["match"] != b["match"]).sum()) + int((a["pr_commit"] != b["pr_commit"]).sum())
        else:
            same_state(a, b, out_a, out_b, (t, mode))
    settle(twin, b, out_b, pk, lanes)
    same_state(a, b, out_a, out_b, "settled")
    check_plane(b, pk)
    settle(twin, b, out_b, pk, lanes)  # (idempotent)
    same_state(a, b, out_a, out_b, "settled twice")


def test_write_behind_leaves_cells_behind(twin):
    """The point of it: on a steady shard the write-behind ticks store no match / committed_index cell at all."""
    G, P, term = 193, 5, 5
    rng = np.random.default_rng(77)
    a, _ = steady(rng, G, P, term)
    b = copy.deepcopy(a)
    pk = new_plane(b)
    out_a, out_b = np.zeros(G, dtype=np.uint32), np.zeros(G, dtype=np.uint32)
    msgs = O.alloc_msgs(G, P)
    for t, mode in enumerate([BUILD, PACKED, PACKED_WB, PACKED_WB]):
        acks(a, msgs, {g: {s: (300 * (t + 1), 300 * t) for s in range(1, P)} for g in range(G)})
        before = (b["match"].copy(), b["pr_commit"].copy())
        run(twin, a, msgs, out_a, None, PLAIN)
        run(twin, b, msgs, out_b, pk, mode)
        if mode == PACKED_WB:
            assert (b["match"] == before[0]).all() and (b["pr_commit"] == before[1]).all()
            assert (a["match"][1:, :G] != b["match"][1:, :G]).all()
            assert check_plane_words_only(pk, G) == 0
    settle(twin, b, out_b, pk)
    same_state(a, b, out_a, out_b, "settled")


def check_plane_words_only(pk, G):
    w = pk[:, :G]
    return int(((w & 0xFFFF) == MT_ESC).sum() + ((w >> 16) == PC_ESC).sum())


# ---- escape transitions --------------------------------------------------------------------------------------------------------
def steady(rng, G, P, term):
    """Every group: all P slots voters with a Progress, the leader in slot 0, steady as readmirror.plant_wave leaves a wave.
    -> (state, commit index per group at the start)"""
    st = O.add_term_table(O.alloc_state(G, P))
    m = (1 << P) - 1
    st["cfg"][:G] = (m << 24) | m
    fuzz.random_state(rng, st)
    for w in range((G + 63) // 64):
        plant_wave(st, w, (), "mt_hi")
    fuzz.random_term_table(rng, st, term, max_runs=4)
    return st, st["commit"][:G].astype(np.uint64).copy()


def acks(st, msgs, per_group):
    """per_group: {group: {slot: (index - c0, Message.commit - c0)}} relative to WAVE_COMMIT's per-group base; silence elsewhere."""
    msgs["m_flags"][...] = 0
    for g, slots in per_group.items():
        c0 = WAVE_COMMIT + 1009 * (g // 64) + 17 * (g % 64)
        for s, (di, dc) in slots.items():
            msgs["m_flags"][g, s] = MF_VALID
            msgs["m_index"][s, g] = c0 + di
            msgs["m_commit"][s, g] = c0 + dc if dc is not None else 0
            msgs["m_hint"][s, g] = msgs["m_rs"][s, g] = 0
            if "m_logterm" in msgs:
                msgs["m_logterm"][s, g] = 0


def transition_plan(kind, P):
    """(cells planted in the focus group relative to its commit index c: {(column, slot): offset}, the messages of the tick in
    which follower 1's field crosses into the escape, of the tick that brings it back) -- slot 0 is the leader, 1 the follower
    whose word escapes, the rest the other followers. Worked out on ProgressTracker's majority: see the comments."""
    others = range(2, P)
    if kind == "mt_hi":  # the follower acks far ahead of the quorum; then the quorum catches up to within 32 767 of it
        return ({("match", 0): 600}, {1: (34000, None)}, {s: (3000, None) for s in others})
    if kind == "mt_lo":  # a lagging follower; the quorum (leader + the others) moves the commit index away; then it catches up
        return ({("match", 0): 5000, ("match", 1): -32000}, {s: (3000, None) for s in others}, {1: (3000, None)})
    if kind == "pc":  # a follower whose committed_index lags by 65 000; the commit index moves on; then the follower reports it
        return ({("match", 0): 5000, ("pr_commit", 1): -65000}, {s: (3000, None) for s in others}, {1: (3000, 3000)})
    if kind == "pc_above":  # the follower reports a commit index the leader has not reached; then the leader reaches it
        return ({("match", 0): 600}, {1: (300, 5000)}, {s: (6000, None) for s in range(1, P)})
    raise AssertionError(kind)


def field_escaped(pk, kind, g, s=1):
    w = int(pk[s, g])
    return (w & 0xFFFF) == MT_ESC if kind.startswith("mt") else (w >> 16) == PC_ESC


def wave_escapes(pk, G, wave, width=64):
    w = pk[:, width * wave:min(G, width * wave + width)]
    return int(((w & 0xFFFF) == MT_ESC).sum() + ((w >> 16) == PC_ESC).sum())


def transitions(twin, P, kind, lanes, upto="end", G=193):
    """Steady shard; focus groups: lane 17 of wave 1 and the one lane of the tail wave. build + WB_AFTER silent write-through ticks,
    then write-behind: CROSS (the field escapes), STAY (silence), BACK (it is representable again), one random tick; settle."""
    term = 5
    rng = np.random.default_rng(0x7E57 + P)
    a, c0 = steady(rng, G, P, term)
    focus = [64 + 17, G - 1]
    plant, cross, back = transition_plan(kind, P)
    for g in focus:
        for (col, s), off in plant.items():
            a[col][s, g] = int(c0[g]) + off
            if col == "match":
                a["next"][s, g] = int(c0[g]) + off + 1
    b = copy.deepcopy(a)
    pk = new_plane(b)
    out_a, out_b = np.zeros(G, dtype=np.uint32), np.zeros(G, dtype=np.uint32)
    msgs = O.alloc_msgs(G, P)

    def tick(mode, per_group=None, random=False):
        if random:
            fuzz.random_msgs(rng, a, msgs, elect_p=0.05, elect_term=term + 3, reject_p=0.2)
        else:
            acks(a, msgs, per_group or {})
        run(twin, a, msgs, out_a, None, PLAIN, lanes)
        run(twin, b, msgs, out_b, pk, mode, lanes)
        same_but_the_two_columns(a, b, out_a, out_b, (kind, mode))

    tick(BUILD)
    for _ in range(max(WB_AFTER, 1)):
        tick(PACKED)
    same_state(a, b, out_a, out_b, "write-through")
    assert check_plane_words_only(pk, G) == 0
    tick(PACKED_WB, {g: cross for g in focus})
    for g in focus:
        assert field_escaped(pk, kind, g), (kind, g, hex(int(pk[1, g])))
        assert wave_escapes(pk, G, g // 64) == 1
    # the invariant: a block that stores an escape stores the cells of all its slots with a Progress (here: every slot)
    for g in focus:
        blk = slice(g, g + 1) if lanes == 1 else slice(64 * (g // 64), min(G, 64 * (g // 64) + 64))
        assert (a["match"][:, blk] == b["match"][:, blk]).all() and (a["pr_commit"][:, blk] == b["pr_commit"][:, blk]).all(), (kind, g)
    if upto == "cross":
        return a, b, pk, out_a, out_b, focus
    tick(PACKED_WB)  # it stays escaped: the loader's escape branch re-reads the block's cells
    for g in focus:
        assert field_escaped(pk, kind, g), (kind, g)
    tick(PACKED_WB, {g: back for g in focus})
    for g in focus:
        assert wave_escapes(pk, G, g // 64) == 0, (kind, g, [hex(int(x)) for x in pk[:, g]])
    tick(PACKED_WB)
    tick(PACKED_WB, random=True)
    settle(twin, b, out_b, pk, lanes)
    same_state(a, b, out_a, out_b, (kind, "settled"))
    check_plane(b, pk)


@pytest.mark.parametrize("lanes", [1, 64])
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("P", [3, 5])
def test_a_lane_crosses_into_an_escape_stays_and_comes_back(twin, P, kind, lanes):
    transitions(twin, P, kind, lanes)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_the_settle_skips_a_block_that_holds_an_escape_and_no_other(twin, kind):
    """Poisoned match / committed_index cells: in a block without an escape the settle overwrites them with the decoded words, in
    the block whose words hold one it touches nothing (its cells are current; here the poison stays)."""
    P, G = 5, 193
    a, b, pk, out_a, out_b, focus = transitions(twin, P, kind, 64, upto="cross", G=G)
    poison = np.uint64(0xDEAD0000DEAD)
    for col in ("match", "pr_commit"):
        b[col][:, :G] = poison
    settle(twin, b, out_b, pk, 64)
    for wave in range((G + 63) // 64):
        blk = slice(64 * wave, min(G, 64 * wave + 64))
        escaped = wave in {g // 64 for g in focus}
        for col in ("match", "pr_commit"):
            if escaped:
                assert (b[col][:, blk] == poison).all(), (kind, wave, col)
            else:
                assert (b[col][:, blk] == a[col][:, blk]).all(), (kind, wave, col)
    for k in NOT_BEHIND:  # ... and nothing else anywhere
        assert (a[k] == b[k]).all(), k


# ---- the host state machine ----------------------------------------------------------------------------------------------------
TICK_MIRROR, TICK_OTHER, DROP, KEEP, KEEP_LOOK, OFF = range(6)
NONE = 0


def model_step(wb_after, executed, call, valid, behind, streak):
    """The rules of rg_mirror_step restated in Python (a guard against edits of the header that change an answer, not a second
    derivation; the sequences below are where the rules are checked against what a host does): -> (kernel, settle, valid, behind, streak)"""
    if call == KEEP:  # rg_results, rg_sync, ...: no settle, the streak goes on
        return NONE, 0, valid, behind, streak
    if call == TICK_MIRROR:
        if valid and wb_after and streak >= wb_after:
            return PACKED_WB, 0, 1, 1, streak  # the dense tick itself never settles and never ends a write-behind streak
        kernel = PACKED if valid else BUILD  # both need current columns
        settle = behind
        streak = 0 if (settle or not valid) else streak + 1
        return kernel, settle, 1, behind and not executed, streak
    # everything else settles what is behind and ends the streak; only the calls that look but do not write keep the plane
    return NONE, behind, valid if call == KEEP_LOOK else 0, behind and not executed, 0


def test_host_state_machine_table(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    if not os.path.exists(STATE_BIN) or os.path.getmtime(STATE_BIN) < max(os.path.getmtime(STATE_SRC), os.path.getmtime(os.path.join(CSRC, "rg_mirror_host.h"))):
        subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", STATE_SRC, "-o", STATE_BIN])
    lines = subprocess.run([STATE_BIN], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    assert lines[0] == "default_wb_after %d" % WB_AFTER and WB_AFTER >= 0
    rows = 0
    for line in lines[1:]:
        lhs, rhs = line.split(" -> ")
        args, got = tuple(int(x) for x in lhs.split()), tuple(int(x) for x in rhs.split())
        want = tuple(int(x) for x in model_step(*args))
        assert got == want, (args, got, want)
        rows += 1
    assert rows == sum(2 * 6 * 2 * 2 * (n + 2) for n in (0, 1, 3))


def test_host_state_machine_sequences():
    """Whole call sequences on the model the table test pins to the header: what the issue spells out."""
    def walk(calls, wb_after):
        st, kernels, settles = (0, 0, 0), [], 0
        for c in calls:
            k, s, *st = model_step(wb_after, 1, c, *st)
            kernels.append(k)
            settles += int(s)
        return kernels, settles, tuple(st)
    # back-to-back ticks: build, WB_AFTER write-through, write-behind from then on; rg_results in between changes nothing
    for n in (1, 3):
        k, s, st = walk([TICK_MIRROR] * (n + 4), n)
        assert k == [BUILD] + [PACKED] * n + [PACKED_WB] * 3 and s == 0 and st == (1, 1, n)
        k2, s2, _ = walk([TICK_MIRROR, KEEP] * (n + 4), n)
        assert [x for x in k2 if x] == k and s2 == 0
        # a host that looks at the columns between ticks never reaches write-behind and never pays a settle
        k3, s3, st3 = walk([TICK_MIRROR, KEEP_LOOK] * 8, n)
        assert [x for x in k3 if x] == [BUILD] + [PACKED] * 7 and s3 == 0 and st3[0] == 1
        # a settle point after a streak: one settle, the plane stays valid for a look and is dropped by RG_ENTER
        k4, s4, st4 = walk([TICK_MIRROR] * (n + 3) + [KEEP_LOOK, TICK_MIRROR], n)
        assert s4 == 1 and k4[-1] == PACKED and st4 == (1, 0, 1)
        k5, s5, st5 = walk([TICK_MIRROR] * (n + 3) + [DROP, TICK_MIRROR], n)
        assert s5 == 1 and k5[-1] == BUILD and st5 == (1, 0, 0)
    # a capture behind a streak: the mirror goes off, and every captured tick is a tick on another kernel. Its settle is CAPTURED,
    # not executed, so the columns stay behind on the host's books and every later captured tick puts a (guarded) settle in front
    # of itself too; the first entry point that executes one clears the books, and nothing settles after that.
    for n in (1, 3):
        st, settles = (0, 0, 0), []
        for c, executed in [(TICK_MIRROR, 1)] * (n + 3) + [(TICK_OTHER, 0)] * 3 + [(KEEP, 1), (KEEP_LOOK, 1), (DROP, 1), (TICK_OTHER, 1)]:
            k, s_, *st = model_step(n, executed, c, *st)
            settles.append(int(s_))
        assert settles == [0] * (n + 3) + [1, 1, 1] + [0, 1, 0, 0] and tuple(st) == (0, 0, 0)
    k, s, st = walk([TICK_MIRROR] * 9, 0)  # 0 = never
    assert k == [BUILD] + [PACKED] * 8 and s == 0 and st[1] == 0
