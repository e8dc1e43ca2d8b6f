"""Helpers of tests/test_ingest_edges_gpu.py: the ingest path's road constants, wire-order record builders and the judge
for windows in which two DIFFERENT records race for one cell.

Test infrastructure: plain numpy, no dependency on the oracle or the engine (tests/test_ingestcheck.py runs it on the CPU).
"""
import os
import re

import numpy as np

import fuzz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Which road rg_ingest_tick takes is decided by these three (raft_rs_amd/csrc/abi_mirror.hip, rg_sparse_roundtrip and rg_flush_launch):
#   records <= RG_INGEST_BLOCK and window <= RG_ZEROCOPY_MAX   one launch (k_flush_small)
#   window <= RG_ZEROCOPY_MAX                                  zero-copy: k_ingest reads pinned host memory, does RgClear's work
#   records <= RG_ROUNDTRIP_MAX                                one round trip through device staging
#   above                                                      rg_ingest + rg_tick_ingested (three calls)
# tests/test_ingestcheck.py compares them with the kernels' headers: a threshold that moves takes the test sizes along.
RG_INGEST_BLOCK = 256     # records one workgroup of k_ingest stages
RG_ZEROCOPY_MAX = 1024    # window (min(records of the window, G)) up to which the kernels work on pinned host memory
RG_ROUNDTRIP_MAX = 16384  # records above which rg_ingest_tick runs the three-call sequence

ROAD_CONSTANT_FILES = {"RG_INGEST_BLOCK": "rg_tick_kernels.h", "RG_ZEROCOPY_MAX": "rg_kernels_sparse.h",
                       "RG_ROUNDTRIP_MAX": "rg_kernels_sparse.h"}


def parse_road_constants(csrc=None):
    """{name: value} of the three #defines as the kernels' headers have them."""
    csrc = csrc or os.path.join(ROOT, "raft_rs_amd", "csrc")
    out = {}
    for name, fn in ROAD_CONSTANT_FILES.items():
        with open(os.path.join(csrc, fn)) as f:
            m = re.findall(r"^#define\s+%s\s+(\d+)\b" % name, f.read(), flags=re.M)
        assert len(m) == 1, f"{fn}: expected exactly one #define {name}, found {len(m)}"
        out[name] = int(m[0])
    return out


def edge_counts(n_groups):
    """The record counts at which rg_ingest_tick / k_ingest change what they do, for an engine of n_groups groups (P = 5):
    one record, around one and two workgroups, around the zero-copy window, around a few thousand, around the three-call
    threshold, and about three records per group."""
    B, Z, R = RG_INGEST_BLOCK, RG_ZEROCOPY_MAX, RG_ROUNDTRIP_MAX
    return [1, B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1, Z, Z + 1, 4 * Z, 4 * Z + 1, R, R + 1, 3 * n_groups]


# rg_wire_msg (include/raftgroups.h); the GPU tests compare it with raft_rs_amd.engine.WIRE_DTYPE
WIRE_DTYPE = np.dtype([("group", "<u8"), ("index", "<u8"), ("commit", "<u8"), ("hint", "<u8"), ("rs", "<u8"),
                       ("log_term", "<u8"), ("slot", "<u4"), ("flags", "<u4"), ("pad", "<u8")])

ORDERS = ("shuffled", "slot_adjacent", "slot_strided")


def records(msgs, groups, P, order="shuffled", rng=None):
    """Wire records of every cell of `groups` that has an event in the alloc_msgs() dict `msgs`.
    order: "shuffled"       arbitrary wire order (needs rng)
           "slot_adjacent"  the slots of a group in consecutive records: they fall into one wave (at most 8 slots, 64 lanes,
                            as long as a group's run does not straddle a multiple of 64) and retry the CAS on one flag word
           "slot_strided"   slot s of every group in block s of the array: the slots of one group fall into different
                            workgroups as soon as a block holds RG_INGEST_BLOCK records -- the race for the group's list entry
    """
    assert order in ORDERS, order
    groups = np.asarray(groups, dtype=np.int64)
    f = msgs["m_flags"][groups, :P]
    gi, p = np.nonzero(f)  # row-major: by group (in the order given), then by slot
    if order == "slot_strided":
        o = np.argsort(p, kind="stable")
        gi, p = gi[o], p[o]
    g = groups[gi]
    arr = np.zeros(len(g), dtype=WIRE_DTYPE)
    arr["group"], arr["slot"], arr["flags"] = g, p, msgs["m_flags"][g, p]
    arr["index"], arr["commit"] = msgs["m_index"][p, g], msgs["m_commit"][p, g]
    arr["hint"], arr["rs"] = msgs["m_hint"][p, g], msgs["m_rs"][p, g]
    if "m_logterm" in msgs:
        arr["log_term"] = msgs["m_logterm"][p, g]
    if order == "shuffled":
        assert rng is not None, "order='shuffled' needs rng"
        rng.shuffle(arr)
    return arr


def keep_groups(msgs, groups):
    """Zero the event bytes of every group that is not in `groups`."""
    keep = np.zeros(msgs["m_flags"].shape[0], dtype=bool)
    keep[np.asarray(groups, dtype=np.int64)] = True
    msgs["m_flags"][~keep] = 0


def fit_record_count(msgs, group_order, n, P, pad_flag=fuzz.MF_SENT):
    """Cut the events in `msgs` down to EXACTLY n records: the groups of `group_order`, in that order, keep their events until n
    cells are reached, the group that crosses n loses its highest slots, every other group loses all. When all the groups
    together have fewer than n events, empty cells (in the same order) get `pad_flag`. Returns the groups left with events,
    sorted."""
    f = msgs["m_flags"]
    G = f.shape[0]
    order = np.asarray(group_order, dtype=np.int64)
    assert len(np.unique(order)) == len(order) and n <= len(order) * P
    f[:, P:] = 0
    keep_groups(msgs, order)
    have = int(np.count_nonzero(f[:, :P]))
    if have < n:  # pad: empty cells of the listed groups, group by group
        sub = f[order, :P]
        gi, p = np.nonzero(sub == 0)
        gi, p = gi[:n - have], p[:n - have]
        f[order[gi], p] = pad_flag
    else:
        per = np.count_nonzero(f[order, :P], axis=1)
        cum = np.cumsum(per)
        k = int(np.searchsorted(cum, n))  # group k crosses (or reaches) n
        f[order[k + 1:]] = 0
        extra = int(cum[k]) - n
        g = int(order[k])
        for p in range(P - 1, -1, -1):
            if extra and f[g, p]:
                f[g, p] = 0
                extra -= 1
    assert int(np.count_nonzero(f[:, :P])) == n
    assert G == f.shape[0]
    return np.nonzero(f[:, :P].any(axis=1))[0]


def fill_cells(msgs, groups, P, pad_flag=fuzz.MF_SENT):
    """Give every empty cell (slots < P) of `groups` the event `pad_flag`: all P slots of each group then carry a record."""
    groups = np.asarray(groups, dtype=np.int64)
    sub = msgs["m_flags"][groups, :P]
    sub[sub == 0] = pad_flag
    msgs["m_flags"][groups, :P] = sub


# ---- the judge ----------------------------------------------------------------------------------------------------------
JUDGED_KEYS = fuzz.STATE_KEYS + ("out",)


def groups_equal(ref, got, groups, P, keys=JUDGED_KEYS):
    """bool[len(groups)]: group g of `got` equals group g of `ref` on EVERY column of `keys` (per-slot columns and pflags on the
    slots that ref's cfg word has a Progress for, as fuzz.diff_states compares them)."""
    groups = np.asarray(groups, dtype=np.int64)
    present = ((ref["cfg"][groups] >> 24) & 0xff).astype(np.uint32)
    mask = np.stack([(present >> p) & 1 for p in range(P)], axis=0).astype(bool)  # [P][n]
    same = np.ones(len(groups), dtype=bool)
    for k in keys:
        x, y = ref[k], got[k]
        if k == "pflags":
            same &= ~(((x[groups, :P] != y[groups, :P]) & mask.T).any(axis=1))
        elif x.ndim == 2:
            same &= ~(((x[:P, groups] != y[:P, groups]) & mask).any(axis=0))
        else:
            same &= x[groups] == y[groups]
    return same


def assert_distinguishable(state_a, state_b, groups, P):
    """The judge's condition on its inputs: "all A" and "all B" differ in every judged group."""
    same = groups_equal(state_a, state_b, groups, P)
    assert not same.any(), f"A and B give the same state in groups {np.asarray(groups)[same][:8]}: the judge could not tell"


def judge(state_a, state_b, got, groups, P):
    """A window in which every group of `groups` had two different records A and B for one cell; which one wins the cell is
    not specified. state_a / state_b: the oracle's state (fuzz.STATE_KEYS + "out") after the window with A / with B in every
    group; got: the engine's. Every group must equal ONE of the two on every column and its result word -- fields of A
    with fields of B fail. Returns u8[len(groups)]: 0 where the engine applied A, 1 where it applied B. No group is left
    out: one that equals both fails as well (assert_distinguishable says so before anything is run)."""
    groups = np.asarray(groups, dtype=np.int64)
    eq_a = groups_equal(state_a, got, groups, P)
    eq_b = groups_equal(state_b, got, groups, P)
    neither = ~eq_a & ~eq_b
    if neither.any():
        g = int(groups[neither][0])
        detail = []
        for k in JUDGED_KEYS:
            col = (lambda s: s[k][g, :P] if k == "pflags" else (s[k][:P, g] if s[k].ndim == 2 else s[k][g]))
            a, b, e = col(state_a), col(state_b), col(got)
            if not (np.array_equal(a, e) and np.array_equal(b, e)):
                detail.append(f"{k}: A={a} B={b} engine={e}")
        raise AssertionError(f"{int(neither.sum())} groups are neither A nor B (a mix of the two records, or neither applied); "
                             f"group {g}:\n  " + "\n  ".join(detail))
    both = eq_a & eq_b
    assert not both.any(), f"groups {groups[both][:8]} equal A and B alike: indistinguishable inputs"
    return np.where(eq_a, 0, 1).astype(np.uint8)
