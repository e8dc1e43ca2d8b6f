"""Commit publication slices (raft_rs_amd/csrc/rg_publish.h) for the tests: the layout, a canonical form to compare two slices
by, the decoded advance, and crafted message streams that move every group's commit index by a chosen amount.

A slice is [ RgPubHdr | RgPubOvf list[cap] | u8 delta[Gpad] ]; the advance of group g = delta[g] + the sum of its list entries.
Two slices that describe the same advances may still differ in the list: its order comes from atomics on the device, and several
saturating steps inside one publication interval append several entries for one group where a single step old -> new appends one.
The canonical form keeps what must agree: the delta bytes, the zero padding behind them, the per-group sums of the list, the
LOST flag. Where a slice is lost (more entries than the list holds) its list is incomplete and only the flag is compared."""
import numpy as np

import fuzz
import oracle_lib as O

HDR_BYTES, OVF_BYTES, PUB_LOST = 16, 16, 0x1
OVF_DTYPE = np.dtype([("group", "<u8"), ("extra", "<u8")])

# advances at the edges of the encoding: the byte, its saturation, the exact list (16 / 32-bit boundaries, beyond 2^32)
EDGES = [0, 1, 254, 255, 256, 65_535, 65_536, 65_537, 2**32 + 3]
# per-tick advances of ONE interval (up to three ticks): the byte crosses 255 only on the second or the third tick, or a
# saturated byte takes more, or an exact step is followed by small ones
MULTI = [[100, 100, 100], [200, 60], [255, 1], [0, 256], [254, 0, 1], [65_535, 1, 1], [1, 2**32 + 3], [128, 127, 1],
         [300, 0, 300], [7, 9, 11]]


def default_cap(G):
    return G // 256 + 64  # (rg_comm_init's overflow_slots = 0)


def layout(G, cap):
    Gpad = (G + 255) // 256 * 256
    off_delta = (HDR_BYTES + cap * OVF_BYTES + 255) // 256 * 256
    return Gpad, off_delta, off_delta + Gpad


def new_slice(G, cap):
    return np.zeros(layout(G, cap)[2], dtype=np.uint8)


def header(sl):
    n, flags = sl[:8].view(np.uint32)
    return int(n), int(flags)


def canonical(sl, G, cap):
    """(delta[0:G), delta[G:Gpad), per-group list sums or None when lost, n_overflow, lost flag)."""
    Gpad, off_delta, total = layout(G, cap)
    assert len(sl) == total, (len(sl), total)
    n, flags = header(sl)
    delta = sl[off_delta:off_delta + G]
    pad = sl[off_delta + G:off_delta + Gpad]
    lost = bool(flags & PUB_LOST)
    sums = None
    if not lost:
        ent = sl[HDR_BYTES:HDR_BYTES + min(n, cap) * OVF_BYTES].view(OVF_DTYPE)
        assert (ent["group"] < G).all(), ent["group"][ent["group"] >= G][:5]
        assert (ent["extra"] > 0).all()
        sums = np.zeros(G, dtype=np.uint64)
        np.add.at(sums, ent["group"].astype(np.int64), ent["extra"])
    return delta, pad, sums, n, lost


def decode(sl, G, cap):
    """The advance of every group the slice describes (it must not be lost)."""
    delta, _, sums, _, lost = canonical(sl, G, cap)
    assert not lost
    return delta.astype(np.uint64) + sums


def assert_same_slice(got, want, G, cap, what=""):
    """`got` and `want` (e.g. a device slice and rg_pub_accumulate_host's) describe the same advances."""
    gd, gp, gs, gn, gl = canonical(got, G, cap)
    wd, wp, ws, wn, wl = canonical(want, G, cap)
    assert not gp.any(), (what, "padding behind delta[G) written", np.nonzero(gp)[0][:5])
    assert not wp.any(), what
    bad = np.nonzero(gd != wd)[0]
    assert bad.size == 0, (what, "delta bytes", bad[:8], gd[bad[:8]], wd[bad[:8]])
    # RG_PUB_LOST exactly when the slice's own list overflowed (a loss announced by the engine sets it too: not here)
    assert gl == (gn > cap), (what, "LOST flag vs n_overflow", gl, gn, cap)
    assert wl == (wn > cap), (what, wl, wn, cap)
    assert gl == wl, (what, "one slice lost, the other not", gn, wn, cap)
    if not gl:
        bad = np.nonzero(gs != ws)[0]
        assert bad.size == 0, (what, "list sums", bad[:8], gs[bad[:8]], ws[bad[:8]])
        assert gn >= wn, (what, "fewer list entries than one step per group needs", gn, wn)


def pattern_advances(G, T, seed=0):
    """[T][G] advances: group g takes one of the edge advances (on the first tick) or one of the multi-tick patterns, cut to T
    ticks; group G - 1 always advances, across 255 on its second tick where there is one."""
    pats = [[e] for e in EDGES] + MULTI
    adv = np.zeros((T, G), dtype=np.uint64)
    for g in range(G):
        p = pats[(g + seed) % len(pats)]
        for t in range(min(T, len(p))):
            adv[t, g] = p[t]
    adv[:, G - 1] = 0
    adv[0, G - 1] = 200
    if T > 1:
        adv[1, G - 1] = 100
    return adv


def crafted_state(G, P, base, gc=False):
    """Every group: leader in slot 0 over P voters (two commit groups with group commit), log, matches and commit at `base`,
    every peer in Replicate."""
    from raft_rs_amd import engine as E
    st = O.alloc_state(G, P)
    st["cfg"][:] = E.cfg_make((1 << P) - 1, self_slot=0, group_commit=gc)
    if gc:
        st["gid"][:P, :G] = (np.arange(P, dtype=np.uint64) % 2 + 1)[:, None]
    st["term_lo"][:] = 1
    st["term_hi"][:] = base
    st["commit"][:] = base
    st["match"][:P, :G] = base
    st["pr_commit"][:P, :G] = base
    st["next"][:P, :G] = base + 1
    st["pflags"][:, :P] = 1  # Replicate
    return st


def ack_msgs(msgs, commit, target):
    """One tick that moves every group's commit index from `commit` to `target` (>= it): the leader (slot 0) appends up to
    target and persists it, every follower acknowledges it."""
    P = msgs["m_index"].shape[0]
    G = len(target)
    msgs["m_flags"][...] = 0
    for k in ("m_index", "m_commit", "m_hint", "m_rs"):
        msgs[k][...] = 0
    if "m_logterm" in msgs:
        msgs["m_logterm"][...] = 0
    moved = target != commit
    for p in range(P):
        msgs["m_index"][p, :G] = target
        msgs["m_commit"][p, :G] = target if p == 0 else commit
        msgs["m_flags"][:, p] = np.where(moved, fuzz.MF_VALID | (fuzz.MF_APPEND if p == 0 else 0), 0).astype(np.uint8)
    return msgs
