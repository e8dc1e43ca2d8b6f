"""Shared helpers of the read-mirror tests (raft_rs_amd/csrc/rg_mirror.h): the packed word in Python integers, planted layouts
(word edges, one escaping lane in an otherwise steady wave), messages that make a tick's commit index depend on ONE silent cell,
the statement of mirror validity the sequence tests count launches with, and the two-engine rig of the GPU tests.

Test infrastructure: numpy and Python integers; the rig at the end takes the product package as an argument."""
import itertools

import numpy as np

import fuzz

MT_ESC, PC_ESC = 0x8000, 0xFFFF
M64 = (1 << 64) - 1
MF_VALID = fuzz.MF_VALID


def model_word(mt, pc, c):
    """The issue's definition, in Python integers: differences in 64-bit wrap-around arithmetic, then range-checked."""
    dm = (mt - c) & M64
    sm = dm - (1 << 64) if dm >> 63 else dm
    lo = (sm & 0xFFFF) if -32767 <= sm <= 32767 else MT_ESC
    dp = (c - pc) & M64
    hi = dp if dp <= 65534 else PC_ESC
    return lo | (hi << 16)


EDGES = (0, 1, 32766, 32767, 32768, 65534, 65535, 65536)


def new_plane(st):
    return np.full((st["n_slots"], st["stride"]), 0xDEADBEEF, dtype=np.uint32)  # (never read before a build tick wrote it)


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


EDGE_COMMITS = (0, 5, (1 << 32) - 1, 1 << 32, (1 << 63) - 1, 3_000_000, 40_000, 65_535)


def plant_edges(rng, st, groups):
    """Groups whose cells sit at the edges of the word: match = commit +- EDGES, committed_index commit - EDGES and ABOVE commit,
    commits at 0, 2^32 - 1, 2^32 and 2^63 - 1 (wrap-around on either side)."""
    P = st["n_slots"]
    commits = list(EDGE_COMMITS)
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


def absent_garbage(rng, st):
    """Slots without a Progress hold arbitrary garbage in every column, some of it within reach of the commit index."""
    present = (st["cfg"] >> 24) & 0xFF
    for p in range(st["n_slots"]):
        absent = np.nonzero(((present >> p) & 1) == 0)[0]
        for k in ("match", "next", "pr_commit"):
            st[k][p, absent] = rng.integers(0, 1 << 63, size=len(absent), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        near = absent[::3]
        st["match"][p, near] = st["commit"][near] + np.uint64(7)
        st["pr_commit"][p, near] = st["commit"][near] - np.minimum(st["commit"][near], np.uint64(3))


# ---- one escaping lane in a steady wave --------------------------------------------------------------------------------------
KINDS = {"mt_hi": ("match", 32768), "mt_lo": ("match", -32768), "pc": ("pr_commit", -65535), "pc_above": ("pr_commit", 1)}
WAVE_COMMIT = 1_000_000


def wave_groups(st, wave):
    return range(64 * wave, min(st["n_groups"], 64 * wave + 64))


def plant_wave(st, wave, lanes, kind):
    """Every group of the 64-group block `wave` is steady: commit well above 2^16 (every planted cell stays a plain index),
    last_index commit + 40 000, the current term's entries from commit - 250; every slot's matched in commit + [-200, 200] and
    committed_index in commit - [0, 200], different per lane and slot, Replicate, nothing pending. The listed lanes get ONE
    field of `kind` that the word cannot hold, in one present slot (the lane picks which). -> [(group, slot)] of those fields."""
    col, off = KINDS[kind]
    P, planted = st["n_slots"], []
    for g in wave_groups(st, wave):
        lane = g - 64 * wave
        c = WAVE_COMMIT + 1009 * wave + 17 * lane
        st["commit"][g], st["term_hi"][g], st["term_lo"][g] = c, c + 40_000, c - 250
        for p in range(P):
            st["match"][p, g] = c + (lane * 37 + p * 113 + wave * 7) % 401 - 200
            st["next"][p, g] = int(st["match"][p, g]) + 1
            st["pr_commit"][p, g] = c - (lane * 11 + p * 59 + wave * 3) % 201
            st["pend_snap"][p, g] = st["pend_rs"][p, g] = 0
            st["pflags"][g, p] = 1 | 8  # Replicate, recent_active
        if lane in lanes:
            present = [p for p in range(P) if (int(st["cfg"][g]) >> (24 + p)) & 1]
            p = present[lane % len(present)]
            st[col][p, g] = c + off
            if col == "match":
                st["next"][p, g] = c + off + 1
            planted.append((g, p))
    return planted


# ---- messages under which ONE silent cell decides the commit index -----------------------------------------------------------
def _quorum_index(cfg, mt):
    """ProgressTracker::maximal_committed_index without group commit: the majority's index of the incoming voters, and of the
    outgoing ones in a joint configuration (the smaller of the two)."""
    q = None
    for mask in (cfg & 0xFF, (cfg >> 8) & 0xFF):
        if not mask:
            continue
        v = sorted((mt[s] for s in range(8) if (mask >> s) & 1), reverse=True)
        k = v[len(v) // 2]
        q = k if q is None else min(q, k)
    return q


def model_commit(cfg, mt, commit, lo, hi, acks):
    """The commit index a tick leaves: the accepted acks land in slot order, Raft::maybe_commit behind each (the quorum index
    commits when it is above the commit index and an entry of the current term: lo <= it <= hi)."""
    mt = list(mt) + [0] * (8 - len(mt))
    for s in sorted(acks):
        if acks[s] > mt[s]:
            mt[s] = acks[s]
            q = _quorum_index(cfg, mt)
            if q > commit and lo <= q <= hi:
                commit = q
    return commit


def deciding_acks(st, msgs, groups, m_commit_above=False):
    """Acks (RG_MF_VALID, index = the group's last_index, Message.commit 0) from FEWER than a quorum of the voters of each listed
    group, none from the leader's own slot, chosen so that the commit index the reference computes is the `matched` cell of a
    voter that gets no message: above the old commit index, inside the current term, and the ONLY cell with that value -- one more
    or one less in that cell and the tick commits something else (checked on the model above, for every candidate set of ackers).
    A listed group that has no such set (a single voter, group commit, a voter without a Progress, every silent cell at or below
    the commit index or outside the term, cells that wrap) gets no message and is not returned. Every message of the listed
    groups is overwritten, the other groups' are left alone. -> [(group, slot)]: the cell that decides.

    m_commit_above: the messages carry Message.commit = the acker's committed_index + 1 instead (Progress::update_committed then
    stores exactly that; the acker must hold a committed_index the word can represent, see the corrupted-plane test)."""
    P, decided = st["n_slots"], []
    for g in groups:
        msgs["m_flags"][g, :] = 0
        cfg = int(st["cfg"][g])
        voters = (cfg | (cfg >> 8)) & 0xFF
        present, self_slot = (cfg >> 24) & 0xFF, (cfg >> 16) & 7
        if (cfg & 0x80000) or (voters & ~present) or (voters >> P):
            continue
        mt = [int(st["match"][p, g]) for p in range(P)]
        c, lo, hi = int(st["commit"][g]), int(st["term_lo"][g]), int(st["term_hi"][g])
        if hi >> 63 or any(m > hi + (1 << 20) for m in mt):  # (wrapped cells: no plain index arithmetic to reason about)
            continue
        cand = [s for s in range(P) if (voters >> s) & 1 and s != self_slot]
        quorum = bin(cfg & 0xFF).count("1") // 2 + 1
        pick = None
        for n in range(min(quorum - 1, len(cand)), 0, -1):
            for A in itertools.combinations(cand, n):
                acks = {s: hi for s in A}
                new = model_commit(cfg, mt, c, lo, hi, acks)
                if new <= c:
                    continue
                who = [s for s in range(P) if (voters >> s) & 1 and s not in A and mt[s] == new]
                if len(who) != 1:
                    continue
                s = who[0]
                moved = [model_commit(cfg, mt[:s] + [mt[s] + d] + mt[s + 1:], c, lo, hi, acks) for d in (1, -1)]
                if new in moved:
                    continue
                pick = (A, s)
                break
            if pick:
                break
        if not pick:
            continue
        A, s = pick
        for a in A:
            msgs["m_flags"][g, a] = MF_VALID
            msgs["m_index"][a, g] = hi
            msgs["m_commit"][a, g] = (int(st["pr_commit"][a, g]) + 1) & M64 if m_commit_above else 0
            msgs["m_hint"][a, g] = msgs["m_rs"][a, g] = 0
            if "m_logterm" in msgs:
                msgs["m_logterm"][a, g] = 0
        decided.append((g, s))
    return decided


# ---- mirror validity, stated once ---------------------------------------------------------------------------------------------
CLASSES = ("tick", "keep", "drop", "off")


def after(call_class, was_valid):
    """Is the plane valid after a call of this class? `tick`: a dense tick of a mirror-capable engine (it leaves a valid plane
    whether it built or read it); `keep`: the documented read-only calls; `drop`: every other entry point; `off`: a call after
    which the engine never uses the mirror again (follow it with launch_counts, which remembers)."""
    assert call_class in CLASSES, call_class
    return {"tick": True, "keep": bool(was_valid), "drop": False, "off": False}[call_class]


def launch_counts(classes, valid=False, build=0, packed=0):
    """(build launches, packed launches, valid) after a sequence of call classes, from `after` alone."""
    off = False
    for c in classes:
        if c == "tick" and not off:
            if valid:
                packed += 1
            else:
                build += 1
        off = off or c == "off"
        valid = after(c, valid) and not off
    return build, packed, valid


# ---- the GPU rig: a mirror-on engine, its RG_CFGF_NO_READ_MIRROR twin, the oracle ----------------------------------------------
def in_domain(st):
    """Groups whose every index is a plain one (nothing wrapped below 0 or sits at the top of the u64 range): where the oracle's
    arithmetic, which is the reference's, is defined. The other groups are compared between the two engines only."""
    G, P = st["n_groups"], st["n_slots"]
    top = np.uint64((1 << 62) + (1 << 40))
    ok = (st["commit"][:G] < top) & (st["term_hi"][:G] < top) & (st["term_lo"][:G] < top)
    present = (st["cfg"][:G] >> 24) & 0xFF
    for p in range(P):
        has = ((present >> p) & 1).astype(bool)
        for k in ("match", "next", "pr_commit"):
            ok &= ~has | (st[k][p, :G] < top)
    return ok


MSG_KEYS = ("m_index", "m_commit", "m_hint", "m_rs", "m_flags")


class Rig:
    """Two engines loaded with the same state (mirror on / off, no size classes) and the oracle over the groups of its domain.
    tick(msgs) runs one tick everywhere and compares: the engines with the oracle (present cells, result words, results()), the
    engines with each other cell for cell, absent slots included. finish(n) asserts the launch counts: 1 build, n packed."""

    def __init__(self, rg, st, term, cache_policy=None, device_msgs=False, oracle_mask=None):
        import oracle_lib
        self.rg, self.G, self.P = rg, st["n_groups"], st["n_slots"]
        kw = {} if cache_policy is None else {"cache_policy": cache_policy}
        self.on = rg.Engine(self.G, self.P, flags=rg.CFGF.NO_SIZE_CLASSES, **kw)
        self.off = rg.Engine(self.G, self.P, flags=rg.CFGF.NO_SIZE_CLASSES | rg.CFGF.NO_READ_MIRROR, **kw)
        assert self.on.stride == st["stride"] == self.off.stride
        for e in (self.on, self.off):
            e.load_state(st)
        assert self.on.mirror_stats()["present"] == 1 and self.off.mirror_stats()["present"] == 0
        self.mask = in_domain(st) if oracle_mask is None else oracle_mask
        self.st = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
        for g in np.nonzero(~self.mask)[0]:  # outside its domain the oracle gets a quiet group (never compared)
            self.st["commit"][g], self.st["term_lo"][g], self.st["term_hi"][g] = 5, 1, 9
            for k in ("match", "next", "pr_commit", "pend_snap", "pend_rs"):
                self.st[k][:, g] = 5
            for k in ("run_first", "run_term"):
                if k in self.st:
                    self.st[k][:, g] = 0
            for k in ("dummy_index", "dummy_term"):
                if k in self.st:
                    self.st[k][g] = 0
        self.cl = oracle_lib.Cluster(self.G)
        self.cl.load_soa(self.st, term=term)
        self.gout = np.zeros(self.G, dtype=np.uint32)
        self.mb = rg.MsgBuffers(self.G, self.P, self.on.stride)
        self.device_msgs = device_msgs
        self.ticks = 0
        self.elected = self.rejected = 0

    def oracle_state(self):
        """The oracle's columns as they stand (what the next tick's messages are made from)."""
        self.cl.store_soa(self.st)
        return self.st

    def tick(self, msgs, streaming=None):
        rg = self.rg
        for k in MSG_KEYS:
            getattr(self.mb, k)[...] = msgs[k]
        if self.device_msgs:
            import torch
            dev = [torch.from_numpy(np.ascontiguousarray(msgs[k]).view(np.uint8 if k == "m_flags" else np.int64).copy()).cuda()
                   for k in MSG_KEYS]
            for e in (self.on, self.off):
                e.tick_device(*[d.data_ptr() for d in dev])
            for e in (self.on, self.off):
                e.sync()
        else:
            for e in (self.on, self.off):
                e.tick(self.mb)
        if streaming is not None:
            info = self.on.device_info()
            assert info["last_tick_streaming"] == streaming and info["last_tick_kernel"] == rg.KERNEL.NAMES[rg.KERNEL.LANE], info
        m = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in msgs.items()}
        m["m_flags"][~self.mask, :] = 0
        self_slot = (self.st["cfg"] >> 16) & 7
        for p in range(self.P):  # rejects of followers (the leader's own slot uses the bit for an election)
            self.rejected += int((((m["m_flags"][:, p] & 3) == 3) & (self_slot != p) & self.mask).sum())
        self.cl.tick_soa(m, self.gout)
        self.cl.store_soa(self.st)
        a, b = self.on.read_state(), self.off.read_state()
        t = self.ticks
        diffs = fuzz.diff_states(a, b, self.G, self.P, present_only=False)
        assert not diffs, (t, "mirror on / off", diffs[:5])
        assert (a["out"] == b["out"]).all(), (t, np.nonzero(a["out"] != b["out"])[0][:5])
        diffs = [d for d in self.diff_oracle(a)]
        assert not diffs, (t, "oracle", diffs[:5])
        bad = np.nonzero((a["out"] != self.gout) & self.mask)[0]
        assert bad.size == 0, (t, bad[:5], [hex(x) for x in a["out"][bad[:5]]], [hex(x) for x in self.gout[bad[:5]]])
        self.elected += int(((self.gout & 0x10) != 0)[self.mask].sum())  # RG_OUT_BECAME_LEADER
        for e, s in ((self.on, a), (self.off, b)):
            commit, out = e.results()
            assert (commit == s["commit"]).all() and (out == s["out"]).all(), t
        self.ticks += 1
        return a

    def diff_oracle(self, got):
        """fuzz.diff_states against the oracle, over the groups of its domain."""
        ref = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in self.st.items()}
        out = ~self.mask
        for k in fuzz.STATE_KEYS:
            if k == "pflags":
                ref[k][out, :] = got[k][out, :]
            elif ref[k].ndim == 2:
                ref[k][:, :self.G][:, out] = got[k][:, :self.G][:, out]
            else:
                ref[k][:self.G][out] = got[k][:self.G][out]
        return fuzz.diff_states(ref, got, self.G, self.P)

    def finish(self, packed, build=1):
        s = self.on.mirror_stats()
        assert (s["build_launches"], s["packed_launches"], s["valid"], s["off"]) == (build, packed, 1, 0), s
        s = self.off.mirror_stats()
        assert (s["build_launches"], s["packed_launches"]) == (0, 0), s
        self.on.close()
        self.off.close()
