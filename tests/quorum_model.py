"""Plain numpy restatements of what the tick unit's small kernels compute -- TEST INFRASTRUCTURE (numpy only).

Written from the reference's text (the citations), one vectorised function per operation, every group at once. Nothing here is
derived from the kernels; tests/test_quorum_model.py pins the functions to the reference's golden vote vectors and to the oracle
before tests/test_tick_unit_edges_gpu.py lets them judge a kernel.

A configuration word is RG_CFG_MAKE's: incoming | outgoing << 8 | self << 16 | group_commit << 19 | transferee + 1 << 20 |
present << 24. Slot s is the peer with id s + 1 wherever the oracle is asked."""
import numpy as np

import hosthints

PENDING, LOST, WON = 0, 1, 2
PF_STATE, PF_PAUSED, PF_RECENT_ACTIVE, PF_INS_FULL, PF_PEND_SNAP = 0x03, 0x04, 0x08, 0x10, 0x40
PROBE, REPLICATE, SNAPSHOT = 0, 1, 2
MF_VALID, MF_REJECT, MF_BECOME_LEADER = hosthints.MF_VALID, hosthints.MF_REJECT, 0x02
OUT_CHANGED, OUT_FAULT, OUT_HOST_HINT = 0x1, 0x2, hosthints.OUT_HOST_HINT
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)


def cfg_fields(cfg):
    """-> (incoming, outgoing, self slot, present) as int64 arrays."""
    c = np.asarray(cfg).astype(np.int64)
    return c & 0xff, (c >> 8) & 0xff, (c >> 16) & 7, (c >> 24) & 0xff


def popcount8(x):
    x = np.asarray(x).astype(np.int64) & 0xff
    return sum((x >> b) & 1 for b in range(8))


def majority_vote(voters, yes, no):
    """MajorityConfig::vote_result (majority.rs:130-154) over slot bitmasks: an empty configuration wins."""
    n = popcount8(voters)
    q = n // 2 + 1  # crate::majority
    y = popcount8(voters & yes)
    missing = popcount8(voters & ~(yes | no))
    res = np.where(y >= q, WON, np.where(y + missing >= q, PENDING, LOST))
    return np.where(n == 0, WON, res)


def joint_vote(i, o):
    """JointConfig::vote_result (joint.rs:56-67)."""
    return np.where((i == WON) & (o == WON), WON, np.where((i == LOST) | (o == LOST), LOST, PENDING))


def recorded(yes, no):
    """record_vote keeps the FIRST vote of an id (tracker.rs:307-309); the bitmask form has no order, a slot set in both masks
    counts as yes."""
    yes = np.asarray(yes).astype(np.int64) & 0xff
    return yes, np.asarray(no).astype(np.int64) & 0xff & ~yes


def vote_result(cfg, yes, no):
    """ProgressTracker::vote_result (tracker.rs:338-340) -> u8[G]: 0 Pending, 1 Lost, 2 Won."""
    inc, out, _, _ = cfg_fields(cfg)
    y, n = recorded(yes, no)
    return joint_vote(majority_vote(inc, y, n), majority_vote(out, y, n)).astype(np.uint8)


def tally_votes(cfg, yes, no):
    """ProgressTracker::tally_votes (tracker.rs:313-333) -> (granted, rejected, result): only the votes of ids that are voters
    now (incoming or outgoing) are counted."""
    inc, out, _, _ = cfg_fields(cfg)
    y, n = recorded(yes, no)
    voters = inc | out
    return popcount8(y & voters).astype(np.uint8), popcount8(n & voters).astype(np.uint8), vote_result(cfg, yes, no)


def quorum_recently_active(cfg, pflags):
    """ProgressTracker::quorum_recently_active (tracker.rs:346-361) -> (result u8[G], pflags afterwards u8[G][8]): over the
    slots that have a Progress, the self slot is set and active, every other one is active iff recent_active was set and is
    cleared; has_quorum (tracker.rs:367-372) over the active set. Nothing else of a flag byte moves."""
    inc, out, self_slot, present = cfg_fields(cfg)
    after = np.array(pflags, dtype=np.uint8, copy=True)
    active = np.zeros(len(inc), dtype=np.int64)
    for s in range(8):
        has = ((present >> s) & 1) == 1
        own = has & (self_slot == s)
        other = has & (self_slot != s)
        was = (after[:, s] & PF_RECENT_ACTIVE) != 0
        active |= ((own | (other & was)).astype(np.int64)) << s
        after[own, s] |= PF_RECENT_ACTIVE
        after[other, s] &= np.uint8(~PF_RECENT_ACTIVE & 0xff)
    zero = np.zeros_like(active)
    won = joint_vote(majority_vote(inc, active, zero), majority_vote(out, active, zero)) == WON
    return won.astype(np.uint8), after


def heartbeat_commits(cfg, match, commit):
    """send_heartbeat's commit (raft.rs:830-838): min(pr.matched, raft_log.committed) per slot -> u64 [P][G]; 0 where the slot
    has no Progress (nothing is sent there)."""
    _, _, _, present = cfg_fields(cfg)
    G = len(present)
    match = np.asarray(match, dtype=np.uint64)[:, :G]
    hb = np.minimum(match, np.asarray(commit, dtype=np.uint64)[None, :G])
    for s in range(match.shape[0]):
        hb[s, ((present >> s) & 1) == 0] = 0
    return hb


def _majority_committed(voters, match, gid, use_gc):
    """MajorityConfig::committed_index (majority.rs:70-124) for ONE majority of every group: (index u64[G], flag bool[G]).
    `match` / `gid` are [P][G] with the cells of voters without a Progress already zero (unwrap_or_default). The voters are
    visited in id order and sorted stably by descending index, as the oracle does."""
    P, G = match.shape
    n = popcount8(voters)
    is_v = np.stack([((voters >> s) & 1) == 1 for s in range(P)], axis=0)
    # (lexsort is stable; its last key is the primary one: non-voters sort behind every voter)
    order = np.lexsort((U64_MAX - match, ~is_v), axis=0)
    m_sorted = np.take_along_axis(match, order, axis=0)
    g_sorted = np.take_along_axis(gid, order, axis=0)
    cols = np.arange(G)
    q = np.maximum(n // 2 + 1, 1)
    qi = m_sorted[np.minimum(q - 1, P - 1), cols]
    qg = g_sorted[np.minimum(q - 1, P - 1), cols]
    if not use_gc:
        idx, flag = qi.copy(), np.zeros(G, dtype=bool)
    else:
        checked = qg.copy()
        single = np.ones(G, dtype=bool)
        done = np.zeros(G, dtype=bool)
        idx = np.zeros(G, dtype=np.uint64)
        for k in range(P):
            live = (k < n) & ~done
            gk, mk = g_sorted[k], m_sorted[k]
            z = live & (gk == 0)
            single &= ~z
            take = live & (gk != 0) & (checked == 0)
            checked = np.where(take, gk, checked)
            diff = live & (gk != 0) & ~take & (checked != gk)
            idx = np.where(diff, np.minimum(mk, qi), idx)
            done |= diff
        last = m_sorted[np.maximum(n - 1, 0), cols]
        idx = np.where(done, idx, np.where(single, qi, last))
        flag = done
    empty = n == 0
    return np.where(empty, U64_MAX, idx).astype(np.uint64), np.where(empty, True, flag)


def maximal_committed_index(cfg, match, gid=None):
    """ProgressTracker::maximal_committed_index (tracker.rs:294-298 -> joint.rs:47-51 -> majority.rs:70-124) ->
    (mci u64[G], used_group_commit bool[G]). Group commit where the word's RG_CFG_GROUP_COMMIT bit is set."""
    inc, out, _, present = cfg_fields(cfg)
    G = len(inc)
    match = np.array(np.asarray(match, dtype=np.uint64)[:, :G], copy=True)
    P = match.shape[0]
    gid = np.zeros_like(match) if gid is None else np.array(np.asarray(gid, dtype=np.uint64)[:, :G], copy=True)
    for s in range(P):
        absent = ((present >> s) & 1) == 0
        match[s, absent] = 0
        gid[s, absent] = 0
    gc = (np.asarray(cfg).astype(np.int64) & 0x00080000) != 0
    res = {}
    for use in (False, True):
        i_idx, i_f = _majority_committed(inc, match, gid, use)
        o_idx, o_f = _majority_committed(out, match, gid, use)
        res[use] = (np.minimum(i_idx, o_idx), i_f & o_f)
    return np.where(gc, res[True][0], res[False][0]).astype(np.uint64), np.where(gc, res[True][1], res[False][1])


def msg_stats(m_flags, cfg):
    """rg_msg_stats' five counters as include/raftgroups.h words them, over u8 [G][8] flag bytes:
    [0] flag bytes with RG_MF_VALID; [1] bytes with RG_MF_VALID and RG_MF_REJECT both, on slots other than the self slot;
    [2] slots with a Progress; [3] groups with a non-zero flag byte; [4] groups whose self slot has a Progress and carries
    RG_MF_BECOME_LEADER."""
    _, _, self_slot, present = cfg_fields(cfg)
    f = np.asarray(m_flags, dtype=np.uint8)
    slot = np.arange(8)[None, :]
    own = slot == self_slot[:, None]
    valid = (f & MF_VALID) != 0
    rej = valid & ((f & MF_REJECT) != 0) & ~own
    self_present = ((present >> self_slot) & 1) == 1
    own_byte = f[np.arange(len(f)), self_slot]
    elect = self_present & ((own_byte & MF_BECOME_LEADER) != 0)
    return [int(valid.sum()), int(rej.sum()), int(popcount8(present).sum()), int((f != 0).any(axis=1).sum()), int(elect.sum())]


def result_counts(out):
    """rg_result_counts: (groups with RG_OUT_CHANGED, groups with RG_OUT_FAULT) of RG_COL_OUT."""
    out = np.asarray(out)
    return int(((out & OUT_CHANGED) != 0).sum()), int(((out & OUT_FAULT) != 0).sum())


def host_hints(out, hhint):
    """rg_host_hints: {group: slot mask} over the groups whose result word carries RG_OUT_HOST_HINT."""
    out, hhint = np.asarray(out), np.asarray(hhint)
    return {int(g): int(hhint[g]) for g in np.nonzero(out & OUT_HOST_HINT)[0]}


def resolved_reject(match, nxt, psnap, pflags, index, hint, device_inflights=False):
    """The rest of handle_append_response's reject branch for one cell each (elementwise over equal-length arrays):
    Progress::maybe_decr_to(index, hint, INVALID_INDEX) (progress.rs:168-206), become_probe when that leaves Replicate
    (raft.rs:1716-1718, progress.rs:95-107). -> (applied bool, next, pending_snapshot, flag byte). RG_PF_PEND_SNAP follows
    pending_snapshot; with device Inflights reset_state's ins.reset() leaves a window that is not full."""
    match, nxt, psnap = (np.asarray(a, dtype=np.uint64) for a in (match, nxt, psnap))
    index, hint = np.asarray(index, dtype=np.uint64), np.asarray(hint, dtype=np.uint64)
    pf = np.asarray(pflags, dtype=np.uint8)
    repl = (pf & PF_STATE) == REPLICATE
    one = np.uint64(1)
    ok_r = repl & (index > match)
    ok_p = ~repl & (nxt != 0) & (nxt - one == index)
    dec = np.maximum(np.minimum(index, hint + one), one)
    dec = np.where(hint == U64_MAX, np.maximum(index, one), dec)  # (hint + 1 does not wrap in the reference's domain)
    nxt2 = np.where(ok_r, match + one, np.where(ok_p, dec, nxt)).astype(np.uint64)
    psnap2 = np.where(ok_r, np.uint64(0), psnap).astype(np.uint64)
    probe = (pf & np.uint8(~(PF_STATE | PF_PAUSED | PF_PEND_SNAP) & 0xff)) | np.uint8(PROBE)
    if device_inflights:
        probe = probe & np.uint8(~PF_INS_FULL & 0xff)
    pf2 = np.where(ok_r, probe, np.where(ok_p, pf & np.uint8(~PF_PAUSED & 0xff), pf)).astype(np.uint8)
    return ok_r | ok_p, nxt2, psnap2, pf2
