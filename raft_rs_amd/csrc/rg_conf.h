// rg_conf.h -- the batched conf change (include/raftgroups_conf.h): the per-group arithmetic of ProgressTracker::apply_conf
// (src/tracker.rs:380-397) and Raft::post_conf_change (src/raft.rs:2604-2673) for a group this store leads. Citations are relative to
// the pingcap/raft-rs v0.6.0 tree.
//
// Everything works on values: the kernels (rg_kernels_conf.h) load a group's cells, call the functions and store what they return,
// so that a lane issues its loads before its first store and the send phase never reads through memory what apply_conf has just
// decided. The order of a group is
//   rg_conf_check      the refusals, in the header's order (FAULT, NOT_LED, HOST) and DEMOTED
//   rg_conf_apply      the new cfg word and flag row, the slots added and removed
//   rg_conf_mci        JointConfig::committed_index over the new voters (the kernels take rg_mci_group instead under group commit),
//                      then rg_conf_log_maybe_commit
//   rg_conf_send_peer  ONE pass of maybe_send_append(to, allow_empty) for one peer -- the literal loop body of rg_send_serve
//                      (rg_send.h), never its `while` loop -- with Progress::update_state(last) applied to the values
//   rg_conf_transfer   the transfer abort
//
// Host/device-clean like rg_term.h: the kernels include it behind rg_common.h, tests/host_check/conf_twin.cpp includes it ALONE and
// is checked against tests/conf_model.py, sanitizers included -- nothing below needs a device header.
#pragma once
#include "rg_term.h"

#include "../../include/raftgroups_conf.h"

#define RG_CONF_FIELDS 0xff00ffffu /* incoming | outgoing << 8 | present << 24: what a record's word may carry */
#define RG_CONF_KEPT 0x00ff0000u   /* SELF, GROUP_COMMIT, TRANSFEREE: what the device keeps of the old word */

// What the sparse form refuses on the host and the kernels as FAULT: the word alone, without the group's state. 0 = fine, else the
// number of the rule it breaks.
RG_FOLLOW_HD int rg_conf_word_check(u32 W, u32 P) {
    if (W & ~RG_CONF_FIELDS) return 1; // a bit outside the three fields
    const u32 in = RG_CFG_INCOMING(W), out = RG_CFG_OUTGOING(W), pres = RG_CFG_PRESENT(W);
    if ((in | out | pres) >> P) return 2; // a slot >= P
    if (in == 0) return 3;                // no voter
    if ((in | out) & ~pres) return 4;     // a voter without a Progress (check_invariants, changer.rs:285-355)
    return 0;
}

// The refusals in the header's order; `clock`: the leader's clock layer is on, `led`: rg_term_led of the group's cell (read only
// under `clock`). -> RGC_CONF_DONE, _DEMOTED or the refusal.
RG_D u32 rg_conf_check(u32 W, u32 old, u32 P, bool clock, bool led) {
    const u32 self = RG_CFG_SELF(old);
    if (rg_conf_word_check(W, P) != 0 || self >= P || !((RG_CFG_PRESENT(old) >> self) & 1u)) return RGC_CONF_FAULT;
    if (clock && !led) return RGC_CONF_NOT_LED;
    if (!((RG_CFG_PRESENT(W) >> self) & 1u)) return RGC_CONF_HOST;
    if (!(((RG_CFG_INCOMING(W) | RG_CFG_OUTGOING(W)) >> self) & 1u)) return RGC_CONF_DEMOTED; // raft.rs:2609-2622
    return RGC_CONF_DONE;
}

// apply_conf on the cfg word and the flag row: an added slot's byte becomes Progress::new's with recent_active (tracker.rs:385-389);
// every other byte stays. The cells of an added slot are the caller's: match 0, next hi + 1, the four others 0, an empty window.
struct RgConfApply {
    u64 pf;
    u32 cfg, added, removed;
};
RG_D RgConfApply rg_conf_apply(u32 W, u32 old, u64 pf) {
    RgConfApply r;
    r.cfg = (W & RG_CONF_FIELDS) | (old & RG_CONF_KEPT);
    r.added = RG_CFG_PRESENT(W) & ~RG_CFG_PRESENT(old);
    r.removed = RG_CFG_PRESENT(old) & ~RG_CFG_PRESENT(W);
    RG_FOLLOW_UNROLL
    for (u32 s = 0; s < 8; s++)
        if ((r.added >> s) & 1u) pf = (pf & ~(0xffULL << (8 * s))) | ((u64)(RG_STATE_PROBE | RG_PF_RECENT_ACTIVE) << (8 * s));
    r.pf = pf;
    return r;
}

// MajorityConfig::committed_index (src/quorum/majority.rs:70-101) without group commit: the q-th largest of the voters' matched
// indices, q = n / 2 + 1; an empty config gives u64::MAX. `v`: slots without a Progress hold 0 (:80-82).
template <int P> RG_D u64 rg_conf_kth(const u64 (&v)[P], u32 M) {
    u32 n = 0;
    RG_FOLLOW_UNROLL
    for (int i = 0; i < P; i++) n += (M >> i) & 1u;
    if (n == 0) return ~0ULL;
    const u32 q = n / 2u + 1u;
    u64 t = 0;
    RG_FOLLOW_UNROLL
    for (int i = 0; i < P; i++) {
        u32 ge = 0;
        RG_FOLLOW_UNROLL
        for (int j = 0; j < P; j++) ge += (((M >> j) & 1u) && v[j] >= v[i]) ? 1u : 0u;
        const u64 c = (((M >> i) & 1u) && ge >= q) ? v[i] : 0ULL;
        t = c > t ? c : t;
    }
    return t;
}
// JointConfig::committed_index (src/quorum/joint.rs:47-51)
template <int P> RG_D u64 rg_conf_mci(const u64 (&v)[P], u32 incoming, u32 outgoing) {
    const u64 a = rg_conf_kth<P>(v, incoming), b = rg_conf_kth<P>(v, outgoing);
    return a < b ? a : b;
}
// RaftLog::maybe_commit (src/raft_log.rs:487-499), term(mci) == the leader's term restated as lo <= mci <= hi (rg_log_maybe_commit)
RG_D bool rg_conf_log_maybe_commit(u64 mci, u64 &commit, u64 lo, u64 hi) {
    if (mci > commit && mci >= lo && mci <= hi) {
        commit = mci;
        return true;
    }
    return false;
}

// One pass of maybe_send_append(to, allow_empty) (raft.rs:773-819) on one peer's values. `full`: Inflights::full() of its window;
// limit(next, avail): how many of the `avail` entries from `next` one message carries under RG_SEND_BYTES (util::limit_size) -- called
// only with that flag. What it answers: the item (kind 0 = none) and the values behind Progress::update_state(last)
// (progress.rs:231-243): `add` = the caller owes ins.add(last) (a Replicate peer that was sent entries).
struct RgConfPeer {
    u64 next, prev, last;
    u32 pb, kind;
    bool add;
};
template <typename Limit>
RG_D RgConfPeer rg_conf_send_peer(u32 pb, u64 next, u64 prs, bool full, u64 hi, u64 first_index, bool allow_empty, u64 max_entries, u32 flags, u32 esz_w, Limit limit) {
    RgConfPeer r;
    r.pb = pb;
    r.next = next;
    r.prev = r.last = 0;
    r.kind = 0;
    r.add = false;
    const u32 state = pb & RG_PF_STATE_MASK;
    // Progress::is_paused (progress.rs:210-216)
    const bool paused = state == RG_STATE_PROBE ? (pb & RG_PF_PAUSED) != 0 : state == RG_STATE_REPLICATE ? full : true;
    if (paused) return r;
    if (prs != 0) { // pending_request_snapshot: prepare_send_snapshot, which sends only to a recently active peer (raft.rs:665-672)
        if (pb & RG_PF_RECENT_ACTIVE) {
            r.kind = RG_SEND_SNAPSHOT;
            r.prev = next - 1;
            r.last = prs;
        }
        return r;
    }
    const u64 avail = next > hi ? 0 : hi - next + 1;
    if (next <= hi && next < first_index) { // entries() = Err(Compacted) (raft_log.rs:382-389)
        if (allow_empty && (pb & RG_PF_RECENT_ACTIVE)) {
            r.kind = RG_SEND_SNAPSHOT;
            r.prev = next - 1;
            r.last = 0;
        }
        return r;
    }
    if (avail == 0 && !allow_empty) return r;
    u64 take;
    if (flags & RG_SEND_BYTES) {
        if (avail > 1 && max_entries != ~0ULL && avail >= esz_w) { // the sizes have left the device's window: the host's to serve
            r.kind = RG_SEND_HOST;
            r.prev = next - 1;
            r.last = hi;
            return r;
        }
        take = limit(next, avail);
    } else {
        take = (max_entries && avail > max_entries) ? max_entries : avail;
    }
    r.kind = RG_SEND_APPEND;
    r.prev = next - 1;
    r.last = next - 1 + take;
    if (take) { // Progress::update_state(last)
        if (state == RG_STATE_REPLICATE) {
            r.next = next + take; // optimistic_update
            r.add = true;
        } else {
            r.pb = pb | RG_PF_PAUSED;
        }
    }
    return r;
}

// The transfer check (raft.rs:2666-2671) on the NEW word: a transferee that is no voter any more -> the bits cleared,
// RGC_CONF_EV_TRANSFER_ABORTED
RG_D u32 rg_conf_transfer(u32 &cfg) {
    const u32 tr = RG_CFG_TRANSFEREE(cfg);
    if (tr == 0 || (((RG_CFG_INCOMING(cfg) | RG_CFG_OUTGOING(cfg)) >> (tr - 1u)) & 1u)) return 0;
    (void)rg_term_abort_transfer(cfg);
    return RGC_CONF_EV_TRANSFER_ABORTED;
}
