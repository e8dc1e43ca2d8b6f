// rg_read.h -- ReadIndex: the per-group arithmetic of the pending-read queue (include/raftgroups.h: "ReadIndex").
//
// The engine's restatement of src/read_only.rs:86-139 (add_request / recv_ack / advance / last_pending_request_ctx) and of the
// three places of src/raft.rs that drive it: the MsgReadIndex step (:2056-2091), the read-only half of
// handle_heartbeat_response (:1805-1818) and the re-check of post_conf_change (:2650-2664). Citations are relative to the
// pingcap/raft-rs v0.6.0 tree. The reference keys its queue by the request's context BYTES; here the host hands over a 64-bit
// handle per context (non-zero, unique among a group's pending reads; 0 = m.context.is_empty()), and `acks` is a slot bitmask
// instead of a HashSet of ids. What is left is integer work on one group.
//
// Host/device-clean: the kernels (rg_kernels_read.h) include it behind rg_common.h; a host program includes it ALONE and compiles
// it with any C++17 compiler (tests/host_check/read_twin.cpp is checked that way against tests/readonly_model.py, sanitizers
// included) -- nothing below needs the HIP headers.
#pragma once
#include <stdint.h>

#include "../../include/raftgroups.h"

#ifndef RG_D /* stand-alone: a plain host build */
typedef uint64_t u64;
typedef unsigned int u32;
typedef unsigned char u8;
#define RG_D static inline
#define RG_READ_M inline /* (member functions) */
#else
#define RG_READ_M RG_D
#endif

// The queue columns (an optional arena, absent until rg_read_index_enable). The queue of a group is a ring of `depth` entries:
// entry j (0 = oldest) lives in ring slot (head + j) % depth, and ring slot s of group g at [s * stride + g] of each column.
struct RgReadCols {
    u32 *qw;     // [G] count | head << 8: the ONE word the dense ack pass reads of a group with nothing pending
    u64 *qterm;  // [G] RG_COL_CUR_TERM as the queue last saw it (the lazy form of Raft::reset's `ReadOnly::new`, raft.rs:957)
    u64 *ctx;    // [depth][stride] the request's handle
    u64 *idx;    // [depth][stride] ReadIndexStatus.index: raft_log.committed when the request arrived
    u8 *acks;    // [depth][stride] ReadIndexStatus.acks as a slot bitmask
    u64 stride;
    u32 depth;
};

#define RG_READ_QW(n, head) ((u32)(n) | ((u32)(head) << 8))
#define RG_READ_QW_N(w) ((u32)(w) & 0xffu)
#define RG_READ_QW_HEAD(w) (((u32)(w) >> 8) & 0xffu)
#define RG_READ_REC_REQUEST 0x80000000u /* internal record flag: a MsgReadIndex (else a heartbeat response's read-only half) */

// One group's ring in the columns ...
struct RgReadRing {
    u64 *c, *i;
    u8 *a;
    u64 stride;
    RG_READ_M u64 ctx(u32 s) const { return c[(u64)s * stride]; }
    RG_READ_M u64 idx(u32 s) const { return i[(u64)s * stride]; }
    RG_READ_M u32 acks(u32 s) const { return a[(u64)s * stride]; }
    RG_READ_M void set_acks(u32 s, u32 v) { a[(u64)s * stride] = (u8)v; }
    RG_READ_M void set(u32 s, u64 cx, u64 ix, u32 ak) {
        c[(u64)s * stride] = cx;
        i[(u64)s * stride] = ix;
        a[(u64)s * stride] = (u8)ak;
    }
};
RG_D RgReadRing rg_read_ring(const RgReadCols &q, u64 g) {
    RgReadRing r;
    r.c = q.ctx + g;
    r.i = q.idx + g;
    r.a = q.acks + g;
    r.stride = q.stride;
    return r;
}
// ... and a private copy of it: the list kernel walks a group's records twice, first over a copy to learn how many read states
// the walk emits (so that a workgroup reserves its part of the list with one atomic), then over the columns.
struct RgReadCopy {
    u64 c[RG_READ_MAX_DEPTH], i[RG_READ_MAX_DEPTH];
    u8 a[RG_READ_MAX_DEPTH];
    RG_READ_M u64 ctx(u32 s) const { return c[s]; }
    RG_READ_M u64 idx(u32 s) const { return i[s]; }
    RG_READ_M u32 acks(u32 s) const { return a[s]; }
    RG_READ_M void set_acks(u32 s, u32 v) { a[s] = (u8)v; }
    RG_READ_M void set(u32 s, u64 cx, u64 ix, u32 ak) {
        c[s] = cx;
        i[s] = ix;
        a[s] = (u8)ak;
    }
};

// the queue's bookkeeping while a lane works on it (RgReadCols::qw unpacked)
struct RgReadPos {
    u32 n, head, depth;
};
RG_D u32 rg_read_slot_of(const RgReadPos &p, u32 j) {
    const u32 s = p.head + j;
    return s >= p.depth ? s - p.depth : s;
}

RG_D u32 rg_read_popcount(u32 x) { return (u32)__builtin_popcount(x); }
// ProgressTracker::has_quorum(acks) (src/tracker.rs:367-372): vote_result over the voters with "in the set" = yes and nobody
// voting no, == Won. MajorityConfig::vote_result (src/quorum/majority.rs:130-154): an empty config wins; JointConfig
// (src/quorum/joint.rs:56-67): both halves must. A learner's bit is in neither mask, so it never counts.
RG_D bool rg_read_majority_has(u32 voters, u32 acks) {
    const u32 n = rg_read_popcount(voters);
    return n == 0 || rg_read_popcount(voters & acks) >= n / 2u + 1u;
}
RG_D bool rg_read_has_quorum(u32 cfg, u32 acks) {
    return rg_read_majority_has(RG_CFG_INCOMING(cfg), acks) && rg_read_majority_has(RG_CFG_OUTGOING(cfg), acks);
}
// ProgressTracker::is_singleton -> JointConfig::is_singleton (src/quorum/joint.rs:77)
RG_D bool rg_read_is_singleton(u32 cfg) { return rg_read_popcount(RG_CFG_INCOMING(cfg)) == 1u && RG_CFG_OUTGOING(cfg) == 0u; }

// Raft::reset replaces the ReadOnly at every term change (raft.rs:957) without answering anybody. Done lazily, by whoever
// touches the queue next: the ticks never see these columns. Returns true when the queue was emptied.
RG_D bool rg_read_sync_term(u64 &qterm, u64 cur_term, RgReadPos &p) {
    if (qterm == cur_term) return false;
    qterm = cur_term;
    p.n = 0;
    p.head = 0;
    return true;
}

// position in the queue (0 = oldest) of the pending read `ctx`, or -1 (pending_read_index.contains_key)
template <typename Q> RG_D int rg_read_find(const Q &q, const RgReadPos &p, u64 ctx) {
    for (u32 j = 0; j < p.n; j++)
        if (q.ctx(rg_read_slot_of(p, j)) == ctx) return (int)j;
    return -1;
}

// ReadOnly::advance (read_only.rs:114-129): pop from the head through position `pos`, one read state per popped entry, in
// queue order, each with the index it was queued with. emit(ctx, index).
template <typename Q, typename EMIT> RG_D void rg_read_advance(const Q &q, RgReadPos &p, u32 pos, EMIT &&emit) {
    for (u32 j = 0; j <= pos; j++) {
        emit(q.ctx(p.head), q.idx(p.head));
        p.head = p.head + 1u == p.depth ? 0u : p.head + 1u;
    }
    p.n -= pos + 1u;
}

// The read-only half of handle_heartbeat_response (raft.rs:1805-1818): recv_ack, has_quorum, advance. `flags` with
// RG_READ_ACK_LAST_SELF: the re-check of post_conf_change (raft.rs:2650-2664) instead -- the LAST pending read is acked from the
// leader's own slot (`slot` and `ctx` of the record are not looked at).
template <typename Q, typename EMIT> RG_D void rg_read_recv_ack(Q &q, RgReadPos &p, u32 cfg, u32 slot, u64 ctx, u32 flags, EMIT &&emit) {
    int pos;
    if (flags & RG_READ_ACK_LAST_SELF) {
        if (p.n == 0) return; // last_pending_request_ctx() == None
        pos = (int)p.n - 1;
        slot = RG_CFG_SELF(cfg);
    } else {
        if (ctx == 0) return;                                                   // m.context.is_empty()
        if (slot >= RG_MAX_SLOTS || !((RG_CFG_PRESENT(cfg) >> slot) & 1u)) return; // "no progress available" (raft.rs:1779-1789)
        pos = rg_read_find(q, p, ctx);
        if (pos < 0) return; // recv_ack: None
    }
    const u32 s = rg_read_slot_of(p, (u32)pos);
    const u32 acks = q.acks(s) | (1u << slot);
    q.set_acks(s, acks);
    if (!rg_read_has_quorum(cfg, acks)) return;
    rg_read_advance(q, p, (u32)pos, emit);
}

// The MsgReadIndex step of a leader (raft.rs:2056-2091), in the reference's order. Returns RG_READ_*.
template <typename Q, typename EMIT>
RG_D u32 rg_read_request(Q &q, RgReadPos &p, u32 cfg, u64 commit, u64 term_lo, u64 ctx, bool lease, EMIT &&emit) {
    // commit_to_current_term (raft.rs:581): term(committed) == self.term, i.e. the commit index has reached the leader's own
    // entries [RG_COL_TERM_LO, RG_COL_TERM_HI]
    if (commit < term_lo) return RG_READ_NOT_READY;
    if (rg_read_is_singleton(cfg) || lease) { // handle_ready_read_index at once (raft.rs:2063-2069, :2083-2088)
        emit(ctx, commit);
        return RG_READ_READY;
    }
    if (rg_read_find(q, p, ctx) >= 0) return RG_READ_DUPLICATE; // add_request returns early (read_only.rs:89-91)
    if (p.n == p.depth) return RG_READ_FULL;                    // the one bound the reference does not have
    q.set(rg_read_slot_of(p, p.n), ctx, commit, 1u << RG_CFG_SELF(cfg));
    p.n++;
    return RG_READ_QUEUED;
}

// one record of a batch, as the library hands them to the list kernel: sorted by group (stable: arrival order inside a group)
struct RgReadRec {
    u64 group, ctx;
    u32 slot;
    u32 flags; // RG_READ_ACK_LAST_SELF | RG_READ_LEASE << 8 | RG_READ_REC_REQUEST
    u32 orig;  // position in the caller's array (where a request's status goes)
    u32 pad;
};
#define RG_READ_REC_LEASE 0x100u

// A group's run of records [first, last) applied in order. status (may be null) is indexed by RgReadRec::orig.
template <typename Q, typename EMIT>
RG_D void rg_read_walk(Q &q, RgReadPos &p, u32 cfg, u64 commit, u64 term_lo, const RgReadRec *recs, u32 first, u32 last, u8 *status,
                       EMIT &&emit) {
    for (u32 k = first; k < last; k++) {
        const RgReadRec r = recs[k];
        if (r.flags & RG_READ_REC_REQUEST) {
            const u32 s = rg_read_request(q, p, cfg, commit, term_lo, r.ctx, (r.flags & RG_READ_REC_LEASE) != 0, emit);
            if (status) status[r.orig] = (u8)s;
        } else {
            rg_read_recv_ack(q, p, cfg, r.slot, r.ctx, r.flags & RG_READ_ACK_LAST_SELF, emit);
        }
    }
}
