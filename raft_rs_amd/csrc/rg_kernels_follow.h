// rg_kernels_follow.h -- kernels of abi_follow.hip: the follower's MsgAppend / MsgHeartbeat step, dense (one record per follower
// group) and over a group-sorted list, and the scatter / gather of whole group states; behind rg_follow_gate_enable the same two
// steps behind the term gate of Raft::step (the sparse one with the vote step), the election clock, and the soft cells' scatter / gather
// Included by exactly one abi_*.hip unit (one definition per library).
#pragma once
#include "rg_engine.h"
#include "rg_follow.h"

// the empty log of a zeroed arena: an empty tail is tail_first == last + 1
__global__ __launch_bounds__(256) void k_follow_init(RgFollowCols fc) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    if (g < fc.stride) fc.tail_first[g] = 1;
}

// The dense step: lane = follower group. A lane reads its flag byte first and a workgroup without a message leaves at once.
// The steady case -- an append on the tail, in the tail's term, entries of that term -- is decided on the four hot cells
// (rg_follow_seg answers from the tail before it looks at anything cold) and writes last_index and committed back; the cold
// columns are read only off that path and written only when a term changes or a log is cut. Responses are columns: no LDS, no
// atomics.
__global__ __launch_bounds__(256) void k_follow_dense(RgFollowCols fc, rg_follow_msgs ms, rg_follow_out out) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    const u32 flags = g < fc.n ? ms.flags[g] : 0u;
    if (!__syncthreads_or((int)flags)) {
        if (g < fc.n) out.status[g] = RG_FOLLOW_NONE;
        return;
    }
    if (g >= fc.n) return;
    if (!flags) {
        out.status[g] = RG_FOLLOW_NONE;
        return;
    }
    RgFollowRec m;
    m.index = ms.index[g];
    m.log_term = ms.log_term[g];
    m.commit = ms.commit[g];
    m.ent_term = ms.ent_term[g];
    m.n_entries = ms.n_entries[g];
    m.flags = flags;
    m.ext = nullptr;
    m.n_ext = 0;
    bool ok = flags == RG_FOLLOW_MSG_APPEND || flags == RG_FOLLOW_MSG_HEARTBEAT;
    if (ms.ext && ms.ext_runs) {
        const u64 e = ms.ext[g], cnt = e & 0xffu, off = e >> 8;
        if (cnt) {
            if (off > ms.n_ext || cnt > ms.n_ext - off) ok = false; // outside the side array: never read
            else {
                m.ext = ms.ext_runs + off;
                m.n_ext = (u32)cnt;
            }
        }
    }
    RgFollowView v = rg_follow_open(fc, g);
    rg_follow_resp r;
    if (ok) {
        const RgFollowView o = v;
        r = rg_follow_apply(v, m);
        rg_follow_close(fc, g, v, o);
    } else {
        r = rg_follow_answer(RG_FOLLOW_FAULT, m.index, v.committed);
    }
    out.status[g] = (u8)r.status;
    out.index[g] = r.index;
    out.commit[g] = r.commit;
    out.conflict[g] = r.conflict;
    if (r.status == RG_FOLLOW_REJECT) {
        out.reject_hint[g] = r.reject_hint;
        out.log_term[g] = r.log_term;
    }
}

// The sparse step: lane i applies run i of the group-sorted records -- [run_start[i], run_start[i + 1]) -- in order, the hot
// cells in registers between the records, and writes each response at the record's original position.
__global__ __launch_bounds__(256) void k_follow_list(RgFollowCols fc, const rg_follow_msg *__restrict__ recs, const u32 *__restrict__ orig,
                                                      const u32 *__restrict__ run_start, u32 n_runs, const rg_follow_ent_run *__restrict__ ext,
                                                      rg_follow_resp *resp) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_runs) return;
    const u32 first = run_start[i], last = run_start[i + 1];
    const u64 g = recs[first].group;
    RgFollowView v = rg_follow_open(fc, g);
    const RgFollowView o = v;
    for (u32 k = first; k < last; k++) {
        const rg_follow_msg r = recs[k];
        RgFollowRec m;
        m.index = r.index;
        m.log_term = r.log_term;
        m.commit = r.commit;
        m.ent_term = r.ent_term;
        m.n_entries = r.n_entries;
        m.flags = r.flags;
        m.n_ext = (u32)(r.ext & 0xffu); // (checked against the side array on the host)
        m.ext = m.n_ext ? ext + (r.ext >> 8) : nullptr;
        resp[orig[k]] = rg_follow_apply(v, m);
    }
    rg_follow_close(fc, g, v, o);
}

// rg_follow_write / rg_follow_read: whole group states, one lane each (the states of a write are canonical and name distinct
// groups: checked on the host)
__global__ __launch_bounds__(256) void k_follow_write(RgFollowCols fc, const rg_follow_state *__restrict__ states, u64 n) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) rg_follow_store_state(fc, states[i]);
}
__global__ __launch_bounds__(256) void k_follow_read(RgFollowCols fc, const u64 *__restrict__ groups, u64 n, rg_follow_state *out) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = rg_follow_load_state(fc, groups[i]);
}

// ---- the gated step, the election clock and the soft cells (rg_follow_gate_enable) ----
// a Follower at term 0 that is not promotable, with a drawn timeout
__global__ __launch_bounds__(256) void k_follow_soft_init(RgSoftCols sc, u64 stride) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    if (g < stride) sc.clock[g] = rg_clock_pack(0, 0, rg_follow_draw(sc.cfg.seed, g, 0, 0, sc.cfg.min_timeout, sc.cfg.max_timeout));
}

// The gated dense step: k_follow_dense behind the term gate of Raft::step, APPEND / HEARTBEAT / TOUCH. The steady case -- an
// equal term, the leader the group already has, an append on the tail -- reads the term, lead and clock cells on top of what
// k_follow_dense reads and writes the clock cell (if election_elapsed was not 0); the cold soft cells are read only when a term
// changes or the group has no leader. No LDS, no atomics.
__global__ __launch_bounds__(256) void k_follow_gate_dense(RgFollowCols fc, RgSoftCols sc, rg_follow_msgs ms, const u64 *__restrict__ m_term,
                                                            const u64 *__restrict__ m_from, rg_follow_out out, u8 *gate, u8 *events, u64 *resp_term) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    const u32 flags = g < fc.n ? ms.flags[g] : 0u;
    const bool any = __syncthreads_or((int)flags);
    if (g >= fc.n) return;
    if (!any || !flags) {
        out.status[g] = RG_FOLLOW_NONE;
        gate[g] = RG_GATE_NONE;
        events[g] = 0;
        return;
    }
    RgFollowRec m;
    m.index = ms.index[g];
    m.log_term = ms.log_term[g];
    m.commit = ms.commit[g];
    m.ent_term = ms.ent_term[g];
    m.n_entries = ms.n_entries[g];
    m.flags = flags;
    m.ext = nullptr;
    m.n_ext = 0;
    const u64 term = m_term[g], from = m_from[g];
    bool ok = rg_gate_well_formed(flags, term, from, m.n_entries, 0, false);
    if (ms.ext && ms.ext_runs) {
        const u64 e = ms.ext[g], cnt = e & 0xffu, off = e >> 8;
        if (cnt) {
            if (off > ms.n_ext || cnt > ms.n_ext - off) ok = false; // outside the side array: never read
            else {
                m.ext = ms.ext_runs + off;
                m.n_ext = (u32)cnt;
            }
        }
    }
    RgFollowView v = rg_follow_open(fc, g);
    RgSoftView s = rg_soft_open(sc, g);
    rg_follow_resp r;
    rg_follow_gate_resp a;
    if (ok) {
        const RgFollowView o = v;
        const RgSoftView so = s;
        a = rg_gate_step(sc.cfg, g, s, v, m, term, from, 0, 0, r);
        rg_follow_close(fc, g, v, o);
        rg_soft_close(sc, g, s, so);
    } else {
        r = rg_follow_answer(RG_FOLLOW_FAULT, m.index, v.committed);
        a = rg_gate_answer(s.term, RG_GATE_NONE, 0);
    }
    out.status[g] = (u8)r.status;
    out.index[g] = r.index;
    out.commit[g] = r.commit;
    out.conflict[g] = r.conflict;
    if (r.status == RG_FOLLOW_REJECT) {
        out.reject_hint[g] = r.reject_hint;
        out.log_term[g] = r.log_term;
    }
    gate[g] = (u8)a.gate;
    events[g] = (u8)a.events;
    resp_term[g] = a.term;
}

// The gated sparse step, all five kinds: k_follow_list's shape -- lane i applies run i of the group-sorted records in array
// order, the hot cells of both halves in registers between the records (the records are well-formed: checked on the host).
__global__ __launch_bounds__(256) void k_follow_gate_list(RgFollowCols fc, RgSoftCols sc, const rg_follow_msg *__restrict__ recs,
                                                           const rg_follow_hdr *__restrict__ hdrs, const u32 *__restrict__ orig,
                                                           const u32 *__restrict__ run_start, u32 n_runs, const rg_follow_ent_run *__restrict__ ext,
                                                           rg_follow_resp *resp, rg_follow_gate_resp *gresp) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_runs) return;
    const u32 first = run_start[i], last = run_start[i + 1];
    const u64 g = recs[first].group;
    RgFollowView v = rg_follow_open(fc, g);
    RgSoftView s = rg_soft_open(sc, g);
    const RgFollowView o = v;
    const RgSoftView so = s;
    for (u32 k = first; k < last; k++) {
        const rg_follow_msg r = recs[k];
        const rg_follow_hdr h = hdrs[k];
        RgFollowRec m;
        m.index = r.index;
        m.log_term = r.log_term;
        m.commit = r.commit;
        m.ent_term = r.ent_term;
        m.n_entries = r.n_entries;
        m.flags = r.flags;
        m.n_ext = (u32)(r.ext & 0xffu);
        m.ext = m.n_ext ? ext + (r.ext >> 8) : nullptr;
        rg_follow_resp a;
        gresp[orig[k]] = rg_gate_step(sc.cfg, g, s, v, m, h.term, h.from, h.priority, h.flags, a);
        resp[orig[k]] = a;
    }
    rg_follow_close(fc, g, v, o);
    rg_soft_close(sc, g, s, so);
}

// One Raft::tick of every followed group on its clock cell. Due groups are appended to hup[cap]: a wave counts its due lanes
// with a ballot and claims their places with ONE atomic (counts[1], the groups due); a lane whose place lies within cap writes
// its group and restarts its clock, any other stays due. counts[0] = the groups appended (one more atomic per wave with any).
__global__ __launch_bounds__(256) void k_follow_clock(RgSoftCols sc, u64 n, u64 *hup, u64 cap, unsigned long long *counts) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    bool due = false;
    u32 c = 0, c0 = 0;
    if (g < n) {
        c0 = sc.clock[g];
        c = rg_clock_tick(c0, due);
    }
    const unsigned long long ballot = __ballot(due);
    if (ballot) {
        const u32 lane = threadIdx.x & 63u, leader = (u32)__ffsll(ballot) - 1u, total = (u32)__popcll(ballot);
        unsigned long long base = 0;
        if (lane == leader) {
            base = atomicAdd(&counts[1], (unsigned long long)total);
            const u64 fit = base >= cap ? 0 : (cap - base < total ? cap - base : total);
            if (fit) atomicAdd(&counts[0], (unsigned long long)fit);
        }
        base = __shfl(base, (int)leader);
        const u64 at = base + (u64)__popcll(ballot & ((1ULL << lane) - 1ULL));
        if (due && at < cap) {
            hup[at] = g;
            c &= ~RG_CLOCK_ELAPSED_MAX;
        }
    }
    if (g < n && c != c0) sc.clock[g] = c;
}

__global__ __launch_bounds__(256) void k_follow_soft_write(RgSoftCols sc, const rg_follow_soft *__restrict__ recs, u64 n) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) rg_follow_store_soft(sc, recs[i]);
}
__global__ __launch_bounds__(256) void k_follow_soft_read(RgSoftCols sc, const u64 *__restrict__ groups, u64 n, rg_follow_soft *out) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = rg_follow_load_soft(sc, groups[i]);
}
