// rg_kernels_follow.h -- kernels of abi_follow.hip: the follower's MsgAppend / MsgHeartbeat step, dense (one record per follower
// group) and over a group-sorted list, and the scatter / gather of whole group states
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
