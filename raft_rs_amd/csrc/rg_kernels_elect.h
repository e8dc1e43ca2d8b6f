// rg_kernels_elect.h -- kernels of abi_elect.hip: the candidate half on the follower arena. MsgHup for a device list of groups
// (what rg_follow_clock wrote), campaign / vote-response records over a group-sorted list, one vote response per followed group,
// and the scatter / gather of the election cells. All of them run rg_elect_step (rg_elect.h) on the three layers.
// Included by exactly one abi_*.hip unit (one definition per library).
#pragma once
#include "rg_engine.h"
#include "rg_elect.h"

// one answer into the columns, at position i (a list position or a group)
RG_D void rg_elect_put(const rg_follow_elect_out &out, u64 i, const rg_follow_elect_resp &a, bool with_term) {
    out.result[i] = (u8)a.result;
    out.events[i] = (u8)a.events;
    out.status[i] = (u8)a.status;
    if (with_term) out.term[i] = a.term;
    if (a.result == RG_ELECT_REQUESTS) {
        out.req_kind[i] = (u8)a.req_kind;
        out.targets[i] = (u8)a.targets;
        out.flags[i] = (u8)a.flags;
        out.req_term[i] = a.req_term;
        out.req_index[i] = a.req_index;
        out.req_log_term[i] = a.req_log_term;
        out.req_commit[i] = a.req_commit;
        out.req_commit_term[i] = a.req_commit_term;
    }
}

// The storm path: lane = entry of the device list, min(*n_dev, cap) of them. The cells of the three layers are gathered through
// the list (the clock appends in wave order, so a wave's groups are mostly neighbours). The list names no group twice (the
// caller's contract): no two lanes work on one group. No LDS, no atomics.
__global__ __launch_bounds__(256) void k_elect_campaign(RgFollowCols fc, RgSoftCols sc, RgElectCols ec, const u64 *__restrict__ groups,
                                                         const u64 *__restrict__ n_dev, u64 cap, const u8 *__restrict__ block, rg_follow_elect_out out) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    u64 n = *n_dev;
    if (n > cap) n = cap;
    if (i >= n) return;
    const u64 g = groups[i];
    if (g >= fc.n) { // not a followed group: nothing is read or written through it
        rg_elect_put(out, i, rg_elect_answer(0, RG_ELECT_NONE, 0, RG_FOLLOW_FAULT), true);
        return;
    }
    RgElectRec m;
    m.term = m.from = m.commit = m.commit_term = 0;
    m.kind = RG_ELECT_K_HUP;
    m.flags = (block && block[g]) ? RG_ELECT_F_BLOCKED : 0u;
    RgFollowView v = rg_follow_open(fc, g);
    RgSoftView s = rg_soft_open(sc, g);
    RgElectView e = rg_elect_open(ec, g);
    const RgFollowView o = v;
    const RgSoftView so = s;
    const RgElectView eo = e;
    const rg_follow_elect_resp a = rg_elect_step(sc.cfg, g, s, v, e, m);
    rg_follow_close(fc, g, v, o);
    rg_soft_close(sc, g, s, so);
    rg_elect_close(ec, g, e, eo);
    rg_elect_put(out, i, a, true);
}

// The sparse records (rg_follow_campaign: runs of one record; rg_follow_vote_resps): k_follow_gate_list's shape -- lane i
// applies run i of the group-sorted records in array order, the hot cells of the three layers in registers between a group's
// records (the records are well-formed: checked on the host).
__global__ __launch_bounds__(256) void k_elect_list(RgFollowCols fc, RgSoftCols sc, RgElectCols ec, const RgElectStaged *__restrict__ recs,
                                                     const u32 *__restrict__ orig, const u32 *__restrict__ run_start, u32 n_runs,
                                                     rg_follow_elect_resp *resp) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_runs) return;
    const u32 first = run_start[i], last = run_start[i + 1];
    const u64 g = recs[first].group;
    RgFollowView v = rg_follow_open(fc, g);
    RgSoftView s = rg_soft_open(sc, g);
    RgElectView e = rg_elect_open(ec, g);
    const RgFollowView o = v;
    const RgSoftView so = s;
    const RgElectView eo = e;
    for (u32 k = first; k < last; k++) {
        const RgElectRec m = recs[k].r;
        resp[orig[k]] = rg_elect_step(sc.cfg, g, s, v, e, m);
    }
    rg_follow_close(fc, g, v, o);
    rg_soft_close(sc, g, s, so);
    rg_elect_close(ec, g, e, eo);
}

// The dense response round: lane = followed group, k_follow_gate_dense's shape. A lane reads its kind byte first and a
// workgroup without a message writes its three answer bytes per group and leaves. No LDS beyond the barrier, no atomics.
__global__ __launch_bounds__(256) void k_elect_dense(RgFollowCols fc, RgSoftCols sc, RgElectCols ec, rg_follow_vote_cols ms, rg_follow_elect_out out) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    const u32 kind = g < fc.n ? ms.kind[g] : 0u;
    const bool any = __syncthreads_or((int)kind);
    if (g >= fc.n) return;
    if (!any || !kind) {
        out.result[g] = RG_ELECT_NONE;
        out.events[g] = 0;
        out.status[g] = RG_FOLLOW_NONE;
        return;
    }
    RgElectRec m;
    m.term = ms.term[g];
    m.from = ms.slot[g];
    m.commit = ms.commit[g];
    m.commit_term = ms.commit_term[g];
    m.kind = kind;
    m.flags = ms.reject[g] ? RG_ELECT_F_REJECT : 0u;
    if (!rg_elect_resp_well_formed(kind, m.term, (u32)m.from)) {
        rg_elect_put(out, g, rg_elect_answer(sc.term[g], RG_ELECT_NONE, 0, RG_FOLLOW_FAULT), true);
        return;
    }
    RgFollowView v = rg_follow_open(fc, g);
    RgSoftView s = rg_soft_open(sc, g);
    RgElectView e = rg_elect_open(ec, g);
    const RgFollowView o = v;
    const RgSoftView so = s;
    const RgElectView eo = e;
    const rg_follow_elect_resp a = rg_elect_step(sc.cfg, g, s, v, e, m);
    rg_follow_close(fc, g, v, o);
    rg_soft_close(sc, g, s, so);
    rg_elect_close(ec, g, e, eo);
    rg_elect_put(out, g, a, true);
}

// rg_follow_elect_write / rg_follow_elect_read: one lane per record (distinct groups, checked on the host)
__global__ __launch_bounds__(256) void k_elect_write(RgElectCols ec, const rg_follow_elect *__restrict__ recs, u64 n) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) rg_follow_store_elect(ec, recs[i]);
}
__global__ __launch_bounds__(256) void k_elect_read(RgElectCols ec, const u8 *__restrict__ role, const u64 *__restrict__ groups, u64 n,
                                                     rg_follow_elect *out) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = rg_follow_load_elect(ec, role, groups[i]);
}
