// rg_kernels_read.h -- kernels of abi_read.hip: ReadIndex requests and acks over a list of touched groups, the dense ack pass,
// last_pending_request_ctx / pending_read_count
// Included by exactly one abi_*.hip unit (one definition per library).
#pragma once
#include "rg_engine.h"
#include "rg_read.h"

// where the read states go: one compact list, `count` items so far (it may run past `cap` if the library's capacity
// bookkeeping were ever wrong: nothing is written out of bounds then, and rg_read_states reports the loss instead of hiding it)
struct RgReadList {
    rg_read_state *items;
    unsigned long long *count;
    u64 cap;
};
RG_D void rg_read_list_put(const RgReadList &l, u64 k, u64 g, u64 ctx, u64 index) {
    if (k >= l.cap) return;
    rg_read_state s;
    s.group = g;
    s.ctx = ctx;
    s.index = index;
    l.items[k] = s;
}

// A workgroup of 256 lanes reserves room for its lanes' `cnt` states with a scan and ONE atomic (as k_send_compact does);
// returns the list position of this lane's first state. Every lane of the workgroup calls it.
RG_D u64 rg_read_reserve(const RgReadList &l, u32 cnt) {
    __shared__ u32 wave_tot[4];
    __shared__ u64 block_base;
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    u32 incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 v = __shfl_up(incl, d, 64);
        if (lane >= (u32)d) incl += v;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 total = 0;
        for (int w = 0; w < 4; w++) {
            const u32 t = wave_tot[w];
            wave_tot[w] = total;
            total += t;
        }
        block_base = total ? (u64)atomicAdd(l.count, (unsigned long long)total) : 0ULL;
    }
    __syncthreads();
    return block_base + wave_tot[wave] + incl - cnt;
}

// the queue word of group g, with the lazy reset of a term change applied (and stored) -- what every read kernel starts with
// for a group it is going to look at
RG_D RgReadPos rg_read_open(const RgState &st, const RgReadCols &rc, u64 g, u32 qw) {
    RgReadPos p;
    p.n = RG_READ_QW_N(qw);
    p.head = RG_READ_QW_HEAD(qw);
    p.depth = rc.depth;
    u64 qt = rc.qterm[g];
    if (rg_read_sync_term(qt, st.cur_term[g], p)) {
        rc.qterm[g] = qt;
        if (qw != 0) rc.qw[g] = 0;
    }
    return p;
}

// Requests and sparse acks: lane i applies run i of the group-sorted records -- [run_start[i], run_start[i + 1]) -- in order.
// Two walks: over a private copy of the ring to COUNT the states the run emits, then, with the list positions reserved, over the
// columns.
__global__ __launch_bounds__(256) void k_read_list(RgState st, RgReadCols rc, const RgReadRec *recs, const u32 *run_start, u32 n_runs,
                                                    u8 *status, RgReadList list) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    const bool live = i < n_runs;
    u32 first = 0, last = 0, cfg = 0, cnt = 0;
    u64 g = 0, commit = 0, lo = 0;
    RgReadPos p0 = {0, 0, rc.depth};
    if (live) {
        first = run_start[i];
        last = run_start[i + 1];
        g = recs[first].group;
        p0 = rg_read_open(st, rc, g, rc.qw[g]);
        cfg = st.cfg[g];
        commit = st.commit[g];
        lo = st.lo[g];
        RgReadCopy cp;
        const RgReadRing ring = rg_read_ring(rc, g);
        for (u32 j = 0; j < p0.n; j++) {
            const u32 s = rg_read_slot_of(p0, j);
            cp.set(s, ring.ctx(s), ring.idx(s), ring.acks(s));
        }
        RgReadPos p = p0;
        rg_read_walk(cp, p, cfg, commit, lo, recs, first, last, (u8 *)nullptr, [&](u64, u64) { cnt++; });
    }
    u64 k = rg_read_reserve(list, cnt);
    if (!live) return;
    RgReadRing ring = rg_read_ring(rc, g);
    RgReadPos p = p0;
    rg_read_walk(ring, p, cfg, commit, lo, recs, first, last, status, [&](u64 ctx, u64 index) { rg_read_list_put(list, k++, g, ctx, index); });
    if (p.n != p0.n || p.head != p0.head) rc.qw[g] = RG_READ_QW(p.n, p.head);
}

// The dense ack pass: one heartbeat round of every group, lane = group, slots 0..P-1 in order. A lane whose queue is empty is
// done after its queue word (no ctx column, no cfg, no term: an empty queue has nothing a term change could reset), and a
// workgroup of such lanes leaves before the scan. Acks only pop: the states a lane emits are the first `cnt` entries its queue
// had, so ONE walk suffices -- count, reserve, then copy those entries out of the ring (a pop leaves the ring's cells alone).
template <int P> __global__ __launch_bounds__(256) void k_read_acks_dense(RgState st, RgReadCols rc, const u64 *__restrict__ dev_ctx, RgReadList list) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    const u32 qw = g < st.G ? rc.qw[g] : 0u;
    if (!__syncthreads_or((int)RG_READ_QW_N(qw))) return;
    u32 cnt = 0, head0 = 0;
    if (RG_READ_QW_N(qw)) {
        u64 c[P];
#pragma unroll
        for (int s = 0; s < P; s++) c[s] = dev_ctx[(u64)s * st.stride + g];
        RgReadPos p = rg_read_open(st, rc, g, qw);
        if (p.n) {
            const u32 cfg = st.cfg[g];
            const u32 n0 = p.n;
            head0 = p.head;
            RgReadRing ring = rg_read_ring(rc, g);
#pragma unroll
            for (int s = 0; s < P; s++) rg_read_recv_ack(ring, p, cfg, (u32)s, c[s], 0u, [](u64, u64) {});
            cnt = n0 - p.n;
            if (cnt) rc.qw[g] = RG_READ_QW(p.n, p.head);
        }
    }
    u64 k = rg_read_reserve(list, cnt);
    if (!cnt) return;
    const RgReadRing ring = rg_read_ring(rc, g);
    RgReadPos p = {cnt, head0, rc.depth};
    for (u32 j = 0; j < cnt; j++) {
        const u32 s = rg_read_slot_of(p, j);
        rg_read_list_put(list, k++, g, ring.ctx(s), ring.idx(s));
    }
}

// last_pending_request_ctx (0 = none) and pending_read_count of every group; either destination may be null
__global__ __launch_bounds__(256) void k_read_pending(RgState st, RgReadCols rc, u64 *last_ctx, u8 *counts) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    if (g >= st.G) return;
    const u32 qw = rc.qw[g];
    u64 ctx = 0;
    u32 n = 0;
    if (RG_READ_QW_N(qw)) {
        const RgReadPos p = rg_read_open(st, rc, g, qw);
        n = p.n;
        if (n) ctx = rg_read_ring(rc, g).ctx(rg_read_slot_of(p, n - 1u));
    }
    if (last_ctx) last_ctx[g] = ctx;
    if (counts) counts[g] = (u8)n;
}
