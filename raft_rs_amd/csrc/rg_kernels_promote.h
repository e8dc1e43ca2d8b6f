// rg_kernels_promote.h -- kernels of ext_handoff.hip (include/raftgroups_handoff.h): the promotion into an engine with device
// Inflights. One lane per record (the sparse form) or per followed group (the dense form), 256-thread blocks; templated on the slot
// count (rg_with_p, as k_send_appends) and on the engine's index width (RG_LAUNCH_IX's, as the hand-off kernels).
//
// A selected lane runs three halves, each with all its loads before its first store:
//   1. the promotion: rg_handoff_promote_one (rg_kernels_handoff.h), unchanged -- the refusals, the import, become_leader, the reset;
//   2. the size record of the empty entry (engines with rg_log_sizes_enable): ONE load, the preceding cumulative cell, ONE store;
//   3. the windows and the first appends: stores only (rg_promote.h: the stage of a group whose every Progress was reset a moment
//      ago is a closed form of the cfg word and the flag row).
// THE ORDERING HAZARD -- a stage half that reads cfg, the flag row, next, match, TERM_HI, DUMMY_INDEX, the window columns and the size
// row through memory right behind the stores of the promotion half of the same lane -- is answered by HANDING THE STAGE THE
// REGISTERS: half 3 loads nothing. The cfg word and the flag row are requested once, together with the promotion's own loads and
// before its first store (the compiler merges them with the loads rg_handoff_promote_one issues); what the promotion makes of them
// is recomputed from those registers (rg_handoff_progress is arithmetic), last_index and the term come back in the answer. The
// alternative -- rg_group_send behind the promotion, no pointer __restrict__ -- costs a selected lane a second round trip of
// scattered loads for cells whose values it holds, and leans on same-lane store-to-load ordering through two cache policies
// (the window columns are non-temporal). No pointer below is __restrict__ all the same: the two halves write cells half 1 read.
// The window's head / tail cells keep what they held (an empty window's cells are meaningless: rg_send_serve rewrites them with
// the value it read); no ring word is touched.
//
// The item list is compacted as k_send_appends compacts it -- wave prefix sums by shuffles, the four wave totals through LDS, at
// most ONE atomic per workgroup -- and a workgroup without items leaves at its first barrier: no atomic, no scan. Items go to the
// CALLER's memory: the engine's own list, counter and item columns are not touched. No scratch in any instantiation
// (tests/test_promote_send_host.py).
#pragma once
#include "rg_kernels_handoff.h"
#include "rg_promote.h"

// Where the items go: `cap` of them are written, *count is the total (the rule of rg_send_items)
struct RgPromoteItems {
    rg_send_item *items;
    u64 cap;
    u32 *count;
};

// Halves 1-3 for follow group g, lead group L (both in range) -> the answer; `n_items` / `peers`: the items this lane owes
template <int P, typename IX>
RG_D rg_handoff_resp rg_promote_send_one(const RgState &st, const RgIns &ins, u32 *esz, const RgFollowCols &fc, const RgSoftCols &sc, const RgElectCols &ec, u64 g,
                                         IX L, const u64 *persisted_cell, u32 &peers, u32 &n_items) {
    const u32 cfg = rg_at(st.cfg, L);
    const u64 pf = rg_at(st.pflags, L);
    const rg_handoff_resp a = rg_handoff_promote_one<IX>(st, fc, sc, ec, (u32)P, g, L, persisted_cell);
    if (a.status != RG_HANDOFF_DONE) return a;
    const u64 hi = a.last_index;
    if (esz) { // esz[L][hi & mask] = esz[L][(hi - 1) & mask] + Entry::compute_size({term, hi}), before any stage can read it
        u32 *row = esz + (u64)L * ins.esz_w;
        const u32 mask = ins.esz_w - 1u;
        const u32 before = row[(u32)(hi - 1) & mask];
        row[(u32)hi & mask] = before + rg_promote_empty_entry_size(a.term, hi);
    }
    const RgHandoffProgress pr = rg_handoff_progress(pf, cfg, (u32)P, hi - 1);
    const RgPromoteSend ps = rg_promote_send(pr.pf, pr.cfg, (u32)P);
#pragma unroll
    for (int s = 0; s < P; s++)
        if ((ps.windows >> s) & 1u) rg_wst<0>(rg_at(ins.meta, (IX)s * (IX)st.stride + L), 0u);
    if (ps.pf != pr.pf) rg_at(st.pflags, L) = ps.pf;
    peers = ps.peers;
    n_items = ps.n_items;
    return a;
}

// The block's items into the caller's list. Every lane of the block calls it (barriers); `n_items` 0 = none of this lane's.
template <int P> RG_D void rg_promote_put_items(const RgPromoteItems &o, u64 L, u64 hi, u32 peers, u32 n_items) {
    __shared__ u32 wave_tot[4];
    __shared__ u32 block_base;
    if (!__syncthreads_or(n_items != 0)) return; // the common block: nobody was promoted
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    u32 incl = n_items;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 v = __shfl_up(incl, d, 64);
        if (lane >= (u32)d) incl += v;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 total = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const u32 t = wave_tot[w];
            wave_tot[w] = total; // exclusive prefix
            total += t;
        }
        block_base = atomicAdd(o.count, total); // (total != 0: the barrier above)
    }
    __syncthreads();
    if (n_items == 0) return;
    u64 k = (u64)block_base + wave_tot[wave] + incl - n_items;
#pragma unroll
    for (int s = 0; s < P; s++) {
        if (!((peers >> s) & 1u)) continue;
        if (k < o.cap) {
            rg_send_item r;
            r.group = L;
            r.prev_index = hi - 1;
            r.last_index = hi;
            r.slot = (u32)s;
            r.n_msgs = 1;
            r.kind = (uint16_t)RG_SEND_APPEND;
            o.items[k] = r;
        }
        k++;
    }
}

// The sparse form: lane = record (distinct follow groups, distinct lead groups, all in range: checked on the host).
template <int P, typename IX>
__global__ __launch_bounds__(256) void k_promote_send_list(RgState st, RgIns ins, u32 *esz, RgFollowCols fc, RgSoftCols sc, RgElectCols ec, const rg_handoff_rec *recs, u64 n,
                                                            rg_handoff_resp *resp, RgPromoteItems o) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    u32 peers = 0, n_items = 0;
    u64 L = 0, hi = 0;
    if (i < n) {
        L = recs[i].lead_group;
        const rg_handoff_resp a = rg_promote_send_one<P, IX>(st, ins, esz, fc, sc, ec, recs[i].follow_group, (IX)L, &recs[i].persisted, peers, n_items);
        hi = a.last_index;
        resp[i] = a;
    }
    rg_promote_put_items<P>(o, L, hi, peers, n_items);
}

// The dense form: lane = followed group. An unselected group costs its selector byte and its status byte.
template <int P, typename IX>
__global__ __launch_bounds__(256) void k_promote_send_dense(RgState st, RgIns ins, u32 *esz, RgFollowCols fc, RgSoftCols sc, RgElectCols ec, const u8 *result,
                                                             const u64 *lead, const u64 *persisted, rg_handoff_out out, RgPromoteItems o) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    u32 peers = 0, n_items = 0;
    u64 L = 0, hi = 0;
    if (g < fc.n) {
        if (result[g] != RG_ELECT_WON) {
            out.status[g] = RG_HANDOFF_NONE;
        } else if ((L = lead[g]) >= st.G) { // not a group of the engine: nothing is read or written through it
            out.status[g] = RG_HANDOFF_FAULT;
        } else {
            const rg_handoff_resp a = rg_promote_send_one<P, IX>(st, ins, esz, fc, sc, ec, g, (IX)L, persisted ? persisted + g : nullptr, peers, n_items);
            hi = a.last_index;
            rg_handoff_put(out, g, a);
        }
    }
    rg_promote_put_items<P>(o, L, hi, peers, n_items);
}
