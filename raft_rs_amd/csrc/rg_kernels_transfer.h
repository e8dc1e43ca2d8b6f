// rg_kernels_transfer.h -- kernels of ext_transfer.hip (include/raftgroups_transfer.h): Raft::handle_transfer_leader for many led
// groups in one launch. One lane per record (k_transfer_list) or per group (k_transfer_dense), 256-thread blocks; templated on the
// slot count (rg_with_p) and on the engine's index width (rg_ix32). There is no group-commit parameter: nothing commits.
//
// A selected lane requests everything it will look at BEFORE its first store: the cfg word, the flag row, last_index, the clock
// cell, its tag and the term, and of the TRANSFEREE's slot alone -- never the whole row -- match and, on an engine with device
// Inflights, next, the window cells, dummy_index and (where the flag byte asks for it) pending_request_snapshot. A slot beyond the
// slot count is never used as an index: such a lane loads slot 0 and answers FAULT. The window columns are non-temporal (rg_wld /
// rg_wst), the state columns are not, and same-lane store-to-load ordering through two cache policies is not leaned on -- the
// hazard rg_kernels_promote.h describes: every later phase works on the registers. The only store in front of the column stores
// goes to an Inflights ring word (rg_ins_add), which no kernel of this file loads; the entry-size rows (rg_limit_size) are read-only
// here. No pointer is restrict-qualified.
//
// A lane owes at most ONE item, so the list is compacted by a ballot per wave, the four wave totals through LDS and at most ONE
// atomic per workgroup (the rule of rg_conf_put_items, in its one-item form); a workgroup without items leaves at its first barrier.
// Every lane of a block reaches the barriers, lanes beyond G or n included. Items go to the CALLER's memory. No scratch in any
// instantiation (tests/test_transfer_host.py).
#pragma once
#include "rg_engine.h"
#include "rg_transfer.h"
#include "rg_kernels_conf.h"

// The item one lane owes: kind != 0 = there is one
struct RgTransferLane {
    u64 prev, last;
    u32 kind, slot;
};

// One selected group g (in range), the transferee's slot t (any value) -> the answer; `it` must come in cleared.
template <int P, typename IX>
RG_D rgm_transfer_resp rg_transfer_one(const RgState &st, const RgIns &ins, const RgLeadCols &lc, IX g, u32 t, u64 max_entries, u32 flags, RgTransferLane &it) {
    const bool has_ins = ins.meta != nullptr, clock = lc.cell != nullptr;
    // ---- the loads ----
    const u32 old = rg_at(st.cfg, g);
    const u64 pf0 = rg_at(st.pflags, g);
    const u64 hi = rg_at(st.hi, g);
    u32 cell = 0;
    u64 tag = 0, cur_term = 0;
    if (clock) {
        cell = rg_at(lc.cell, g);
        tag = rg_at(lc.tag, g);
        cur_term = rg_at(st.cur_term, g);
    }
    const u32 ts = t < (u32)P ? t : 0u; // (never an index beyond the slot count)
    const IX o = (IX)ts * (IX)st.stride + g;
    const u64 mt = rg_at(st.match, o);
    u64 nx = 0, hd = 0, tl = 0, first_index = 0, prs = 0;
    u32 meta = 0;
    u32 pb = (u32)(pf0 >> (8 * ts)) & 0xffu;
    if (has_ins) {
        nx = rg_at(st.next, o);
        meta = rg_wld<0>(rg_at(ins.meta, o));
        hd = rg_wld<1>(rg_at(ins.head, o));
        tl = rg_wld<1>(rg_at(ins.tail, o));
        first_index = rg_at(st.dummy_idx, g) + 1;
        if (pb & RG_PF_PEND_RS) prs = rg_at(st.prs, o);
    }
    rgm_transfer_resp a;
    a.last_index = hi;
    a.matched = (t < (u32)P && ((RG_CFG_PRESENT(old) >> ts) & 1u)) ? mt : 0ULL;
    a.cfg = old;
    a.n_items = 0;
    a.events = a.previous = a.reserved = 0;
    a.reserved2 = 0;
    const u32 status = rg_transfer_check(t, old, (u32)P, clock, rg_term_led(cell, tag, cur_term));
    a.status = (uint8_t)status;
    if (status != RGM_XFER_STARTED && status != RGM_XFER_SELF) return a;

    const RgTransferWord w = rg_transfer_word(status, t, old);
    u32 events = w.events;
    bool put_cell = false, moved = false;
    u64 row = pf0;
    if (status == RGM_XFER_STARTED) {
        if (clock) put_cell = rg_transfer_clock(cell, tag, cur_term);
        events |= rg_transfer_first(mt, hi);
        if ((events & RGM_XFER_EV_APPEND) && has_ins) { // send_append(t): ONE maybe_send_append(t, allow_empty = true) (raft.rs:1887)
            u32 start = meta & 0xffffu, count = meta >> 16;
            const RgConfPeer r = rg_conf_send_peer(pb, nx, prs, count == ins.cap, hi, first_index, true, max_entries, flags, ins.esz_w,
                                                   [&](u64 nxt, u64 avail) { return rg_limit_size(ins.esz + (u64)g * ins.esz_w, ins.esz_w - 1u, nxt, avail, max_entries); });
            if (r.add) {
                rg_ins_add(ins, ((u64)g * (u64)P + (u64)ts) * ins.cap, start, count, hd, tl, r.last);
                meta = start | (count << 16);
                nx = r.next;
                moved = true;
            }
            pb = (r.pb & ~RG_PF_INS_FULL) | (((r.pb & RG_PF_STATE_MASK) == RG_STATE_REPLICATE && count == ins.cap) ? RG_PF_INS_FULL : 0u);
            row = (row & ~(0xffULL << (8 * ts))) | ((u64)pb << (8 * ts));
            it.kind = r.kind;
            it.prev = r.prev;
            it.last = r.last;
            it.slot = ts;
        }
    }

    // ---- the stores ----
    if (w.cfg != old) rg_at(st.cfg, g) = w.cfg;
    if (put_cell) rg_at(lc.cell, g) = cell;
    if (row != pf0) rg_at(st.pflags, g) = row;
    if (moved) { // update_state of a Replicate peer: next = last + 1, ins.add(last)
        rg_at(st.next, o) = nx;
        rg_wst<0>(rg_at(ins.meta, o), meta);
        rg_wst<1>(rg_at(ins.head, o), hd);
        rg_wst<1>(rg_at(ins.tail, o), tl);
    }
    a.cfg = w.cfg;
    a.n_items = it.kind ? 1u : 0u;
    a.events = (uint8_t)events;
    a.previous = (uint8_t)w.previous;
    return a;
}

// The block's items into the caller's list. Every lane of the block calls it (barriers); kind 0 = none of this lane's.
RG_D void rg_transfer_put_item(const RgConfItems &o, u64 g, const RgTransferLane &it) {
    __shared__ u32 wave_tot[4];
    __shared__ u32 block_base;
    const bool has = it.kind != 0;
    if (!__syncthreads_or(has)) return; // the common block: no group of it sends
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const u64 b = __ballot(has);
    const u32 before = (u32)__popcll(b & ((1ULL << lane) - 1ULL));
    if (lane == 0) wave_tot[wave] = (u32)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 total = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const u32 n = wave_tot[w];
            wave_tot[w] = total; // exclusive prefix
            total += n;
        }
        block_base = atomicAdd(o.count, total); // (total != 0: the barrier above)
    }
    __syncthreads();
    if (!has) return;
    const u64 k = (u64)block_base + wave_tot[wave] + before;
    if (k < o.cap) {
        rg_send_item r;
        r.group = g;
        r.prev_index = it.prev;
        r.last_index = it.last;
        r.slot = it.slot;
        r.n_msgs = 1;
        r.kind = (uint16_t)it.kind;
        o.items[k] = r;
    }
}

// The sparse form: lane = record (distinct groups, all in range, every slot below the slot count: checked on the host).
template <int P, typename IX>
__global__ __launch_bounds__(256) void k_transfer_list(RgState st, RgIns ins, RgLeadCols lc, const rgm_transfer_rec *recs, u64 n, rgm_transfer_resp *resp, u64 max_entries,
                                                        u32 flags, RgConfItems o) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    RgTransferLane it = {0, 0, 0, 0};
    u64 g = 0;
    if (i < n) {
        g = recs[i].group;
        const u32 t = recs[i].slot;
        resp[i] = rg_transfer_one<P, IX>(st, ins, lc, (IX)g, t, max_entries, flags, it);
    }
    if (o.count) rg_transfer_put_item(o, g, it); // (uniform: an engine without device Inflights has no list)
}

// The dense form: lane = group. An unselected group costs its dev_to byte and its status byte.
template <int P, typename IX>
__global__ __launch_bounds__(256) void k_transfer_dense(RgState st, RgIns ins, RgLeadCols lc, const u8 *to, u8 *status, u8 *events, u64 max_entries, u32 flags, RgConfItems o) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    RgTransferLane it = {0, 0, 0, 0};
    if (g < st.G) {
        const u32 sel = to[g];
        if (!sel) {
            status[g] = (u8)RGM_XFER_NONE;
        } else {
            const rgm_transfer_resp a = rg_transfer_one<P, IX>(st, ins, lc, (IX)g, sel - 1u, max_entries, flags, it);
            status[g] = a.status;
            if (events) events[g] = a.events;
        }
    }
    if (o.count) rg_transfer_put_item(o, g, it);
}
