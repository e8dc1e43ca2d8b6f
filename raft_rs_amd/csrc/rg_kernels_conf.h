// rg_kernels_conf.h -- kernels of ext_conf.hip (include/raftgroups_conf.h): apply_conf and post_conf_change for many led groups in
// one launch. One lane per record (k_conf_list) or per group (k_conf_dense), 256-thread blocks; templated on the slot count
// (rg_with_p), on the engine's index width (rg_ix32) and on group commit (GC, chosen from any_group_commit as k_recompute's: the
// common instantiation does not carry rg_mci_group).
//
// A selected lane requests everything it will look at BEFORE its first store to a column: the cfg word, the flag row, last_index,
// term_lo, commit, dummy_index, the clock cell, its tag and the term, and per slot match, next and -- on an engine with device
// Inflights -- the window cells; behind the checks, still in front of every column store, the own slot's committed_index and, where
// the flag row or the cfg word asks for them, pending_request_snapshot and commit_group_id. Every later phase works on those
// REGISTERS: the send phase reads nothing through memory that apply_conf decides in the same lane -- an added slot's cells are known
// without a load (Progress::new) and override what was loaded. This is the ordering hazard rg_kernels_promote.h describes: the window
// columns are non-temporal (rg_wld / rg_wst), the state columns are not, and same-lane store-to-load ordering through two cache
// policies is not leaned on. The only stores in front of the column stores go to Inflights ring words (rg_ins_add), which no kernel
// of this file loads; the entry-size rows (rg_limit_size) are read-only here. No pointer is __restrict__.
//
// The item list is compacted as rg_promote_put_items compacts it -- wave prefix sums by shuffles, the four wave totals through LDS, at
// most ONE atomic per workgroup -- and a workgroup without items leaves at its first barrier. Every lane of a block reaches the
// barriers, lanes beyond G or n included. Items go to the CALLER's memory. No scratch in any instantiation
// (tests/test_conf_change_host.py).
#pragma once
#include "rg_engine.h"
#include "rg_conf.h"

// Where the items go: `cap` of them are written, *count is the total (the rule of rg_send_items)
struct RgConfItems {
    rg_send_item *items;
    u64 cap;
    u32 *count;
};
// The items one lane owes: kind[s] != 0 = slot s gets one
template <int P> struct RgConfLane {
    u64 prev[P], last[P];
    u32 kind[P];
    u32 n_items;
};

// One selected group g (in range), the record's word W -> the answer; `it` must come in cleared.
template <int P, typename IX, bool GC>
RG_D rgc_conf_resp rg_conf_one(const RgState &st, const RgIns &ins, const RgLeadCols &lc, IX g, u32 W, u64 max_entries, u32 flags, RgConfLane<P> &it) {
    const bool has_ins = ins.meta != nullptr, clock = lc.cell != nullptr;
    // ---- the loads ----
    const u32 old = rg_at(st.cfg, g);
    const u64 pf0 = rg_at(st.pflags, g);
    const u64 hi = rg_at(st.hi, g), lo = rg_at(st.lo, g), commit0 = rg_at(st.commit, g);
    const u64 first_index = rg_at(st.dummy_idx, g) + 1;
    u32 cell = 0;
    u64 tag = 0, cur_term = 0;
    if (clock) {
        cell = rg_at(lc.cell, g);
        tag = rg_at(lc.tag, g);
        cur_term = rg_at(st.cur_term, g);
    }
    const u32 pub0 = rg_pub_load(st, g);
    u64 mt[P], nx[P], hd[P], tl[P];
    u32 meta[P];
#pragma unroll
    for (int s = 0; s < P; s++) {
        const IX o = (IX)s * (IX)st.stride + g;
        mt[s] = rg_at(st.match, o);
        nx[s] = 0;
        hd[s] = tl[s] = 0;
        meta[s] = 0;
        if (has_ins) {
            nx[s] = rg_at(st.next, o);
            meta[s] = rg_wld<0>(rg_at(ins.meta, o));
            hd[s] = rg_wld<1>(rg_at(ins.head, o));
            tl[s] = rg_wld<1>(rg_at(ins.tail, o));
        }
    }
    rgc_conf_resp a;
    a.commit = commit0;
    a.last_index = hi;
    a.cfg = old;
    a.out = 0;
    a.n_items = 0;
    a.events = a.added = a.removed = 0;
    const u32 status = rg_conf_check(W, old, (u32)P, clock, rg_term_led(cell, tag, cur_term));
    a.status = (uint8_t)status;
    if (status != RGC_CONF_DONE && status != RGC_CONF_DEMOTED) return a;

    const u32 self = RG_CFG_SELF(old);
    RgConfApply ap = rg_conf_apply(W, old, pf0);
    const u32 Wp = RG_CFG_PRESENT(W);
    u64 commit = commit0;
    u32 events = 0, dirty = 0;
    u64 row = ap.pf;
    u64 prc_self = 0;
    if (status == RGC_CONF_DONE) {
        prc_self = rg_at(st.prc, (IX)self * (IX)st.stride + g);
        // ---- maybe_commit on the new configuration (raft.rs:2630) ----
        u64 v[P];
#pragma unroll
        for (int s = 0; s < P; s++) v[s] = (((Wp & ~ap.added) >> s) & 1u) ? mt[s] : 0ULL; // (absent voters ack 0; a new Progress has matched 0)
        u64 mci;
        if (GC && (ap.cfg & RG_CFG_GROUP_COMMIT)) {
            u64 gidv[P];
#pragma unroll
            for (int s = 0; s < P; s++) gidv[s] = (((Wp & ~ap.added) >> s) & 1u) ? rg_at(st.gid, (IX)s * (IX)st.stride + g) : 0ULL;
            bool used;
            mci = rg_mci_group<P>(v, gidv, RG_CFG_INCOMING(W), RG_CFG_OUTGOING(W), used);
        } else {
            mci = rg_conf_mci<P>(v, RG_CFG_INCOMING(W), RG_CFG_OUTGOING(W));
        }
        const bool committed = rg_conf_log_maybe_commit(mci, commit, lo, hi);
        if (committed) events |= RGC_CONF_EV_COMMITTED;
        // ---- bcast_append (:2633) or the probe of the others (:2634-2646): one maybe_send_append per peer ----
        if (has_ins) {
#pragma unroll
            for (int s = 0; s < P; s++) {
                if (!((Wp >> s) & 1u) || s == (int)self) continue;
                const bool added = (ap.added >> s) & 1u;
                u32 pb = (u32)(row >> (8 * s)) & 0xffu;
                u32 start = added ? 0u : meta[s] & 0xffffu, count = added ? 0u : meta[s] >> 16;
                const u64 next = added ? hi + 1 : nx[s];
                const u64 prs = (pb & RG_PF_PEND_RS) ? rg_at(st.prs, (IX)s * (IX)st.stride + g) : 0ULL; // (never an added slot's)
                const RgConfPeer r = rg_conf_send_peer(pb, next, prs, count == ins.cap, hi, first_index, committed, max_entries, flags, ins.esz_w,
                                                       [&](u64 nxt, u64 avail) { return rg_limit_size(ins.esz + (u64)g * ins.esz_w, ins.esz_w - 1u, nxt, avail, max_entries); });
                if (r.add) {
                    rg_ins_add(ins, ((u64)g * (u64)P + (u64)s) * ins.cap, start, count, hd[s], tl[s], r.last);
                    meta[s] = start | (count << 16);
                    nx[s] = r.next;
                    dirty |= 1u << s;
                }
                pb = r.pb;
                if (!added) pb = (pb & ~RG_PF_INS_FULL) | (((pb & RG_PF_STATE_MASK) == RG_STATE_REPLICATE && count == ins.cap) ? RG_PF_INS_FULL : 0u);
                row = (row & ~(0xffULL << (8 * s))) | ((u64)pb << (8 * s));
                it.kind[s] = r.kind;
                it.prev[s] = r.prev;
                it.last[s] = r.last;
                it.n_items += r.kind ? 1u : 0u;
            }
        }
        events |= rg_conf_transfer(ap.cfg);
    }

    // ---- the stores ----
    rg_at(st.cfg, g) = ap.cfg;
    if (row != pf0) rg_at(st.pflags, g) = row;
    if (events & RGC_CONF_EV_COMMITTED) {
        if (st.pub) rg_pub_store(st, g, pub0 + (u32)rg_min(commit - commit0, 0x10000ULL), commit); // (in front of the commit column's store)
        rg_at(st.commit, g) = commit;
        if (prc_self < commit) rg_at(st.prc, (IX)self * (IX)st.stride + g) = commit;
        a.out = RG_OUT_CHANGED;
    }
#pragma unroll
    for (int s = 0; s < P; s++) {
        const IX o = (IX)s * (IX)st.stride + g;
        const bool added = (ap.added >> s) & 1u, moved = (dirty >> s) & 1u;
        if (added) { // Progress::new(hi + 1) (tracker.rs:385)
            rg_at(st.match, o) = 0ULL;
            rg_at(st.next, o) = hi + 1;
            rg_at(st.prc, o) = 0ULL;
            rg_at(st.psnap, o) = 0ULL;
            rg_at(st.prs, o) = 0ULL;
            rg_at(st.gid, o) = 0ULL;
            if (has_ins) rg_wst<0>(rg_at(ins.meta, o), 0u);
        }
        if (moved) { // update_state of a Replicate peer: next = last + 1, ins.add(last)
            rg_at(st.next, o) = nx[s];
            rg_wst<0>(rg_at(ins.meta, o), meta[s]);
            rg_wst<1>(rg_at(ins.head, o), hd[s]);
            rg_wst<1>(rg_at(ins.tail, o), tl[s]);
        }
    }
    a.commit = commit;
    a.cfg = ap.cfg;
    a.n_items = it.n_items;
    a.events = (uint8_t)events;
    a.added = (uint8_t)ap.added;
    a.removed = (uint8_t)ap.removed;
    return a;
}

template <int P> RG_D void rg_conf_lane_clear(RgConfLane<P> &it) {
#pragma unroll
    for (int s = 0; s < P; s++) {
        it.prev[s] = it.last[s] = 0;
        it.kind[s] = 0;
    }
    it.n_items = 0;
}

// The block's items into the caller's list. Every lane of the block calls it (barriers); n_items 0 = none of this lane's.
template <int P> RG_D void rg_conf_put_items(const RgConfItems &o, u64 g, const RgConfLane<P> &it) {
    __shared__ u32 wave_tot[4];
    __shared__ u32 block_base;
    const u32 n_items = it.n_items;
    if (!__syncthreads_or(n_items != 0)) return; // the common block: no group of it sends
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
        if (!it.kind[s]) continue;
        if (k < o.cap) {
            rg_send_item r;
            r.group = g;
            r.prev_index = it.prev[s];
            r.last_index = it.last[s];
            r.slot = (u32)s;
            r.n_msgs = 1;
            r.kind = (uint16_t)it.kind[s];
            o.items[k] = r;
        }
        k++;
    }
}

// The sparse form: lane = record (distinct groups, all in range, no malformed word: checked on the host).
template <int P, typename IX, bool GC>
__global__ __launch_bounds__(256) void k_conf_list(RgState st, RgIns ins, RgLeadCols lc, const rgc_conf_rec *recs, u64 n, rgc_conf_resp *resp, u64 max_entries, u32 flags,
                                                    RgConfItems o) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    RgConfLane<P> it;
    rg_conf_lane_clear<P>(it);
    u64 g = 0;
    if (i < n) {
        g = recs[i].group;
        const u32 W = recs[i].cfg;
        resp[i] = rg_conf_one<P, IX, GC>(st, ins, lc, (IX)g, W, max_entries, flags, it);
    }
    rg_conf_put_items<P>(o, g, it);
}

// The dense form: lane = group. An unselected group costs its selector byte and its status byte.
template <int P, typename IX, bool GC>
__global__ __launch_bounds__(256) void k_conf_dense(RgState st, RgIns ins, RgLeadCols lc, const u8 *sel, const u32 *cfgs, u8 *status, u8 *events, u64 *commit,
                                                     u64 max_entries, u32 flags, RgConfItems o) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    RgConfLane<P> it;
    rg_conf_lane_clear<P>(it);
    if (g < st.G) {
        if (!sel[g]) {
            status[g] = (u8)RGC_CONF_NONE;
        } else {
            const rgc_conf_resp a = rg_conf_one<P, IX, GC>(st, ins, lc, (IX)g, cfgs[g], max_entries, flags, it);
            status[g] = a.status;
            if (events) events[g] = a.events;
            if (commit) commit[g] = a.commit;
        }
    }
    rg_conf_put_items<P>(o, g, it);
}
