// rg_kernels_handoff.h -- kernels of abi_handoff.hip: the hand-off between the follower arena and the leader columns, one lane per
// record (the sparse forms) or per followed group (the dense forms), 256-thread blocks. A selected lane gathers scattered cold
// cells a stride apart -- latency, not bandwidth --, so it issues ALL its loads before its first store (the one-round-trip
// discipline RgTick::become_leader documents; the lead group's cells come one trip behind dev_lead[g], which names them). The
// leader columns are addressed with the engine's index width (IX: 32- or 64-bit cell offsets, as the tick's). No LDS, no
// atomics, plain stores. Included by exactly one abi_*.hip unit (one definition per library).
#pragma once
#include "rg_engine.h"
#include "rg_handoff.h"

RG_D RgHandoffLog rg_handoff_load_log(const RgFollowCols &c, u64 g) {
    RgHandoffLog f;
    f.committed = c.committed[g];
    f.last = c.last[g];
    f.tail_first = c.tail_first[g];
    f.tail_term = c.tail_term[g];
    f.dummy_idx = c.dummy_idx[g];
    f.dummy_term = c.dummy_term[g];
    f.n_old = c.n_old[g];
#pragma unroll
    for (u32 k = 0; k < RG_TERM_RUNS; k++) {
        f.run_first[k] = c.run_first[(u64)k * c.stride + g];
        f.run_term[k] = c.run_term[(u64)k * c.stride + g];
    }
    return f;
}
// ... and a log summary back into the arena's columns (the demotion, the step-down and the deposition end in it)
RG_D void rg_handoff_store_log(const RgFollowCols &fc, u64 g, const RgHandoffLog &f) {
    fc.committed[g] = f.committed;
    fc.last[g] = f.last;
    fc.tail_first[g] = f.tail_first;
    fc.tail_term[g] = f.tail_term;
    fc.dummy_idx[g] = f.dummy_idx;
    fc.dummy_term[g] = f.dummy_term;
    fc.n_old[g] = (u8)f.n_old;
#pragma unroll
    for (u32 k = 0; k < RG_TERM_RUNS; k++) {
        fc.run_first[(u64)k * fc.stride + g] = f.run_first[k];
        fc.run_term[(u64)k * fc.stride + g] = f.run_term[k];
    }
}
template <typename IX> RG_D RgHandoffLead rg_handoff_load_lead(const RgState &st, IX L) {
    RgHandoffLead l;
    l.commit = rg_at(st.commit, L);
    l.lo = rg_at(st.lo, L);
    l.hi = rg_at(st.hi, L);
    l.cur_term = rg_at(st.cur_term, L);
    l.dummy_idx = rg_at(st.dummy_idx, L);
    l.dummy_term = rg_at(st.dummy_term, L);
    l.n_runs = rg_at(rg_run_n(st), L);
#pragma unroll
    for (u32 k = 0; k < RG_TERM_RUNS; k++) {
        l.run_first[k] = rg_at(st.run_first, (IX)k * (IX)st.stride + L);
        l.run_term[k] = rg_at(st.run_term, (IX)k * (IX)st.stride + L);
    }
    return l;
}

// Promotion of follow group g into lead group L (both in range). Returns the answer; writes nothing unless it is DONE.
template <typename IX> RG_D rg_handoff_resp rg_handoff_promote_one(const RgState &st, const RgFollowCols &fc, const RgSoftCols &sc, const RgElectCols &ec, u32 P,
                                                                   u64 g, IX L, const u64 *persisted_cell) {
    // ---- loads ----
    const RgHandoffLog f = rg_handoff_load_log(fc, g);
    RgHandoffWin w;
    w.term = sc.term[g];
    w.lead = sc.lead[g];
    w.role = sc.role[g];
    w.self_id = ec.self_id[g];
    w.conf = ec.conf[g];
    const u64 persisted = persisted_cell ? *persisted_cell : f.last;
    const u32 cfg = rg_at(st.cfg, L);
    const u64 pf = rg_at(st.pflags, L);
    // ---- arithmetic ----
    const u32 status = rg_handoff_promote_check(f, w, cfg, P, persisted);
    if (status != RG_HANDOFF_DONE) return rg_handoff_answer(status, 0, 0, 0, 0);
    RgHandoffLead l = rg_handoff_import(f);
    const u64 old_hi = l.hi;
    rg_handoff_become_leader(l, w.term);
    const RgHandoffProgress pr = rg_handoff_progress(pf, cfg, P, old_hi);
    // ---- stores ----
    rg_at(st.commit, L) = l.commit;
    rg_at(st.lo, L) = l.lo;
    rg_at(st.hi, L) = l.hi;
    rg_at(st.cur_term, L) = l.cur_term;
    rg_at(st.dummy_idx, L) = l.dummy_idx;
    rg_at(st.dummy_term, L) = l.dummy_term;
    rg_at(rg_run_n(st), L) = (u8)l.n_runs;
#pragma unroll
    for (u32 k = 0; k < RG_TERM_RUNS; k++) {
        rg_at(st.run_first, (IX)k * (IX)st.stride + L) = l.run_first[k];
        rg_at(st.run_term, (IX)k * (IX)st.stride + L) = l.run_term[k];
    }
#pragma unroll
    for (u32 i = 0; i < 8; i++) {
        if (!((pr.present >> i) & 1u)) continue;
        const IX o = (IX)i * (IX)st.stride + L;
        const bool own = i == pr.self;
        rg_at(st.match, o) = own ? persisted : 0ULL;
        rg_at(st.next, o) = own ? persisted + 1 : pr.next_all;
        if (own) rg_at(st.prc, o) = l.commit;
        if ((pr.clear_snap >> i) & 1u) rg_at(st.psnap, o) = 0;
        if ((pr.clear_rs >> i) & 1u) rg_at(st.prs, o) = 0;
    }
    if (pr.pf != pf) rg_at(st.pflags, L) = pr.pf;
    if (pr.cfg != cfg) rg_at(st.cfg, L) = pr.cfg;
    return rg_handoff_answer(RG_HANDOFF_DONE, w.term, l.hi, l.commit, RG_OUT_BECAME_LEADER | RG_OUT_APPENDED);
}

// Demotion of lead group L into follow group g (both in range): nothing of the leader side is written.
template <typename IX> RG_D rg_handoff_resp rg_handoff_demote_one(const RgState &st, const RgFollowCols &fc, u64 g, IX L) {
    const RgHandoffLead l = rg_handoff_load_lead<IX>(st, L);
    rg_follow_state s;
    s.group = g;
    if (rg_handoff_demote(l, s) != RG_HANDOFF_DONE) return rg_handoff_answer(RG_HANDOFF_FAULT, 0, 0, 0, 0);
    const RgHandoffLog f = rg_handoff_export(s);
    rg_handoff_store_log(fc, g, f);
    return rg_handoff_answer(RG_HANDOFF_DONE, l.cur_term, l.hi, l.commit, 0);
}

// The sparse forms: lane = record (distinct follow groups, distinct lead groups, all in range: checked on the host).
template <typename IX>
__global__ __launch_bounds__(256) void k_handoff_promote_list(RgState st, RgFollowCols fc, RgSoftCols sc, RgElectCols ec, u32 P, const rg_handoff_rec *__restrict__ recs,
                                                               u64 n, rg_handoff_resp *resp) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    resp[i] = rg_handoff_promote_one<IX>(st, fc, sc, ec, P, recs[i].follow_group, (IX)recs[i].lead_group, &recs[i].persisted);
}
template <typename IX>
__global__ __launch_bounds__(256) void k_handoff_demote_list(RgState st, RgFollowCols fc, const rg_handoff_rec *__restrict__ recs, u64 n, rg_handoff_resp *resp) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    resp[i] = rg_handoff_demote_one<IX>(st, fc, recs[i].follow_group, (IX)recs[i].lead_group);
}

// The dense forms: lane = followed group. An unselected group costs its selector byte and its status byte.
RG_D void rg_handoff_put(const rg_handoff_out &out, u64 g, const rg_handoff_resp &a) {
    out.status[g] = (u8)a.status;
    if (a.status == RG_HANDOFF_DONE) {
        out.term[g] = a.term;
        out.last_index[g] = a.last_index;
    }
}
template <typename IX>
__global__ __launch_bounds__(256) void k_handoff_promote_dense(RgState st, RgFollowCols fc, RgSoftCols sc, RgElectCols ec, u32 P, const u8 *__restrict__ result,
                                                                const u64 *__restrict__ lead, const u64 *__restrict__ persisted, rg_handoff_out out) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    if (g >= fc.n) return;
    if (result[g] != RG_ELECT_WON) {
        out.status[g] = RG_HANDOFF_NONE;
        return;
    }
    const u64 L = lead[g];
    if (L >= st.G) { // not a group of the engine: nothing is read or written through it
        out.status[g] = RG_HANDOFF_FAULT;
        return;
    }
    rg_handoff_put(out, g, rg_handoff_promote_one<IX>(st, fc, sc, ec, P, g, (IX)L, persisted ? persisted + g : nullptr));
}
template <typename IX>
__global__ __launch_bounds__(256) void k_handoff_demote_dense(RgState st, RgFollowCols fc, const u8 *__restrict__ select, const u64 *__restrict__ lead,
                                                               rg_handoff_out out) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    if (g >= fc.n) return;
    if (!select[g]) {
        out.status[g] = RG_HANDOFF_NONE;
        return;
    }
    const u64 L = lead[g];
    if (L >= st.G) {
        out.status[g] = RG_HANDOFF_FAULT;
        return;
    }
    rg_handoff_put(out, g, rg_handoff_demote_one<IX>(st, fc, g, (IX)L));
}
