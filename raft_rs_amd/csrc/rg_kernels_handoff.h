// rg_kernels_handoff.h -- kernels of abi_handoff.hip, and what every way back from the leader engine into the follower arena shares
// (the step-down of rg_kernels_lead.h, the deposition of rg_kernels_term.h, the led half of rg_kernels_vote.h): the layers' columns
// as one kernel argument, one loader, one storer, one lead-side stop, one rg_handoff_back_one. One lane per record (the sparse
// forms) or per followed group (the dense forms), 256-thread blocks. A selected lane gathers scattered cold cells a stride apart
// -- latency, not bandwidth --, so it issues ALL its loads before its first store (the one-round-trip discipline
// RgTick::become_leader documents; the lead group's cells come one trip behind dev_lead[g], which names them). The leader columns
// are addressed with the engine's index width (IX: 32- or 64-bit cell offsets, as the tick's). No LDS, no atomics, plain stores.
// The kernels below are abi_handoff.hip's (one definition per library); everything else is a template or inline.
#pragma once
#include "rg_engine.h"
#include "rg_handoff.h"
#include "rg_term.h"

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
// ... and a log summary back into the arena's columns (every way back ends in it)
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

// ---- the way back with the soft cells and the lead side: step-down, deposition, the vote's led half ----
// The layers' columns; lc.cell / read_qterm (RgReadCols::qterm) are null while their layer is off.
struct RgArenaCols {
    RgState st;
    RgFollowCols fc;
    RgSoftCols sc;
    RgElectCols ec;
    RgLeadCols lc;
    u64 *read_qterm;
};

// The lead-side stop, idempotent: the clock cell STOPPED WITH the tag of the group's current term -- a promotion the clock has not
// seen yet (tag != RG_COL_CUR_TERM) must not re-arm the group on the next call. `all` (a deposition; the step-down's clock call did
// both already): the transferee gone, the group's pending reads dropped (the queue's term stamp) -- else neither the cfg word nor
// the stamp is touched. -> RGT_GATE_EV_TRANSFER_ABORTED or 0
struct RgLeadStop {
    u32 cell, cfg;
    u64 tag;
};
template <typename IX> RG_D RgLeadStop rg_handoff_load_stop(const RgState &st, const RgLeadCols &lc, IX L, bool all) {
    RgLeadStop c;
    c.cell = lc.cell ? lc.cell[L] : 0u;
    c.tag = lc.cell ? lc.tag[L] : 0ULL;
    c.cfg = all ? rg_at(st.cfg, L) : 0u;
    return c;
}
template <typename IX> RG_D u32 rg_handoff_store_stop(const RgState &st, const RgLeadCols &lc, u64 *read_qterm, IX L, const RgLeadStop &c, u64 cur_term, bool all) {
    if (lc.cell) {
        const u32 cell = rg_lead_stop(c.cell, c.tag, cur_term);
        if (cell != c.cell) lc.cell[L] = cell;
        if (c.tag != cur_term) lc.tag[L] = cur_term;
    }
    if (!all) return 0;
    u32 cfg = c.cfg;
    const u32 ev = rg_term_abort_transfer(cfg);
    if (cfg != c.cfg) rg_at(st.cfg, L) = cfg;
    if (read_qterm) read_qterm[L] = rg_lead_read_stamp(cur_term); // reset's ReadOnly::new (raft.rs:957)
    return ev;
}

// What a lane holds of (follow group g, lead group L) between its loads and its stores
struct RgBack {
    RgSoftView s, so; // the arena's soft view (role loaded) and its original
    RgHandoffWin w;
    RgHandoffLead l;
    RgLeadStop stop;
};
RG_D void rg_handoff_back_open(RgBack &b, const RgArenaCols &c, u64 g) {
    b.s = rg_soft_open(c.sc, g);
    b.so = b.s;
    b.w.term = b.s.term;
    b.w.lead = b.s.lead;
    b.w.role = rg_soft_role(b.s);
    b.w.self_id = c.ec.self_id[g];
    b.w.conf = 0;
}
// The loader of the lead side (L in range) ...
template <typename IX> RG_D void rg_handoff_back_load(RgBack &b, const RgArenaCols &c, IX L, bool all) {
    b.l = rg_handoff_load_lead<IX>(c.st, L);
    b.stop = rg_handoff_load_stop<IX>(c.st, c.lc, L, all);
}
// ... and the storer: the log `f` the arena takes, the soft view where `soft`, the lead-side stop (whose events it returns)
template <typename IX> RG_D u32 rg_handoff_back_store(const RgArenaCols &c, u64 g, IX L, const RgBack &b, const RgHandoffLog &f, bool soft, bool all) {
    rg_handoff_store_log(c.fc, g, f);
    if (soft) rg_soft_close(c.sc, g, b.s, b.so);
    return rg_handoff_store_stop<IX>(c.st, c.lc, c.read_qterm, L, b.stop, b.l.cur_term, all);
}

// Lead group L (in range) goes back into follow group g (in range); nothing is written unless the answer is DONE. `how` is a
// constant at every call site:
//                          refusals                       soft cells: become_follower(.., 0)     lead-side stop   answered term
//   RG_BACK_STEP_DOWN      rg_lead_step_down_check        at the unchanged term                  cell and tag     the group's
//   RG_BACK_DEPOSE         rg_term_depose_check at T      at T                                   all              T
//   RG_BACK_DEPOSE_SCAN    rg_lead_step_down_check        left to the gated step that follows    all              T
enum RgBackHow { RG_BACK_STEP_DOWN, RG_BACK_DEPOSE, RG_BACK_DEPOSE_SCAN };
template <typename IX> RG_D rg_handoff_resp rg_handoff_back_one(const RgArenaCols &c, u64 g, IX L, RgBackHow how, u64 T) {
    const bool depose = how != RG_BACK_STEP_DOWN, soft = how != RG_BACK_DEPOSE_SCAN;
    // ---- loads ----
    RgBack b;
    rg_handoff_back_open(b, c, g);
    rg_handoff_back_load<IX>(b, c, L, depose);
    // ---- arithmetic ----
    const u32 status = depose ? rg_term_depose_check(b.w, b.l.cur_term, T, soft) : rg_lead_step_down_check(b.w, b.l.cur_term);
    if (status != RG_HANDOFF_DONE) return rg_handoff_answer(status, 0, 0, 0, 0);
    rg_follow_state fs;
    fs.group = g;
    if (rg_handoff_demote(b.l, fs) != RG_HANDOFF_DONE) return rg_handoff_answer(RG_HANDOFF_FAULT, 0, 0, 0, 0);
    const RgHandoffLog f = rg_handoff_export(fs);
    if (how == RG_BACK_DEPOSE) rg_term_depose_soft(c.sc.cfg, g, b.s, T);
    if (how == RG_BACK_STEP_DOWN) rg_lead_step_down_soft(c.sc.cfg, g, b.s);
    // ---- stores ----
    rg_handoff_back_store<IX>(c, g, L, b, f, soft, depose);
    return rg_handoff_answer(RG_HANDOFF_DONE, depose ? T : b.l.cur_term, b.l.hi, b.l.commit, 0);
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
