// rg_kernels_term.h -- kernels of ext_term.hip: the leader's term gate (one lane per group of the leader engine, 256-thread blocks)
// and the deposition into the follower arena (one lane per record or per followed group). The gate's lane loads its flag row as one
// word, the three hot cells (RG_COL_CUR_TERM, the clock's tag and cell) and the term of every record of a led group -- nothing else
// unless the group is deposed; it keeps no scratch and no LDS. The deposed groups are listed through rg_lead_append (a ballot per
// wave, ONE atomic per wave), the two record counts are summed per wave before their atomic. The per-slot columns are addressed
// with the engine's index width (IX, as in rg_kernels_lead.h). Included by exactly one unit.
#pragma once
#include "rg_engine.h"
#define RG_LEAD_KERNELS_SHARED_ONLY // rg_lead_append and the hand-off's loaders; the clock's own kernels are ext_lead.hip's
#include "rg_kernels_lead.h"
#include "rg_term.h"

// The wave's sum of `n` (small: at most 8 per lane) added to *count with one atomic; nothing is issued for a wave of zeros.
RG_D void rg_term_wave_add(u32 n, unsigned long long *count) {
    if (!__ballot(n != 0)) return;
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) n += __shfl_xor(n, w);
    if ((threadIdx.x & 63u) == 0) atomicAdd(count, (unsigned long long)n);
}

// The lead-side stop of a deposition, idempotent: the clock cell STOPPED with the tag of the current term, the transferee gone, the
// group's pending reads dropped (the queue's term stamp). `lc.cell` / `read_qterm` are null while their layer is off.
// -> RGT_GATE_EV_TRANSFER_ABORTED or 0
struct RgTermLeadCells {
    u32 cell, cfg;
    u64 tag;
};
template <typename IX> RG_D RgTermLeadCells rg_term_load_stop(const RgState &st, const RgLeadCols &lc, IX L) {
    RgTermLeadCells c;
    c.cell = lc.cell ? lc.cell[L] : 0u;
    c.tag = lc.cell ? lc.tag[L] : 0ULL;
    c.cfg = rg_at(st.cfg, L);
    return c;
}
template <typename IX> RG_D u32 rg_term_store_stop(const RgState &st, const RgLeadCols &lc, u64 *read_qterm, IX L, const RgTermLeadCells &c, u64 cur_term) {
    if (lc.cell) {
        const u32 cell = rg_lead_stop(c.cell, c.tag, cur_term);
        if (cell != c.cell) lc.cell[L] = cell;
        if (c.tag != cur_term) lc.tag[L] = cur_term;
    }
    u32 cfg = c.cfg;
    const u32 ev = rg_term_abort_transfer(cfg);
    if (cfg != c.cfg) rg_at(st.cfg, L) = cfg;
    if (read_qterm) read_qterm[L] = rg_lead_read_stamp(cur_term); // reset's ReadOnly::new (raft.rs:957)
    return ev;
}

template <typename IX>
__global__ __launch_bounds__(256) void k_term_gate(RgState st, RgLeadCols lc, u32 P, const u64 *m_flags /* may alias out_flags */, const u64 *__restrict__ m_term, u64 *out_flags,
                                                    rgt_lead_gate_out out, unsigned long long *counts, u64 *read_qterm) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    u32 ev = 0, n_stale = 0, n_not_led = 0;
    if (g < st.G) {
        // ---- the row and the three hot cells ----
        const u64 row = m_flags[g], cur = st.cur_term[g], tag = lc.tag[g];
        const u32 cell = lc.cell[g];
        const bool led = rg_term_led(cell, tag, cur);
        // ---- the terms of a led group's records ----
        u64 t[8];
#pragma unroll
        for (u32 p = 0; p < 8; p++) t[p] = (p < P && led && rg_term_is_record(row, p)) ? rg_at(m_term, (IX)p * (IX)st.stride + (IX)g) : 0ULL;
        const RgTermGate r = rg_term_gate_row(row, P, led, cur, t);
        ev = r.events;
        n_stale = r.n_stale;
        n_not_led = r.n_not_led;
        // ---- a deposition: become_follower(new_term, INVALID_ID) as far as the leader engine has the state ----
        if (ev & RGT_GATE_EV_DEPOSED) {
            RgTermLeadCells c;
            c.cell = cell;
            c.tag = tag;
            c.cfg = st.cfg[g];
            ev |= rg_term_store_stop<IX>(st, lc, read_qterm, (IX)g, c, cur);
            out.new_term[g] = r.new_term;
        }
        out_flags[g] = r.row;
        out.events[g] = (u8)ev;
    }
    rg_lead_append((ev & RGT_GATE_EV_DEPOSED) != 0, g, out.down, out.down_cap, &counts[0]);
    rg_term_wave_add(n_stale, &counts[1]);
    rg_term_wave_add(n_not_led, &counts[2]);
}

// The way back at the new term: lead group L (in range) is deposed into follow group g (in range) at term T. Nothing is written
// unless the answer is DONE. soft = false (the scan form): the soft cells are left to the gated step that follows.
template <typename IX>
RG_D rg_handoff_resp rg_term_depose_one(const RgState &st, const RgFollowCols &fc, const RgSoftCols &sc, const RgElectCols &ec, const RgLeadCols &lc, u64 *read_qterm,
                                        u64 g, IX L, u64 T, bool soft) {
    // ---- loads ----
    RgSoftView s = rg_soft_open(sc, g);
    const RgSoftView so = s;
    RgHandoffWin w;
    w.term = s.term;
    w.lead = s.lead;
    w.role = rg_soft_role(s);
    w.self_id = ec.self_id[g];
    w.conf = 0;
    const RgHandoffLead l = rg_handoff_load_lead<IX>(st, L);
    const RgTermLeadCells c = rg_term_load_stop<IX>(st, lc, L);
    // ---- arithmetic ----
    const u32 status = rg_term_depose_check(w, l.cur_term, T, soft);
    if (status != RG_HANDOFF_DONE) return rg_handoff_answer(status, 0, 0, 0, 0);
    rg_follow_state fs;
    fs.group = g;
    if (rg_handoff_demote(l, fs) != RG_HANDOFF_DONE) return rg_handoff_answer(RG_HANDOFF_FAULT, 0, 0, 0, 0);
    const RgHandoffLog f = rg_handoff_export(fs);
    if (soft) rg_term_depose_soft(sc.cfg, g, s, T);
    // ---- stores ----
    rg_handoff_store_log(fc, g, f);
    if (soft) rg_soft_close(sc, g, s, so);
    rg_term_store_stop<IX>(st, lc, read_qterm, L, c, l.cur_term);
    return rg_handoff_answer(RG_HANDOFF_DONE, T, l.hi, l.commit, 0);
}

template <typename IX>
__global__ __launch_bounds__(256) void k_term_depose_list(RgState st, RgFollowCols fc, RgSoftCols sc, RgElectCols ec, RgLeadCols lc, u64 *read_qterm,
                                                           const rgt_depose_rec *__restrict__ recs, u64 n, rg_handoff_resp *resp) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    resp[i] = rg_term_depose_one<IX>(st, fc, sc, ec, lc, read_qterm, recs[i].follow_group, (IX)recs[i].lead_group, recs[i].term, true);
}
// Lane = followed group. A group without a lead group costs its dev_lead cell and its status byte, an unselected one an event byte more.
template <typename IX>
__global__ __launch_bounds__(256) void k_term_depose_dense(RgState st, RgFollowCols fc, RgSoftCols sc, RgElectCols ec, RgLeadCols lc, u64 *read_qterm,
                                                            const u8 *__restrict__ events, const u64 *__restrict__ new_term, const u64 *__restrict__ lead,
                                                            rg_handoff_out out) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    if (g >= fc.n) return;
    const u64 L = lead[g];
    if (L >= st.G) { // no lead group -- or not a group of the engine: nothing is read or written through it
        out.status[g] = L == RG_HANDOFF_NO_LEAD ? RG_HANDOFF_NONE : RG_HANDOFF_FAULT;
        return;
    }
    if (!(events[L] & RGT_GATE_EV_DEPOSED)) {
        out.status[g] = RG_HANDOFF_NONE;
        return;
    }
    rg_handoff_put(out, g, rg_term_depose_one<IX>(st, fc, sc, ec, lc, read_qterm, g, (IX)L, new_term[L], true));
}
// Lane = followed group; the selectors are the gated step's own columns. A group without a message costs its flag byte and its
// status byte; one with a message its dev_lead cell more, and where that names a lead group the four cells of the selection.
template <typename IX>
__global__ __launch_bounds__(256) void k_term_depose_scan(RgState st, RgFollowCols fc, RgSoftCols sc, RgElectCols ec, RgLeadCols lc, u64 *read_qterm,
                                                           const u8 *__restrict__ msg_flags, const u64 *__restrict__ m_term, const u64 *__restrict__ lead,
                                                           rg_handoff_out out) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    if (g >= fc.n) return;
    const u32 kind = msg_flags[g];
    if (!kind) {
        out.status[g] = RG_HANDOFF_NONE;
        return;
    }
    const u64 L = lead[g];
    if (L >= st.G) {
        out.status[g] = L == RG_HANDOFF_NO_LEAD ? RG_HANDOFF_NONE : RG_HANDOFF_FAULT;
        return;
    }
    RgHandoffWin w;
    w.term = sc.term[g];
    w.lead = sc.lead[g];
    w.role = sc.role[g];
    w.self_id = ec.self_id[g];
    w.conf = 0;
    const u64 T = m_term[g];
    if (!rg_term_scan_selects(kind, w, rg_at(st.cur_term, (IX)L), T)) {
        out.status[g] = RG_HANDOFF_NONE;
        return;
    }
    rg_handoff_put(out, g, rg_term_depose_one<IX>(st, fc, sc, ec, lc, read_qterm, g, (IX)L, T, false));
}
