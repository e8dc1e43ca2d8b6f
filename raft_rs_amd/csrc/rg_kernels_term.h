// rg_kernels_term.h -- kernels of ext_term.hip: the leader's term gate (one lane per group of the leader engine, 256-thread blocks)
// and the deposition into the follower arena (one lane per record or per followed group; rg_handoff_back_one of
// rg_kernels_handoff.h). The gate's lane loads its flag row as one word, the three hot cells (RG_COL_CUR_TERM, the clock's tag and
// cell) and the term of every record of a led group -- nothing else unless the group is deposed; it keeps no scratch and no LDS.
// The deposed groups are listed and the two record counts summed per wave (rg_wave.h: ONE atomic per wave). The per-slot columns are
// addressed with the engine's index width (IX, as in rg_kernels_handoff.h). Included by exactly one unit.
#pragma once
#include "rg_engine.h"
#include "rg_kernels_handoff.h"
#include "rg_term.h"
#include "rg_wave.h"

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
            RgLeadStop c;
            c.cell = cell;
            c.tag = tag;
            c.cfg = st.cfg[g];
            ev |= rg_handoff_store_stop<IX>(st, lc, read_qterm, (IX)g, c, cur, true);
            out.new_term[g] = r.new_term;
        }
        out_flags[g] = r.row;
        out.events[g] = (u8)ev;
    }
    rg_wave_append((ev & RGT_GATE_EV_DEPOSED) != 0, g, out.down, out.down_cap, &counts[0]);
    rg_wave_add(n_stale, &counts[1]);
    rg_wave_add(n_not_led, &counts[2]);
}

// The way back at the new term of a group the gate deposed
template <typename IX>
__global__ __launch_bounds__(256) void k_term_depose_list(RgArenaCols c, const rgt_depose_rec *__restrict__ recs, u64 n, rg_handoff_resp *resp) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    resp[i] = rg_handoff_back_one<IX>(c, recs[i].follow_group, (IX)recs[i].lead_group, RG_BACK_DEPOSE, recs[i].term);
}
// Lane = followed group. A group without a lead group costs its dev_lead cell and its status byte, an unselected one an event byte more.
template <typename IX>
__global__ __launch_bounds__(256) void k_term_depose_dense(RgArenaCols c, const u8 *__restrict__ events, const u64 *__restrict__ new_term, const u64 *__restrict__ lead,
                                                            rg_handoff_out out) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    if (g >= c.fc.n) return;
    const u64 L = lead[g];
    if (L >= c.st.G) { // no lead group -- or not a group of the engine: nothing is read or written through it
        out.status[g] = L == RG_HANDOFF_NO_LEAD ? RG_HANDOFF_NONE : RG_HANDOFF_FAULT;
        return;
    }
    if (!(events[L] & RGT_GATE_EV_DEPOSED)) {
        out.status[g] = RG_HANDOFF_NONE;
        return;
    }
    rg_handoff_put(out, g, rg_handoff_back_one<IX>(c, g, (IX)L, RG_BACK_DEPOSE, new_term[L]));
}
// Lane = followed group; the selectors are the gated step's own columns. A group without a message costs its flag byte and its
// status byte; one with a message its dev_lead cell more, and where that names a lead group the four cells of the selection. The
// soft cells are left to the gated step that follows.
template <typename IX>
__global__ __launch_bounds__(256) void k_term_depose_scan(RgArenaCols c, const u8 *__restrict__ msg_flags, const u64 *__restrict__ m_term, const u64 *__restrict__ lead,
                                                           rg_handoff_out out) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    if (g >= c.fc.n) return;
    const u32 kind = msg_flags[g];
    if (!kind) {
        out.status[g] = RG_HANDOFF_NONE;
        return;
    }
    const u64 L = lead[g];
    if (L >= c.st.G) {
        out.status[g] = L == RG_HANDOFF_NO_LEAD ? RG_HANDOFF_NONE : RG_HANDOFF_FAULT;
        return;
    }
    RgHandoffWin w;
    w.term = c.sc.term[g];
    w.lead = c.sc.lead[g];
    w.role = c.sc.role[g];
    w.self_id = c.ec.self_id[g];
    w.conf = 0;
    const u64 T = m_term[g];
    if (!rg_term_scan_selects(kind, w, rg_at(c.st.cur_term, (IX)L), T)) {
        out.status[g] = RG_HANDOFF_NONE;
        return;
    }
    rg_handoff_put(out, g, rg_handoff_back_one<IX>(c, g, (IX)L, RG_BACK_DEPOSE_SCAN, T));
}
