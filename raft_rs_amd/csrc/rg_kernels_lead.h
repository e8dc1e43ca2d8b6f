// rg_kernels_lead.h -- kernels of ext_lead.hip: the leader's clock (one lane per group of the leader engine, 256-thread blocks) and
// the way back into the follower arena (one lane per record or per followed group; rg_handoff_back_one of rg_kernels_handoff.h). A
// lane issues the loads of a phase before its first store; the cfg word and the flag row are loaded only at an election timeout, the
// matched cells and the commit index only on a beat with hb_commit. A lane that steps down stores one word more: the term stamp of
// its group's ReadIndex queue (read_qterm = RgReadCols::qterm, null without that layer), so that the queue's own lazy reset empties
// it. The per-slot columns are addressed with the engine's index width (IX, as in rg_kernels_handoff.h). The lists are compacted as
// k_follow_clock does it (rg_wave.h): a ballot per wave, ONE atomic per wave and list. No LDS, plain stores. Included by exactly one
// unit.
#pragma once
#include "rg_engine.h"
#include "rg_kernels_handoff.h"
#include "rg_lead.h"
#include "rg_wave.h"

__global__ __launch_bounds__(256) void k_lead_init(RgLeadCols lc, const u64 *__restrict__ cur_term, u64 G, u64 stride, u32 led) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    if (g >= stride) return;
    lc.tag[g] = g < G ? cur_term[g] : 0;
    lc.cell[g] = g < G && led ? 0u : RG_LEAD_CELL_STOPPED;
}

template <typename IX>
__global__ __launch_bounds__(256) void k_lead_clock(RgState st, RgLeadCols lc, u32 P, rg_lead_clock_out out, unsigned long long *counts, u64 *read_qterm) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    u32 ev = 0;
    if (g < st.G) {
        // ---- phase 1: the three hot cells ----
        const u32 cell0 = lc.cell[g];
        const u64 tag0 = lc.tag[g], term = st.cur_term[g];
        RgLeadAdvance a = rg_lead_advance(lc.cfg, cell0, tag0, term);
        // ---- phase 2: what a timeout needs ----
        const bool quorum = a.at_election && (lc.cfg.flags & RG_GATE_CHECK_QUORUM), commits = a.at_heartbeat && out.hb_commit;
        u32 cfg0 = 0;
        u64 pf0 = 0, commit = 0, m[8];
        if (a.at_election || commits) cfg0 = st.cfg[g];
        if (quorum) pf0 = st.pflags[g];
        if (commits) {
            commit = st.commit[g];
#pragma unroll
            for (u32 p = 0; p < 8; p++) m[p] = p < P ? rg_at(st.match, (IX)p * (IX)st.stride + (IX)g) : 0;
        }
        u32 cfg = cfg0;
        u64 pf = pf0;
        if (a.at_election) rg_lead_timeout(lc.cfg, a, cfg, pf);
        rg_lead_beat(a);
        ev = a.events;
        // ---- stores ----
        if (a.tag != tag0) lc.tag[g] = a.tag;
        if (a.cell != cell0) lc.cell[g] = a.cell;
        if (cfg != cfg0) st.cfg[g] = cfg;
        if (pf != pf0) st.pflags[g] = pf;
        if (read_qterm && (ev & RG_LEAD_EV_STEPPED_DOWN)) read_qterm[g] = rg_lead_read_stamp(term); // reset's ReadOnly::new (raft.rs:957)
        if (commits && (ev & RG_LEAD_EV_BEAT)) {
#pragma unroll
            for (u32 p = 0; p < 8; p++)
                if (p < P) rg_at(out.hb_commit, (IX)p * (IX)st.stride + (IX)g) = rg_lead_hb_commit(cfg, p, m[p], commit);
        }
        out.events[g] = (u8)ev;
    }
    rg_wave_append((ev & RG_LEAD_EV_BEAT) != 0, g, out.beat, out.beat_cap, &counts[0]);
    rg_wave_append((ev & RG_LEAD_EV_STEPPED_DOWN) != 0, g, out.down, out.down_cap, &counts[2]);
    rg_wave_append((ev & RG_LEAD_EV_CHECK_QUORUM) != 0, g, nullptr, 0, &counts[1]);
    rg_wave_append((ev & RG_LEAD_EV_TRANSFER_ABORTED) != 0, g, nullptr, 0, &counts[3]);
}

__global__ __launch_bounds__(256) void k_lead_clock_write(RgLeadCols lc, const rg_lead_clock_cell *__restrict__ recs, u64 n) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const rg_lead_clock_cell w = recs[i];
    lc.tag[w.group] = w.term;
    lc.cell[w.group] = rg_lead_cell_of(w);
}
__global__ __launch_bounds__(256) void k_lead_clock_read(RgLeadCols lc, const u64 *__restrict__ groups, u64 n, rg_lead_clock_cell *out) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 g = groups[i];
    out[i] = rg_lead_record(g, lc.tag[g], lc.cell[g]);
}
// rg_permute_groups: new position i takes the cells of old position perm[i]
__global__ __launch_bounds__(256) void k_lead_place(RgLeadCols src, u64 *tag, u32 *cell, const u64 *__restrict__ perm, u64 G) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= G) return;
    const u64 o = perm[i];
    tag[i] = src.tag[o];
    cell[i] = src.cell[o];
}

// The way back into the arena of a group that stepped down, at its unchanged term
template <typename IX>
__global__ __launch_bounds__(256) void k_handoff_step_down_list(RgArenaCols c, const rg_handoff_rec *__restrict__ recs, u64 n, rg_handoff_resp *resp) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    resp[i] = rg_handoff_back_one<IX>(c, recs[i].follow_group, (IX)recs[i].lead_group, RG_BACK_STEP_DOWN, 0);
}
// Lane = followed group. A group without a lead group costs its dev_lead cell and its status byte, an unselected one an event byte more.
template <typename IX>
__global__ __launch_bounds__(256) void k_handoff_step_down_dense(RgArenaCols c, const u8 *__restrict__ events, const u64 *__restrict__ lead, rg_handoff_out out) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    if (g >= c.fc.n) return;
    const u64 L = lead[g];
    if (L >= c.st.G) { // no lead group -- or not a group of the engine: nothing is read or written through it
        out.status[g] = L == RG_HANDOFF_NO_LEAD ? RG_HANDOFF_NONE : RG_HANDOFF_FAULT;
        return;
    }
    if (!(events[L] & RG_LEAD_EV_STEPPED_DOWN)) {
        out.status[g] = RG_HANDOFF_NONE;
        return;
    }
    rg_handoff_put(out, g, rg_handoff_back_one<IX>(c, g, (IX)L, RG_BACK_STEP_DOWN, 0));
}
