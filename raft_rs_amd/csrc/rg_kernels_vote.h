// rg_kernels_vote.h -- kernels of ext_vote.hip: the dense vote step (one lane per followed group, 256-thread blocks) and its sparse
// form (one lane per record). A block without a request leaves after its flag bytes and writes its three answer bytes per group --
// decided per WAVE with a ballot, not with k_follow_gate_dense's __syncthreads_or, which costs 256 B of LDS and a barrier: every
// collective below is a wave's, so a wave is the unit that may leave. A request of a group that is not led runs rg_gate_step on the
// arena's views: the soft hot cells and the log's hot cells, the cold ones (vote, role, priority, the older runs) only where the
// arithmetic asks. Only a led group touches the leader columns -- its log summary, one trip behind dev_lead[g] which names them,
// all loads before the first store -- and only a deposed one stores: through the loader and the storer of rg_kernels_handoff.h.
// The answered list is appended per wave (rg_wave.h: ONE atomic per wave and tile), the five counts are ballots summed in registers
// over the tiles a wave walks: one atomic per wave and count that is not zero. No scratch, no LDS. The leader columns are addressed
// with the engine's index width (IX, as in rg_kernels_handoff.h). Included by exactly one unit.
#pragma once
#include "rg_engine.h"
#include "rg_kernels_handoff.h"
#include "rg_vote.h"
#include "rg_wave.h"

// One well-formed request of follow group g (in range); L = its dev_lead value (RG_HANDOFF_NO_LEAD: none). Nothing is written
// where the status is FAULT or HOST.
template <typename IX> RG_D rgv_vote_resp rg_vote_one(const RgArenaCols &c, u64 g, u64 L, const RgVoteReq &m) {
    RgBack b;
    b.s = rg_soft_open(c.sc, g);
    b.so = b.s;
    bool led = false;
    if (L != RG_HANDOFF_NO_LEAD) {
        if (L >= c.st.G) return rg_vote_fault(); // not a group of the engine: nothing is read or written through it
        led = rg_vote_win_state(b.s.lead, c.ec.self_id[g], rg_soft_role(b.s));
    }
    if (!led) { // exactly the gated step (rg_follow.h)
        RgFollowView v = rg_follow_open(c.fc, g);
        const RgFollowView o = v;
        RgFollowRec r;
        r.index = m.index;
        r.log_term = m.log_term;
        r.commit = m.commit;
        r.ent_term = m.commit_term;
        r.n_entries = 0;
        r.flags = m.kind;
        r.ext = nullptr;
        r.n_ext = 0;
        rg_follow_resp fr;
        const rg_follow_gate_resp a = rg_gate_step(c.sc.cfg, g, b.s, v, r, m.term, m.from, m.priority, m.hdr_flags, fr);
        rg_follow_close(c.fc, g, v, o);
        rg_soft_close(c.sc, g, b.s, b.so);
        return rg_vote_answer(fr.status, a.gate, a.events, a.term, fr.commit, fr.log_term, v.last);
    }
    // ---- led: the loads ----
    rg_handoff_back_load<IX>(b, c, (IX)L, true);
    // ---- arithmetic ----
    RgHandoffLog f;
    bool depose;
    rgv_vote_resp a = rg_vote_led_group(c.sc.cfg, g, b.s, b.l, c.lc.cell != nullptr, b.stop.cell, b.stop.tag, m, f, depose);
    if (!depose) return a;
    // ---- a deposition: the arena takes the group back at m.term, the lead side is stopped ----
    if (rg_handoff_back_store<IX>(c, g, (IX)L, b, f, true, true)) a.events |= RGV_VOTE_EV_TRANSFER_ABORTED;
    return a;
}

// counts: u64 [6] = requests, grants, rejects, ignored, deposed, and the cursor of the answered list. A block walks the tiles of 256
// groups blockIdx.x, blockIdx.x + gridDim.x, ...: a wave sums its five counts in registers over its tiles and issues ONE atomic per
// count that is not zero when it is done -- same-line atomics are what bounds this kernel, so their number follows the grid, not
// the arena. The cursor's atomic stays one per wave and tile with an answered lane, and is not issued without a list.
template <typename IX>
__global__ __launch_bounds__(256) void k_vote_dense(RgArenaCols c, rg_follow_msgs ms, const u64 *__restrict__ m_term, const u64 *__restrict__ m_from,
                                                     const int64_t *__restrict__ m_priority, const u8 *__restrict__ m_hdr, const u64 *__restrict__ lead, rgv_vote_out out,
                                                     unsigned long long *counts) {
    const u64 n_tiles = (c.fc.n + 255) / 256;
    u32 n_req = 0, n_grant = 0, n_reject = 0, n_ignored = 0, n_deposed = 0;
    for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) { // (block-uniform: every lane of a wave makes the same trips)
        const u64 g = tile * 256 + threadIdx.x;
        const bool in = g < c.fc.n;
        const u32 flags = in ? ms.flags[g] : 0u;
        const bool req = in && rg_vote_is_request(flags);
        if (!__ballot(req)) { // the whole WAVE skips the tile (a block without a request: all four): no wave operation below is skipped by part of one
            if (in) {
                out.status[g] = RG_FOLLOW_NONE;
                out.gate[g] = RG_GATE_NONE;
                out.events[g] = 0;
            }
            continue;
        }
        rgv_vote_resp a = rg_vote_answer(RG_FOLLOW_NONE, RG_GATE_NONE, 0, 0, 0, 0, 0);
        if (req) {
            RgVoteReq m;
            m.term = m_term[g];
            m.from = m_from[g];
            m.index = ms.index[g];
            m.log_term = ms.log_term[g];
            m.commit = ms.commit[g];
            m.commit_term = ms.ent_term[g];
            m.priority = m_priority ? m_priority[g] : 0;
            m.kind = flags;
            m.hdr_flags = m_hdr ? (u32)m_hdr[g] & RG_GATE_FORCE : 0u;
            a = (m.term == 0 || m.from == 0) ? rg_vote_fault() : rg_vote_one<IX>(c, g, lead ? lead[g] : RG_HANDOFF_NO_LEAD, m);
            out.term[g] = a.term;
            out.commit[g] = a.commit;
            out.log_term[g] = a.log_term;
        }
        if (in) {
            out.status[g] = (u8)a.status;
            out.gate[g] = (u8)a.gate;
            out.events[g] = (u8)a.events;
        }
        const bool grant = a.gate == RG_GATE_VOTE_GRANT, reject = a.gate == RG_GATE_VOTE_REJECT || a.gate == RG_GATE_PREVOTE_LOW;
        n_req += rg_wave_count(req);
        n_grant += rg_wave_count(grant);
        n_reject += rg_wave_count(reject);
        n_ignored += rg_wave_count(a.gate == RG_GATE_IGNORED);
        n_deposed += rg_wave_count((a.events & RGV_VOTE_EV_DEPOSED) != 0);
        if (out.answered_cap) rg_wave_append(grant || reject, g, out.answered, out.answered_cap, &counts[5]); // (uniform: no list, no cursor atomic)
    }
    if ((threadIdx.x & 63u) == 0) {
        if (n_req) atomicAdd(&counts[0], (unsigned long long)n_req);
        if (n_grant) atomicAdd(&counts[1], (unsigned long long)n_grant);
        if (n_reject) atomicAdd(&counts[2], (unsigned long long)n_reject);
        if (n_ignored) atomicAdd(&counts[3], (unsigned long long)n_ignored);
        if (n_deposed) atomicAdd(&counts[4], (unsigned long long)n_deposed);
    }
}

// The sparse form: lane i = record i (checked on the host: in range, well-formed, no group twice)
template <typename IX>
__global__ __launch_bounds__(256) void k_vote_list(RgArenaCols c, const rgv_vote_rec *__restrict__ recs, u64 n, rgv_vote_resp *resp) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const rgv_vote_rec q = recs[i];
    RgVoteReq m;
    m.term = q.term;
    m.from = q.from;
    m.index = q.index;
    m.log_term = q.log_term;
    m.commit = q.commit;
    m.commit_term = q.commit_term;
    m.priority = q.priority;
    m.kind = q.kind;
    m.hdr_flags = q.flags;
    resp[i] = rg_vote_one<IX>(c, q.follow_group, q.lead_group, m);
}
