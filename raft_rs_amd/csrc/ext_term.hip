// ext_term.hip -- the leader's term gate and the deposition (include/raftgroups_term.h, the second extension header: its entry points
// are rgt_*): the term check of Raft::step for every record of a dense leader tick in one launch, and the way back into the follower
// arena at the higher term for a group it deposed. The unit keeps no state of its own: the gate's three count words are
// RG_COUNTS_TERM of the engine's d_counts scratch (rg_engine.h).
// There is NO CPU fallback anywhere in this file: without a HIP device every entry point fails.
#include "rg_engine.h"
#include "rg_handoff_host.h"
#include "rg_kernels_term.h"

static unsigned long long *rg_term_counts(const rg_engine *h) { return reinterpret_cast<unsigned long long *>(h->d_counts + RG_COUNTS_TERM); }

extern "C" uint32_t rgt_term_version(void) { return RGT_TERM_VERSION; }

extern "C" const uint64_t *rgt_lead_gate_counts(const rg_engine *h) { return h ? reinterpret_cast<const uint64_t *>(rg_term_counts(h)) : nullptr; }

// ---- the gate: one launch over the leader engine ----
extern "C" int rgt_lead_gate_device(rg_engine *h, const rg_msgs *dev_msgs, const uint64_t *dev_m_term, const rgt_lead_gate_out *dev_out,
                                    uint64_t *host_counts) try {
    if (!h || !dev_msgs || !dev_msgs->m_flags || !dev_m_term || !dev_out || !dev_out->flags || !dev_out->events || !dev_out->new_term ||
        (dev_out->down_cap && !dev_out->down))
        return rg_fail(RG_ERR_INVALID_ARG, "rgt_lead_gate_device: bad argument");
    if ((reinterpret_cast<uintptr_t>(dev_msgs->m_flags) | reinterpret_cast<uintptr_t>(dev_out->flags)) & 7u)
        return rg_fail(RG_ERR_INVALID_ARG, "rgt_lead_gate_device: a flag column is not 8-byte aligned");
    if (!h->ld) return rg_fail(RG_ERR_STATE, "rgt_lead_gate_device: rgx_lead_clock_enable first (the clock's STOPPED bit is the record of \"led\")");
    if (h->host_mirror) return rg_fail(RG_ERR_STATE, "rgt_lead_gate_device: the engine has a host mirror; rg_step gates by its own table");
    RG_ENTER(h);
    rgt_lead_gate_out out = *dev_out;
    if (!out.down) out.down_cap = 0;
    unsigned long long *counts = rg_term_counts(h);
    RG_HIP(hipMemsetAsync(counts, 0, RG_COUNTS_TERM_N * 8, h->stream));
    RG_LAUNCH_IX(h, k_term_gate, rg_grid(h->G, 256), h->st, h->ld->cols, h->P, reinterpret_cast<const u64 *>(dev_msgs->m_flags), (const u64 *)dev_m_term,
                 reinterpret_cast<u64 *>(out.flags), out, counts, rg_read_qterm(h));
    if (int rc = rg_launch_check("rgt_lead_gate_device")) return rc;
    return rg_fetch_counts(h, host_counts, counts, RG_COUNTS_TERM_N * 8);
} RG_ABI_GUARD

// ---- the way back into the arena, at the new term ----
extern "C" int rgt_follow_depose(rg_engine *h, const rgt_depose_rec *host_recs, uint64_t n, rg_handoff_resp *host_resp) try {
    if (!h || (n && (!host_recs || !host_resp))) return rg_fail(RG_ERR_INVALID_ARG, "rgt_follow_depose: bad argument");
    if (int src = rg_elect_enabled(h, "rgt_follow_depose")) return src;
    const auto rule = [](const rgt_depose_rec &q, u64 i) {
        if (q.reserved) return rg_fail(RG_ERR_INVALID_ARG, "rgt_follow_depose: record %llu: reserved is %llu", (unsigned long long)i, (unsigned long long)q.reserved);
        return (int)RG_OK;
    };
    if (int crc = rg_walk_pairs(h, "rgt_follow_depose", host_recs, n, RG_WALK_SIDE_IN_WHO, rule)) return crc;
    if (n == 0) return RG_OK;
    RG_ENTER(h);
    const RgArenaCols c = rg_arena_cols(h);
    if (h->host_mirror) h->host_cfg_valid = false; // transferee bits may go: the mirror re-reads its copy
    return rg_list_round_trip(h, "rgt_follow_depose", host_recs, n, host_resp, [&](const rgt_depose_rec *d_recs, rg_handoff_resp *d_resp) {
        RG_LAUNCH_IX(h, k_term_depose_list, rg_grid(n, 256), c, d_recs, n, d_resp);
    });
} RG_ABI_GUARD

extern "C" int rgt_follow_depose_device(rg_engine *h, const uint8_t *dev_events, const uint64_t *dev_new_term, const uint64_t *dev_lead,
                                        const rg_handoff_out *dev_out) try {
    if (!h || !dev_events || !dev_new_term || !dev_lead || !dev_out) return rg_fail(RG_ERR_INVALID_ARG, "rgt_follow_depose_device: bad argument");
    if (int src = rg_elect_enabled(h, "rgt_follow_depose_device")) return src;
    if (h->host_mirror) return rg_fail(RG_ERR_STATE, "rgt_follow_depose_device: the engine has a host mirror; rgt_follow_depose");
    if (!rg_handoff_out_complete(*dev_out)) return rg_fail(RG_ERR_INVALID_ARG, "rgt_follow_depose_device: an output column is NULL");
    RG_ENTER(h);
    RG_LAUNCH_IX(h, k_term_depose_dense, rg_grid(h->fo->cols.n, 256), rg_arena_cols(h), dev_events, (const u64 *)dev_new_term, (const u64 *)dev_lead, *dev_out);
    return rg_launch_check("rgt_follow_depose_device");
} RG_ABI_GUARD

extern "C" int rgt_follow_depose_scan_device(rg_engine *h, const uint8_t *dev_msg_flags, const uint64_t *dev_term, const uint64_t *dev_lead,
                                             const rg_handoff_out *dev_out) try {
    if (!h || !dev_msg_flags || !dev_term || !dev_lead || !dev_out) return rg_fail(RG_ERR_INVALID_ARG, "rgt_follow_depose_scan_device: bad argument");
    if (int src = rg_elect_enabled(h, "rgt_follow_depose_scan_device")) return src;
    if (h->host_mirror) return rg_fail(RG_ERR_STATE, "rgt_follow_depose_scan_device: the engine has a host mirror; rg_follow_demote, then rg_follow_step_gated");
    if (!rg_handoff_out_complete(*dev_out)) return rg_fail(RG_ERR_INVALID_ARG, "rgt_follow_depose_scan_device: an output column is NULL");
    RG_ENTER(h);
    RG_LAUNCH_IX(h, k_term_depose_scan, rg_grid(h->fo->cols.n, 256), rg_arena_cols(h), dev_msg_flags, (const u64 *)dev_term, (const u64 *)dev_lead, *dev_out);
    return rg_launch_check("rgt_follow_depose_scan_device");
} RG_ABI_GUARD
