// ext_term.hip -- the leader's term gate and the deposition (include/raftgroups_term.h, the second extension header: its entry points
// are rgt_*): the term check of Raft::step for every record of a dense leader tick in one launch, and the way back into the follower
// arena at the higher term for a group it deposed. The unit keeps no state of its own: the gate's three count words are words 8..10
// of the engine's d_counts scratch (rg_create sets 256 bytes aside; the reductions of abi_tick.hip use the first 40).
// There is NO CPU fallback anywhere in this file: without a HIP device every entry point fails.
#include "rg_engine.h"
#include "rg_kernels_term.h"

#define RG_TERM_COUNTS_AT 8 /* u64 words into rg_engine::d_counts */
static unsigned long long *rg_term_counts(const rg_engine *h) { return reinterpret_cast<unsigned long long *>(h->d_counts + RG_TERM_COUNTS_AT); }
static u64 *rg_term_read_qterm(rg_engine *h) { return h->rd ? h->rd->cols.qterm : nullptr; } // (looked up per call: either enable order)

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
    RG_HIP(hipMemsetAsync(counts, 0, 24, h->stream));
    const dim3 grid(rg_grid(h->G, 256)), block(256);
    const u64 *m_flags = reinterpret_cast<const u64 *>(dev_msgs->m_flags);
    u64 *out_flags = reinterpret_cast<u64 *>(out.flags);
    if (rg_ix32(h->st, h->P))
        hipLaunchKernelGGL(k_term_gate<u32>, grid, block, 0, h->stream, h->st, h->ld->cols, h->P, m_flags, (const u64 *)dev_m_term, out_flags, out, counts, rg_term_read_qterm(h));
    else
        hipLaunchKernelGGL(k_term_gate<u64>, grid, block, 0, h->stream, h->st, h->ld->cols, h->P, m_flags, (const u64 *)dev_m_term, out_flags, out, counts, rg_term_read_qterm(h));
    if (int rc = rg_launch_check("rgt_lead_gate_device")) return rc;
    if (host_counts) {
        RG_HIP(hipMemcpyAsync(host_counts, counts, 24, hipMemcpyDeviceToHost, h->stream));
        RG_HIP(hipStreamSynchronize(h->stream));
    }
    return RG_OK;
} RG_ABI_GUARD

// ---- the way back into the arena, at the new term ----
static int rg_depose_state(rg_engine *h, const char *who) {
    if (!h->fo || !h->fo->has(RG_FL_ELECT)) return rg_fail(RG_ERR_STATE, "%s: rg_follow_elect_enable first", who);
    return RG_OK;
}

extern "C" int rgt_follow_depose(rg_engine *h, const rgt_depose_rec *host_recs, uint64_t n, rg_handoff_resp *host_resp) try {
    if (!h || (n && (!host_recs || !host_resp))) return rg_fail(RG_ERR_INVALID_ARG, "rgt_follow_depose: bad argument");
    if (int src = rg_depose_state(h, "rgt_follow_depose")) return src;
    RgFollowEngine *fo = h->fo;
    RgSeen seen_f, seen_l;
    for (u64 i = 0; i < n; i++) {
        const rgt_depose_rec &q = host_recs[i];
        if (q.follow_group >= fo->cols.n || q.lead_group >= h->G)
            return rg_fail(RG_ERR_INVALID_ARG, "rgt_follow_depose: record %llu: follow group %llu of %llu, lead group %llu of %llu", (unsigned long long)i,
                           (unsigned long long)q.follow_group, (unsigned long long)fo->cols.n, (unsigned long long)q.lead_group, (unsigned long long)h->G);
        if (q.reserved) return rg_fail(RG_ERR_INVALID_ARG, "rgt_follow_depose: record %llu: reserved is %llu", (unsigned long long)i, (unsigned long long)q.reserved);
        if (int rc = rg_named_once("rgt_follow_depose (follow)", seen_f.emplace(q.follow_group, i), i)) return rc;
        if (int rc = rg_named_once("rgt_follow_depose (lead)", seen_l.emplace(q.lead_group, i), i)) return rc;
    }
    if (n == 0) return RG_OK;
    RG_ENTER(h);
    RgLayout lay;
    lay.add(n * sizeof(rgt_depose_rec));
    const size_t off_resp = lay.add(n * sizeof(rg_handoff_resp));
    fo->stage.assign(lay.total, 0);
    memcpy(fo->stage.data(), host_recs, n * sizeof(rgt_depose_rec));
    const RgLeadCols cells = h->ld ? h->ld->cols : RgLeadCols{}; // (cell == nullptr: the clock layer is off)
    u64 *read_qterm = rg_term_read_qterm(h);
    if (h->host_mirror) h->host_cfg_valid = false; // transferee bits may go: the mirror re-reads its copy
    return rg_follow_round_trip(h, "rgt_follow_depose", fo->stage.data(), lay.total, [&](char *d) {
        const rgt_depose_rec *d_recs = reinterpret_cast<const rgt_depose_rec *>(d);
        rg_handoff_resp *d_resp = reinterpret_cast<rg_handoff_resp *>(d + off_resp);
        const dim3 grid(rg_grid(n, 256)), block(256);
        if (rg_ix32(h->st, h->P)) hipLaunchKernelGGL(k_term_depose_list<u32>, grid, block, 0, h->stream, h->st, fo->cols, fo->soft, fo->elect, cells, read_qterm, d_recs, n, d_resp);
        else hipLaunchKernelGGL(k_term_depose_list<u64>, grid, block, 0, h->stream, h->st, fo->cols, fo->soft, fo->elect, cells, read_qterm, d_recs, n, d_resp);
    }, {{host_resp, off_resp, n * sizeof(rg_handoff_resp)}});
} RG_ABI_GUARD

extern "C" int rgt_follow_depose_device(rg_engine *h, const uint8_t *dev_events, const uint64_t *dev_new_term, const uint64_t *dev_lead,
                                        const rg_handoff_out *dev_out) try {
    if (!h || !dev_events || !dev_new_term || !dev_lead || !dev_out) return rg_fail(RG_ERR_INVALID_ARG, "rgt_follow_depose_device: bad argument");
    if (int src = rg_depose_state(h, "rgt_follow_depose_device")) return src;
    if (h->host_mirror) return rg_fail(RG_ERR_STATE, "rgt_follow_depose_device: the engine has a host mirror; rgt_follow_depose");
    if (!dev_out->status || !dev_out->term || !dev_out->last_index) return rg_fail(RG_ERR_INVALID_ARG, "rgt_follow_depose_device: an output column is NULL");
    RG_ENTER(h);
    RgFollowEngine *fo = h->fo;
    const RgLeadCols cells = h->ld ? h->ld->cols : RgLeadCols{};
    const dim3 grid(rg_grid(fo->cols.n, 256)), block(256);
    if (rg_ix32(h->st, h->P))
        hipLaunchKernelGGL(k_term_depose_dense<u32>, grid, block, 0, h->stream, h->st, fo->cols, fo->soft, fo->elect, cells, rg_term_read_qterm(h), dev_events,
                           (const u64 *)dev_new_term, (const u64 *)dev_lead, *dev_out);
    else
        hipLaunchKernelGGL(k_term_depose_dense<u64>, grid, block, 0, h->stream, h->st, fo->cols, fo->soft, fo->elect, cells, rg_term_read_qterm(h), dev_events,
                           (const u64 *)dev_new_term, (const u64 *)dev_lead, *dev_out);
    return rg_launch_check("rgt_follow_depose_device");
} RG_ABI_GUARD

extern "C" int rgt_follow_depose_scan_device(rg_engine *h, const uint8_t *dev_msg_flags, const uint64_t *dev_term, const uint64_t *dev_lead,
                                             const rg_handoff_out *dev_out) try {
    if (!h || !dev_msg_flags || !dev_term || !dev_lead || !dev_out) return rg_fail(RG_ERR_INVALID_ARG, "rgt_follow_depose_scan_device: bad argument");
    if (int src = rg_depose_state(h, "rgt_follow_depose_scan_device")) return src;
    if (h->host_mirror) return rg_fail(RG_ERR_STATE, "rgt_follow_depose_scan_device: the engine has a host mirror; rg_follow_demote, then rg_follow_step_gated");
    if (!dev_out->status || !dev_out->term || !dev_out->last_index) return rg_fail(RG_ERR_INVALID_ARG, "rgt_follow_depose_scan_device: an output column is NULL");
    RG_ENTER(h);
    RgFollowEngine *fo = h->fo;
    const RgLeadCols cells = h->ld ? h->ld->cols : RgLeadCols{};
    const dim3 grid(rg_grid(fo->cols.n, 256)), block(256);
    if (rg_ix32(h->st, h->P))
        hipLaunchKernelGGL(k_term_depose_scan<u32>, grid, block, 0, h->stream, h->st, fo->cols, fo->soft, fo->elect, cells, rg_term_read_qterm(h), dev_msg_flags,
                           (const u64 *)dev_term, (const u64 *)dev_lead, *dev_out);
    else
        hipLaunchKernelGGL(k_term_depose_scan<u64>, grid, block, 0, h->stream, h->st, fo->cols, fo->soft, fo->elect, cells, rg_term_read_qterm(h), dev_msg_flags,
                           (const u64 *)dev_term, (const u64 *)dev_lead, *dev_out);
    return rg_launch_check("rgt_follow_depose_scan_device");
} RG_ABI_GUARD
