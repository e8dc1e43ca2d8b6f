// abi_handoff.hip -- the hand-off between the follower arena and the leader columns (include/raftgroups.h: "The hand-off"):
// promotion of a followed group that won its election, demotion of a group this store has been leading. No state of its own.
// There is NO CPU fallback anywhere in this file: without a HIP device every entry point fails.
#include "rg_engine.h"
#include "rg_kernels_handoff.h"

// What both promotions need of the engine; 0 = fine.
static int rg_handoff_promote_state(rg_engine *h, const char *who) {
    if (!h->fo || !h->fo->has(RG_FL_ELECT)) return rg_fail(RG_ERR_STATE, "%s: rg_follow_elect_enable first", who);
    if (h->ins_arena)
        return rg_fail(RG_ERR_STATE, "%s: the engine holds device Inflights (max_inflight > 0), whose windows only a tick's send stage empties", who);
    return RG_OK;
}
// ... and what a promotion leaves behind on the host side of the engine
static void rg_handoff_promoted(rg_engine *h) {
    if (h->pub) h->pub->local_lost = true; // RG_COL_COMMIT was written outside a tick: the published advances no longer describe it
    h->host_res_valid = false;
}

static bool rg_handoff_out_complete(const rg_handoff_out &o) { return o.status && o.term && o.last_index; }

// The host checks of both sparse forms: groups in range, no follow group and no lead group twice.
static int rg_handoff_check_recs(rg_engine *h, const char *who, const rg_handoff_rec *recs, u64 n) {
    RgSeen seen_f, seen_l;
    for (u64 i = 0; i < n; i++) {
        const rg_handoff_rec &q = recs[i];
        if (q.follow_group >= h->fo->cols.n || q.lead_group >= h->G)
            return rg_fail(RG_ERR_INVALID_ARG, "%s: record %llu: follow group %llu of %llu, lead group %llu of %llu", who, (unsigned long long)i,
                           (unsigned long long)q.follow_group, (unsigned long long)h->fo->cols.n, (unsigned long long)q.lead_group, (unsigned long long)h->G);
        if (!seen_f.emplace(q.follow_group, i).second)
            return rg_fail(RG_ERR_INVALID_ARG, "%s: records %llu and %llu name follow group %llu", who, (unsigned long long)seen_f[q.follow_group],
                           (unsigned long long)i, (unsigned long long)q.follow_group);
        if (!seen_l.emplace(q.lead_group, i).second)
            return rg_fail(RG_ERR_INVALID_ARG, "%s: records %llu and %llu name lead group %llu", who, (unsigned long long)seen_l[q.lead_group],
                           (unsigned long long)i, (unsigned long long)q.lead_group);
    }
    return RG_OK;
}

// Stage the records, run one lane per record, fetch the answers. Synchronises: the staging is reused by the next call.
static int rg_handoff_run_list(rg_engine *h, const char *who, bool promote, const rg_handoff_rec *recs, u64 n, rg_handoff_resp *host_resp) {
    RgFollowEngine *fo = h->fo;
    RgLayout lay;
    lay.add(n * sizeof(rg_handoff_rec));
    const size_t off_resp = lay.add(n * sizeof(rg_handoff_resp));
    fo->stage.assign(lay.total, 0);
    memcpy(fo->stage.data(), recs, n * sizeof(rg_handoff_rec));
    return rg_follow_round_trip(h, who, fo->stage.data(), lay.total, [&](char *d) {
        const rg_handoff_rec *d_recs = reinterpret_cast<const rg_handoff_rec *>(d);
        rg_handoff_resp *d_resp = reinterpret_cast<rg_handoff_resp *>(d + off_resp);
        const dim3 grid(rg_grid(n, 256)), block(256);
        const bool ix32 = rg_ix32(h->st, h->P);
        if (promote) {
            if (ix32) hipLaunchKernelGGL(k_handoff_promote_list<u32>, grid, block, 0, h->stream, h->st, fo->cols, fo->soft, fo->elect, h->P, d_recs, n, d_resp);
            else hipLaunchKernelGGL(k_handoff_promote_list<u64>, grid, block, 0, h->stream, h->st, fo->cols, fo->soft, fo->elect, h->P, d_recs, n, d_resp);
        } else {
            if (ix32) hipLaunchKernelGGL(k_handoff_demote_list<u32>, grid, block, 0, h->stream, h->st, fo->cols, d_recs, n, d_resp);
            else hipLaunchKernelGGL(k_handoff_demote_list<u64>, grid, block, 0, h->stream, h->st, fo->cols, d_recs, n, d_resp);
        }
    }, {{host_resp, off_resp, n * sizeof(rg_handoff_resp)}});
}

extern "C" int rg_follow_promote(rg_engine *h, const rg_handoff_rec *host_recs, uint64_t n, rg_handoff_resp *host_resp) try {
    if (!h || (n && (!host_recs || !host_resp))) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_promote: bad argument");
    if (int src = rg_handoff_promote_state(h, "rg_follow_promote")) return src;
    if (int crc = rg_handoff_check_recs(h, "rg_follow_promote", host_recs, n)) return crc;
    if (h->host_mirror) // events queued for the lead group belong to the old term (rg_local_become_leader's rule)
        for (u64 i = 0; i < n; i++) {
            u64 row = 0;
            memcpy(&row, &h->q_mf[host_recs[i].lead_group * 8], 8);
            if (row)
                return rg_fail(RG_ERR_SLOT_BUSY, "rg_follow_promote: record %llu: lead group %llu has events queued (they belong to the old term); rg_flush first",
                               (unsigned long long)i, (unsigned long long)host_recs[i].lead_group);
        }
    if (n == 0) return RG_OK;
    RG_ENTER(h);
    int rc = rg_handoff_run_list(h, "rg_follow_promote", true, host_recs, n, host_resp);
    if (rc) return rc;
    rg_handoff_promoted(h);
    for (u64 i = 0; i < n; i++) {
        if (host_resp[i].status != RG_HANDOFF_DONE) continue;
        const u64 L = host_recs[i].lead_group;
        if (h->host_mirror) h->terms[L] = host_resp[i].term; // RG_COL_CUR_TERM and the registered term of a group belong together
        if (h->host_cfg_valid) h->host_cfg[L] &= ~(0xfu << 20); // (the transferee, if there was one, is gone)
    }
    return RG_OK;
} RG_ABI_GUARD

extern "C" int rg_follow_promote_device(rg_engine *h, const uint8_t *dev_result, const uint64_t *dev_lead, const uint64_t *dev_persisted,
                                        const rg_handoff_out *dev_out) try {
    if (!h || !dev_result || !dev_lead || !dev_out) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_promote_device: bad argument");
    if (int src = rg_handoff_promote_state(h, "rg_follow_promote_device")) return src;
    if (h->host_mirror) return rg_fail(RG_ERR_STATE, "rg_follow_promote_device: the engine has a host mirror, whose term gate lives on the host; rg_follow_promote");
    if (!rg_handoff_out_complete(*dev_out)) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_promote_device: an output column is NULL");
    RG_ENTER(h);
    RgFollowEngine *fo = h->fo;
    const dim3 grid(rg_grid(fo->cols.n, 256)), block(256);
    if (rg_ix32(h->st, h->P))
        hipLaunchKernelGGL(k_handoff_promote_dense<u32>, grid, block, 0, h->stream, h->st, fo->cols, fo->soft, fo->elect, h->P, dev_result, dev_lead, dev_persisted,
                           *dev_out);
    else
        hipLaunchKernelGGL(k_handoff_promote_dense<u64>, grid, block, 0, h->stream, h->st, fo->cols, fo->soft, fo->elect, h->P, dev_result, dev_lead, dev_persisted,
                           *dev_out);
    if (int rc = rg_launch_check("rg_follow_promote_device")) return rc;
    rg_handoff_promoted(h);
    return RG_OK;
} RG_ABI_GUARD

extern "C" int rg_follow_demote(rg_engine *h, const rg_handoff_rec *host_recs, uint64_t n, rg_handoff_resp *host_resp) try {
    if (!h || (n && (!host_recs || !host_resp))) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_demote: bad argument");
    if (!h->fo) return rg_fail(RG_ERR_STATE, "rg_follow_demote: rg_follow_enable first");
    if (int crc = rg_handoff_check_recs(h, "rg_follow_demote", host_recs, n)) return crc;
    if (n == 0) return RG_OK;
    RG_ENTER(h);
    return rg_handoff_run_list(h, "rg_follow_demote", false, host_recs, n, host_resp);
} RG_ABI_GUARD

extern "C" int rg_follow_demote_device(rg_engine *h, const uint8_t *dev_select, const uint64_t *dev_lead, const rg_handoff_out *dev_out) try {
    if (!h || !dev_select || !dev_lead || !dev_out) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_demote_device: bad argument");
    if (!h->fo) return rg_fail(RG_ERR_STATE, "rg_follow_demote_device: rg_follow_enable first");
    if (h->host_mirror) return rg_fail(RG_ERR_STATE, "rg_follow_demote_device: the engine has a host mirror; rg_follow_demote");
    if (!rg_handoff_out_complete(*dev_out)) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_demote_device: an output column is NULL");
    RG_ENTER(h);
    RgFollowEngine *fo = h->fo;
    const dim3 grid(rg_grid(fo->cols.n, 256)), block(256);
    if (rg_ix32(h->st, h->P)) hipLaunchKernelGGL(k_handoff_demote_dense<u32>, grid, block, 0, h->stream, h->st, fo->cols, dev_select, dev_lead, *dev_out);
    else hipLaunchKernelGGL(k_handoff_demote_dense<u64>, grid, block, 0, h->stream, h->st, fo->cols, dev_select, dev_lead, *dev_out);
    return rg_launch_check("rg_follow_demote_device");
} RG_ABI_GUARD
