// abi_handoff.hip -- the hand-off between the follower arena and the leader columns (include/raftgroups.h: "The hand-off"):
// promotion of a followed group that won its election, demotion of a group this store has been leading. No state of its own.
// There is NO CPU fallback anywhere in this file: without a HIP device every entry point fails.
#include "rg_engine.h"
#include "rg_handoff_host.h"

// What both promotions need of the engine; 0 = fine.
static int rg_handoff_promote_state(rg_engine *h, const char *who) {
    if (int rc = rg_elect_enabled(h, who)) return rc;
    if (h->ins_arena)
        return rg_fail(RG_ERR_STATE, "%s: the engine holds device Inflights (max_inflight > 0), whose windows only a tick's send stage empties", who);
    return RG_OK;
}
// ... and what a promotion leaves behind on the host side of the engine: rg_handoff_promoted, rg_handoff_registered (rg_handoff_host.h)

extern "C" int rg_follow_promote(rg_engine *h, const rg_handoff_rec *host_recs, uint64_t n, rg_handoff_resp *host_resp) try {
    if (!h || (n && (!host_recs || !host_resp))) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_promote: bad argument");
    if (int src = rg_handoff_promote_state(h, "rg_follow_promote")) return src;
    if (int crc = rg_walk_pairs(h, "rg_follow_promote", host_recs, n, 0)) return crc;
    if (const u64 i = rg_handoff_first_queued(h, host_recs, n); i < n)
        return rg_fail(RG_ERR_SLOT_BUSY, "rg_follow_promote: record %llu: lead group %llu has events queued (they belong to the old term); rg_flush first",
                       (unsigned long long)i, (unsigned long long)host_recs[i].lead_group);
    if (n == 0) return RG_OK;
    RG_ENTER(h);
    RgFollowEngine *fo = h->fo;
    int rc = rg_list_round_trip(h, "rg_follow_promote", host_recs, n, host_resp, [&](const rg_handoff_rec *d_recs, rg_handoff_resp *d_resp) {
        RG_LAUNCH_IX(h, k_handoff_promote_list, rg_grid(n, 256), h->st, fo->cols, fo->soft, fo->elect, h->P, d_recs, n, d_resp);
    });
    if (rc) return rc;
    rg_handoff_promoted(h);
    rg_handoff_registered(h, host_recs, host_resp, n);
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
    RG_LAUNCH_IX(h, k_handoff_promote_dense, rg_grid(fo->cols.n, 256), h->st, fo->cols, fo->soft, fo->elect, h->P, dev_result, dev_lead, dev_persisted, *dev_out);
    if (int rc = rg_launch_check("rg_follow_promote_device")) return rc;
    rg_handoff_promoted(h);
    return RG_OK;
} RG_ABI_GUARD

extern "C" int rg_follow_demote(rg_engine *h, const rg_handoff_rec *host_recs, uint64_t n, rg_handoff_resp *host_resp) try {
    if (!h || (n && (!host_recs || !host_resp))) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_demote: bad argument");
    if (!h->fo) return rg_fail(RG_ERR_STATE, "rg_follow_demote: rg_follow_enable first");
    if (int crc = rg_walk_pairs(h, "rg_follow_demote", host_recs, n, 0)) return crc;
    if (n == 0) return RG_OK;
    RG_ENTER(h);
    return rg_list_round_trip(h, "rg_follow_demote", host_recs, n, host_resp, [&](const rg_handoff_rec *d_recs, rg_handoff_resp *d_resp) {
        RG_LAUNCH_IX(h, k_handoff_demote_list, rg_grid(n, 256), h->st, h->fo->cols, d_recs, n, d_resp);
    });
} RG_ABI_GUARD

extern "C" int rg_follow_demote_device(rg_engine *h, const uint8_t *dev_select, const uint64_t *dev_lead, const rg_handoff_out *dev_out) try {
    if (!h || !dev_select || !dev_lead || !dev_out) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_demote_device: bad argument");
    if (!h->fo) return rg_fail(RG_ERR_STATE, "rg_follow_demote_device: rg_follow_enable first");
    if (h->host_mirror) return rg_fail(RG_ERR_STATE, "rg_follow_demote_device: the engine has a host mirror; rg_follow_demote");
    if (!rg_handoff_out_complete(*dev_out)) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_demote_device: an output column is NULL");
    RG_ENTER(h);
    RG_LAUNCH_IX(h, k_handoff_demote_dense, rg_grid(h->fo->cols.n, 256), h->st, h->fo->cols, dev_select, dev_lead, *dev_out);
    return rg_launch_check("rg_follow_demote_device");
} RG_ABI_GUARD
