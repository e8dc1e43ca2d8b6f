// ext_vote.hip -- the dense vote step (include/raftgroups_vote.h, the third extension header: its entry points are rgv_*):
// MsgRequestVote / MsgRequestPreVote for every followed group in one launch, the groups this store leads judged as a leader judges
// them and a leader deposed by a real vote of a higher term taken back into the arena in the same launch. The unit keeps no state
// of its own: its five count words and the cursor of the answered list are words 16..21 of the engine's d_counts scratch (rg_create
// sets 256 bytes aside; the reductions of abi_tick.hip use the first 40, ext_term.hip words 8..10).
// There is NO CPU fallback anywhere in this file: without a HIP device every entry point fails.
#include "rg_engine.h"
#pragma GCC visibility push(default) // (the build hides everything else: the exports are the header's declarations, as in rg_engine.h)
#include "../../include/raftgroups_vote.h"
#pragma GCC visibility pop
#include "rg_kernels_vote.h"

#define RG_VOTE_COUNTS_AT 16 /* u64 words into rg_engine::d_counts */
#define RG_VOTE_MAX_BLOCKS 1024u /* of the dense launch: four blocks per CU of an MI355X; what bounds the count atomics */
static unsigned long long *rg_vote_counts(const rg_engine *h) { return reinterpret_cast<unsigned long long *>(h->d_counts + RG_VOTE_COUNTS_AT); }

extern "C" uint32_t rgv_vote_version(void) { return RGV_VOTE_VERSION; }

extern "C" const uint64_t *rgv_follow_vote_counts(const rg_engine *h) { return h ? reinterpret_cast<const uint64_t *>(rg_vote_counts(h)) : nullptr; }

// What both forms need of the engine: the election layer, and ONE Config across the arena's gate and the leader's clock
static int rg_vote_state(rg_engine *h, const char *who) {
    if (!h->fo || !h->fo->has(RG_FL_ELECT)) return rg_fail(RG_ERR_STATE, "%s: rg_follow_elect_enable first", who);
    if (h->ld && ((h->ld->cols.cfg.flags ^ h->fo->soft.cfg.flags) & RG_GATE_CHECK_QUORUM))
        return rg_fail(RG_ERR_STATE, "%s: RG_GATE_CHECK_QUORUM of the leader's clock differs from the arena gate's (a store has one Config)", who);
    return RG_OK;
}
static RgVoteCols rg_vote_cols(rg_engine *h) {
    RgVoteCols c;
    c.st = h->st;
    c.fc = h->fo->cols;
    c.sc = h->fo->soft;
    c.ec = h->fo->elect;
    c.lc = h->ld ? h->ld->cols : RgLeadCols{}; // (cell == nullptr: the clock layer is off)
    c.read_qterm = h->rd ? h->rd->cols.qterm : nullptr; // (looked up per call: either enable order)
    return c;
}

extern "C" int rgv_follow_vote_device(rg_engine *h, const rg_follow_msgs *dev_msgs, const uint64_t *dev_term, const uint64_t *dev_from,
                                      const int64_t *dev_priority, const uint8_t *dev_hdr_flags, const uint64_t *dev_lead,
                                      const rgv_vote_out *dev_out, uint64_t *host_counts) try {
    if (!h || !dev_msgs || !dev_term || !dev_from || !dev_out) return rg_fail(RG_ERR_INVALID_ARG, "rgv_follow_vote_device: bad argument");
    if (!dev_msgs->flags || !dev_msgs->index || !dev_msgs->log_term || !dev_msgs->commit || !dev_msgs->ent_term)
        return rg_fail(RG_ERR_INVALID_ARG, "rgv_follow_vote_device: a request column is NULL");
    if (!dev_out->status || !dev_out->gate || !dev_out->events || !dev_out->term || !dev_out->commit || !dev_out->log_term ||
        (dev_out->answered_cap && !dev_out->answered))
        return rg_fail(RG_ERR_INVALID_ARG, "rgv_follow_vote_device: an output column is NULL");
    if (int src = rg_vote_state(h, "rgv_follow_vote_device")) return src;
    if (dev_lead && h->host_mirror) return rg_fail(RG_ERR_STATE, "rgv_follow_vote_device: the engine has a host mirror; rgv_follow_vote");
    RG_ENTER(h);
    RgFollowEngine *fo = h->fo;
    rgv_vote_out out = *dev_out;
    if (!out.answered) out.answered_cap = 0;
    unsigned long long *counts = rg_vote_counts(h);
    RG_HIP(hipMemsetAsync(counts, 0, 48, h->stream));
    const u64 tiles = rg_grid(fo->cols.n, 256);
    const dim3 grid((unsigned)(tiles < RG_VOTE_MAX_BLOCKS ? tiles : RG_VOTE_MAX_BLOCKS)), block(256); // (a block walks tiles: rg_kernels_vote.h)
    const RgVoteCols c = rg_vote_cols(h);
    if (rg_ix32(h->st, h->P))
        hipLaunchKernelGGL(k_vote_dense<u32>, grid, block, 0, h->stream, c, *dev_msgs, (const u64 *)dev_term, (const u64 *)dev_from, dev_priority, dev_hdr_flags,
                           (const u64 *)dev_lead, out, counts);
    else
        hipLaunchKernelGGL(k_vote_dense<u64>, grid, block, 0, h->stream, c, *dev_msgs, (const u64 *)dev_term, (const u64 *)dev_from, dev_priority, dev_hdr_flags,
                           (const u64 *)dev_lead, out, counts);
    if (int rc = rg_launch_check("rgv_follow_vote_device")) return rc;
    if (host_counts) {
        RG_HIP(hipMemcpyAsync(host_counts, counts, 40, hipMemcpyDeviceToHost, h->stream));
        RG_HIP(hipStreamSynchronize(h->stream));
    }
    return RG_OK;
} RG_ABI_GUARD

extern "C" int rgv_follow_vote(rg_engine *h, const rgv_vote_rec *host_recs, uint64_t n, rgv_vote_resp *host_resp) try {
    if (!h || (n && (!host_recs || !host_resp))) return rg_fail(RG_ERR_INVALID_ARG, "rgv_follow_vote: bad argument");
    if (int src = rg_vote_state(h, "rgv_follow_vote")) return src;
    RgFollowEngine *fo = h->fo;
    RgSeen seen_f, seen_l;
    for (u64 i = 0; i < n; i++) {
        const rgv_vote_rec &q = host_recs[i];
        if (q.follow_group >= fo->cols.n || (q.lead_group >= h->G && q.lead_group != RG_HANDOFF_NO_LEAD))
            return rg_fail(RG_ERR_INVALID_ARG, "rgv_follow_vote: record %llu: follow group %llu of %llu, lead group %llu of %llu", (unsigned long long)i,
                           (unsigned long long)q.follow_group, (unsigned long long)fo->cols.n, (unsigned long long)q.lead_group, (unsigned long long)h->G);
        if (!rg_vote_is_request(q.kind) || q.term == 0 || q.from == 0 || (q.flags & ~RG_GATE_FORCE))
            return rg_fail(RG_ERR_INVALID_ARG, "rgv_follow_vote: record %llu: kind 0x%x, term %llu, from %llu, flags 0x%x", (unsigned long long)i, q.kind,
                           (unsigned long long)q.term, (unsigned long long)q.from, q.flags);
        if (int rc = rg_named_once("rgv_follow_vote (follow)", seen_f.emplace(q.follow_group, i), i)) return rc;
        if (q.lead_group != RG_HANDOFF_NO_LEAD)
            if (int rc = rg_named_once("rgv_follow_vote (lead)", seen_l.emplace(q.lead_group, i), i)) return rc;
    }
    if (n == 0) return RG_OK;
    RG_ENTER(h);
    RgLayout lay;
    lay.add(n * sizeof(rgv_vote_rec));
    const size_t off_resp = lay.add(n * sizeof(rgv_vote_resp));
    fo->stage.assign(lay.total, 0);
    memcpy(fo->stage.data(), host_recs, n * sizeof(rgv_vote_rec));
    const RgVoteCols c = rg_vote_cols(h);
    if (h->host_mirror) h->host_cfg_valid = false; // transferee bits may go: the mirror re-reads its copy
    return rg_follow_round_trip(h, "rgv_follow_vote", fo->stage.data(), lay.total, [&](char *d) {
        const rgv_vote_rec *d_recs = reinterpret_cast<const rgv_vote_rec *>(d);
        rgv_vote_resp *d_resp = reinterpret_cast<rgv_vote_resp *>(d + off_resp);
        const dim3 grid(rg_grid(n, 256)), block(256);
        if (rg_ix32(h->st, h->P)) hipLaunchKernelGGL(k_vote_list<u32>, grid, block, 0, h->stream, c, d_recs, n, d_resp);
        else hipLaunchKernelGGL(k_vote_list<u64>, grid, block, 0, h->stream, c, d_recs, n, d_resp);
    }, {{host_resp, off_resp, n * sizeof(rgv_vote_resp)}});
} RG_ABI_GUARD
