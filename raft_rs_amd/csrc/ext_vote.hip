// ext_vote.hip -- the dense vote step (include/raftgroups_vote.h, the third extension header: its entry points are rgv_*):
// MsgRequestVote / MsgRequestPreVote for every followed group in one launch, the groups this store leads judged as a leader judges
// them and a leader deposed by a real vote of a higher term taken back into the arena in the same launch. The unit keeps no state
// of its own: its five count words and the cursor of the answered list are RG_COUNTS_VOTE of the engine's d_counts scratch
// (rg_engine.h).
// There is NO CPU fallback anywhere in this file: without a HIP device every entry point fails.
#include "rg_engine.h"
#pragma GCC visibility push(default) // (the build hides everything else: the exports are the header's declarations, as in rg_engine.h)
#include "../../include/raftgroups_vote.h"
#pragma GCC visibility pop
#include "rg_handoff_host.h"
#include "rg_kernels_vote.h"

#define RG_VOTE_MAX_BLOCKS 1024u /* of the dense launch: four blocks per CU of an MI355X; what bounds the count atomics */
static unsigned long long *rg_vote_counts(const rg_engine *h) { return reinterpret_cast<unsigned long long *>(h->d_counts + RG_COUNTS_VOTE); }

extern "C" uint32_t rgv_vote_version(void) { return RGV_VOTE_VERSION; }

extern "C" const uint64_t *rgv_follow_vote_counts(const rg_engine *h) { return h ? reinterpret_cast<const uint64_t *>(rg_vote_counts(h)) : nullptr; }

// What both forms need of the engine: the election layer, and ONE Config across the arena's gate and the leader's clock
static int rg_vote_state(rg_engine *h, const char *who) {
    if (int rc = rg_elect_enabled(h, who)) return rc;
    if (h->ld && ((h->ld->cols.cfg.flags ^ h->fo->soft.cfg.flags) & RG_GATE_CHECK_QUORUM))
        return rg_fail(RG_ERR_STATE, "%s: RG_GATE_CHECK_QUORUM of the leader's clock differs from the arena gate's (a store has one Config)", who);
    return RG_OK;
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
    rgv_vote_out out = *dev_out;
    if (!out.answered) out.answered_cap = 0;
    unsigned long long *counts = rg_vote_counts(h);
    RG_HIP(hipMemsetAsync(counts, 0, RG_COUNTS_VOTE_N * 8, h->stream));
    const u64 tiles = rg_grid(h->fo->cols.n, 256); // (a block walks tiles: rg_kernels_vote.h)
    RG_LAUNCH_IX(h, k_vote_dense, (unsigned)(tiles < RG_VOTE_MAX_BLOCKS ? tiles : RG_VOTE_MAX_BLOCKS), rg_arena_cols(h), *dev_msgs, (const u64 *)dev_term,
                 (const u64 *)dev_from, dev_priority, dev_hdr_flags, (const u64 *)dev_lead, out, counts);
    if (int rc = rg_launch_check("rgv_follow_vote_device")) return rc;
    return rg_fetch_counts(h, host_counts, counts, (RG_COUNTS_VOTE_N - 1) * 8); // (without the cursor)
} RG_ABI_GUARD

extern "C" int rgv_follow_vote(rg_engine *h, const rgv_vote_rec *host_recs, uint64_t n, rgv_vote_resp *host_resp) try {
    if (!h || (n && (!host_recs || !host_resp))) return rg_fail(RG_ERR_INVALID_ARG, "rgv_follow_vote: bad argument");
    if (int src = rg_vote_state(h, "rgv_follow_vote")) return src;
    const auto rule = [](const rgv_vote_rec &q, u64 i) {
        if (!rg_vote_is_request(q.kind) || q.term == 0 || q.from == 0 || (q.flags & ~RG_GATE_FORCE))
            return rg_fail(RG_ERR_INVALID_ARG, "rgv_follow_vote: record %llu: kind 0x%x, term %llu, from %llu, flags 0x%x", (unsigned long long)i, q.kind,
                           (unsigned long long)q.term, (unsigned long long)q.from, q.flags);
        return (int)RG_OK;
    };
    if (int crc = rg_walk_pairs(h, "rgv_follow_vote", host_recs, n, RG_WALK_NO_LEAD_OK | RG_WALK_SIDE_IN_WHO, rule)) return crc;
    if (n == 0) return RG_OK;
    RG_ENTER(h);
    const RgArenaCols c = rg_arena_cols(h);
    if (h->host_mirror) h->host_cfg_valid = false; // transferee bits may go: the mirror re-reads its copy
    return rg_list_round_trip(h, "rgv_follow_vote", host_recs, n, host_resp, [&](const rgv_vote_rec *d_recs, rgv_vote_resp *d_resp) {
        RG_LAUNCH_IX(h, k_vote_list, rg_grid(n, 256), c, d_recs, n, d_resp);
    });
} RG_ABI_GUARD
