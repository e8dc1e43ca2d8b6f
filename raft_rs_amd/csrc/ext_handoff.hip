// ext_handoff.hip -- the promotion into an engine with device Inflights (include/raftgroups_handoff.h, the fourth extension header:
// its entry points are rgh_*): rg_follow_promote*'s promotion, the window resets of Raft::reset and the first appends of the new
// leader in one launch, the work items into the CALLER's memory. The unit keeps no state of its own and touches none of the
// engine's send-stage bookkeeping.
// There is NO CPU fallback anywhere in this file: without a HIP device every entry point fails.
#include "rg_engine.h"
#pragma GCC visibility push(default) // (the build hides everything else: the exports are the header's declarations, as in rg_engine.h)
#include "../../include/raftgroups_handoff.h"
#pragma GCC visibility pop
#include "rg_handoff_host.h"
#include "rg_kernels_promote.h"

extern "C" uint32_t rgh_handoff_version(void) { return RGH_HANDOFF_VERSION; }

// What both forms need of the engine, all of it decided on the host; 0 = fine. (Groups that still carry RG_OUT_HOST_HINT are refused
// where every next step refuses them: RG_ENTER_STEP, in front of anything this unit stages or launches.)
static int rgh_promote_state(rg_engine *h, uint32_t flags, const char *who) {
    if (!h->ins_arena)
        return rg_fail(RG_ERR_STATE, "%s: the engine holds no device Inflights (max_inflight = 0); its promotion is rg_follow_promote / rg_follow_promote_device", who);
    if (int rc = rg_elect_enabled(h, who)) return rc;
    if (int rc = rg_send_check(h, flags, who)) return rc; // unknown flags; RG_SEND_BYTES without the size table
    if (h->send_ready)
        return rg_fail(RG_ERR_STATE, "%s: the last tick's send stage is still owed (rg_send_appends): its result words describe windows this call would empty", who);
    return RG_OK;
}

// One launch of kernel<P, IX> for the engine's slot count and index width over `blocks` blocks of 256 threads
#define RGH_LAUNCH(h, kernel, blocks, ...)                                                                                      \
    rg_with_p((h)->P, [&](auto p) {                                                                                             \
        constexpr int P_ = decltype(p)::value;                                                                                  \
        if (rg_ix32((h)->st, (h)->P)) hipLaunchKernelGGL((kernel<P_, u32>), dim3(blocks), dim3(256), 0, (h)->stream, __VA_ARGS__); \
        else hipLaunchKernelGGL((kernel<P_, u64>), dim3(blocks), dim3(256), 0, (h)->stream, __VA_ARGS__);                        \
    })

extern "C" int rgh_follow_promote(rg_engine *h, const rg_handoff_rec *host_recs, uint64_t n, rg_handoff_resp *host_resp, uint64_t max_entries_per_msg,
                                  uint32_t flags, rg_send_item *host_items, uint64_t item_cap, uint64_t *n_items) try {
    (void)max_entries_per_msg; // (a first append carries one entry: rg_promote.h)
    if (!h || !n_items || (n && (!host_recs || !host_resp)) || (item_cap && !host_items)) return rg_fail(RG_ERR_INVALID_ARG, "rgh_follow_promote: bad argument");
    if (int src = rgh_promote_state(h, flags, "rgh_follow_promote")) return src;
    if (int crc = rg_walk_pairs(h, "rgh_follow_promote", host_recs, n, 0)) return crc;
    if (const u64 i = rg_handoff_first_queued(h, host_recs, n); i < n)
        return rg_fail(RG_ERR_SLOT_BUSY, "rgh_follow_promote: record %llu: lead group %llu has events queued (they belong to the old term); rg_flush first",
                       (unsigned long long)i, (unsigned long long)host_recs[i].lead_group);
    *n_items = 0;
    RG_ENTER_STEP(h, "rgh_follow_promote");
    if (n == 0) return RG_OK;
    // staged: recs | resp | count -- and behind them, never uploaded, room for the items the caller can take
    const u64 dev_cap = item_cap < n * h->P ? item_cap : n * h->P;
    RgLayout lay;
    lay.add(n * sizeof(rg_handoff_rec));
    const size_t off_resp = lay.add(n * sizeof(rg_handoff_resp)), off_count = lay.add(8), staged = lay.total, off_items = lay.add(dev_cap * sizeof(rg_send_item));
    if (int rc = rg_stage_reserve(h, lay.total)) return rc;
    std::vector<char> &stage = h->fo->stage;
    stage.assign(staged, 0);
    memcpy(stage.data(), host_recs, n * sizeof(rg_handoff_rec));
    u32 count = 0;
    const RgFollowEngine *fo = h->fo;
    int rc = rg_follow_round_trip(h, "rgh_follow_promote", stage.data(), staged, [&](char *d) {
        const RgPromoteItems o = {reinterpret_cast<rg_send_item *>(d + off_items), dev_cap, reinterpret_cast<u32 *>(d + off_count)};
        RGH_LAUNCH(h, k_promote_send_list, rg_grid(n, 256), h->st, h->ins, h->esz, fo->cols, fo->soft, fo->elect, reinterpret_cast<const rg_handoff_rec *>(d), (u64)n,
                   reinterpret_cast<rg_handoff_resp *>(d + off_resp), o);
    }, {{host_resp, off_resp, n * sizeof(rg_handoff_resp)}, {&count, off_count, 4}});
    if (rc) return rc;
    rg_handoff_promoted(h);
    rg_handoff_registered(h, host_recs, host_resp, n);
    *n_items = count;
    if (const u64 k = count < dev_cap ? count : dev_cap) { // (the staging is still this call's: nothing ran since the round trip)
        RG_HIP(hipMemcpyAsync(host_items, static_cast<char *>(h->d_recs) + off_items, k * sizeof(rg_send_item), hipMemcpyDeviceToHost, h->stream));
        RG_HIP(hipStreamSynchronize(h->stream));
    }
    return RG_OK;
} RG_ABI_GUARD

extern "C" int rgh_follow_promote_device(rg_engine *h, const uint8_t *dev_result, const uint64_t *dev_lead, const uint64_t *dev_persisted,
                                         uint64_t max_entries_per_msg, uint32_t flags, const rgh_promote_out *dev_out) try {
    (void)max_entries_per_msg;
    if (!h || !dev_result || !dev_lead || !dev_out) return rg_fail(RG_ERR_INVALID_ARG, "rgh_follow_promote_device: bad argument");
    if (!rg_handoff_out_complete(dev_out->out) || !dev_out->count || (dev_out->item_cap && !dev_out->items))
        return rg_fail(RG_ERR_INVALID_ARG, "rgh_follow_promote_device: an output column, the count word or the item list is NULL");
    if (int src = rgh_promote_state(h, flags, "rgh_follow_promote_device")) return src;
    if (h->host_mirror) return rg_fail(RG_ERR_STATE, "rgh_follow_promote_device: the engine has a host mirror, whose term gate lives on the host; rgh_follow_promote");
    RG_ENTER_STEP(h, "rgh_follow_promote_device");
    const RgFollowEngine *fo = h->fo;
    const RgPromoteItems o = {dev_out->items, dev_out->item_cap, dev_out->count};
    RG_HIP(hipMemsetAsync(dev_out->count, 0, 4, h->stream));
    RGH_LAUNCH(h, k_promote_send_dense, rg_grid(fo->cols.n, 256), h->st, h->ins, h->esz, fo->cols, fo->soft, fo->elect, dev_result, (const u64 *)dev_lead,
               (const u64 *)dev_persisted, dev_out->out, o);
    if (int rc = rg_launch_check("rgh_follow_promote_device")) return rc;
    rg_handoff_promoted(h);
    return RG_OK;
} RG_ABI_GUARD
