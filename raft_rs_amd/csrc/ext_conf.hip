// ext_conf.hip -- the batched conf change (include/raftgroups_conf.h, the fifth extension header: its entry points are rgc_*):
// ProgressTracker::apply_conf and Raft::post_conf_change for many led groups in one launch, the work items into the CALLER's memory.
// The unit keeps no state of its own and touches none of the engine's send-stage bookkeeping.
// There is NO CPU fallback anywhere in this file: without a HIP device every entry point fails.
#include "rg_engine.h"
#pragma GCC visibility push(default) // (the build hides everything else: the exports are the header's declarations, as in rg_engine.h)
#include "../../include/raftgroups_conf.h"
#pragma GCC visibility pop
#include "rg_kernels_conf.h"

extern "C" uint32_t rgc_conf_version(void) { return RGC_CONF_VERSION; }

// What both forms need of the engine, all of it decided on the host; 0 = fine. (Groups that still carry RG_OUT_HOST_HINT are refused
// where every next step refuses them: RG_ENTER_STEP, in front of anything this unit stages or launches.)
static int rgc_conf_state(rg_engine *h, uint32_t flags, bool items, const char *who) {
    if (flags & ~(RG_SEND_SKIP_BCAST_COMMIT | RG_SEND_BYTES)) return rg_fail(RG_ERR_INVALID_ARG, "%s: unknown flags %#x", who, flags);
    if (items && !h->ins_arena)
        return rg_fail(RG_ERR_INVALID_ARG, "%s: the engine holds no device Inflights (max_inflight = 0): it produces no work items, the host sends from the events", who);
    if (h->host_mirror)
        return rg_fail(RG_ERR_STATE, "%s: the engine has a host mirror, whose peer-id tables map ids to slots; rg_set_config is its road", who);
    if ((flags & RG_SEND_BYTES) && !h->esz) return rg_fail(RG_ERR_STATE, "%s: RG_SEND_BYTES needs the entry sizes (rg_log_sizes_enable)", who);
    if (h->ins_arena && h->send_ready)
        return rg_fail(RG_ERR_STATE, "%s: the last tick's send stage is still owed (rg_send_appends): its result words describe windows this call would add to", who);
    if (h->ingested_upper) return rg_fail(RG_ERR_STATE, "%s: records are ingested and not ticked yet (rg_ingest): tick them first", who);
    return RG_OK;
}

// ... and what a launched call leaves behind
static void rgc_conf_applied(rg_engine *h) {
    if (h->pub) h->pub->local_lost = true; // RG_COL_COMMIT was written outside a tick: the published advances no longer describe it
    h->host_res_valid = false;
}

// One launch of kernel<P, IX, GC> for the engine's slot count, index width and group commit over `blocks` blocks of 256 threads
#define RGC_LAUNCH(h, kernel, blocks, ...)                                                                                  \
    rg_with_p((h)->P, [&](auto p) {                                                                                         \
        constexpr int P_ = decltype(p)::value;                                                                              \
        const bool ix32 = rg_ix32((h)->st, (h)->P), gc = (h)->any_group_commit;                                             \
        if (ix32 && !gc) hipLaunchKernelGGL((kernel<P_, u32, false>), dim3(blocks), dim3(256), 0, (h)->stream, __VA_ARGS__); \
        else if (ix32) hipLaunchKernelGGL((kernel<P_, u32, true>), dim3(blocks), dim3(256), 0, (h)->stream, __VA_ARGS__);    \
        else if (!gc) hipLaunchKernelGGL((kernel<P_, u64, false>), dim3(blocks), dim3(256), 0, (h)->stream, __VA_ARGS__);    \
        else hipLaunchKernelGGL((kernel<P_, u64, true>), dim3(blocks), dim3(256), 0, (h)->stream, __VA_ARGS__);              \
    })

extern "C" int rgc_apply_conf(rg_engine *h, const rgc_conf_rec *host_recs, uint64_t n, rgc_conf_resp *host_resp, uint64_t max_entries_per_msg, uint32_t flags,
                              rg_send_item *host_items, uint64_t item_cap, uint64_t *n_items) try {
    if (!h || (n && (!host_recs || !host_resp)) || (item_cap && !host_items)) return rg_fail(RG_ERR_INVALID_ARG, "rgc_apply_conf: bad argument");
    if (int src = rgc_conf_state(h, flags, host_items || item_cap || n_items, "rgc_apply_conf")) return src;
    if (h->ins_arena && !n_items) return rg_fail(RG_ERR_INVALID_ARG, "rgc_apply_conf: n_items is NULL on an engine with device Inflights");
    RgSeen seen;
    for (u64 i = 0; i < n; i++) {
        const rgc_conf_rec &q = host_recs[i];
        if (q.group >= h->G) return rg_fail(RG_ERR_INVALID_ARG, "rgc_apply_conf: record %llu: group %llu of %llu", (unsigned long long)i, (unsigned long long)q.group, (unsigned long long)h->G);
        if (q.reserved) return rg_fail(RG_ERR_INVALID_ARG, "rgc_apply_conf: record %llu: reserved is %u", (unsigned long long)i, q.reserved);
        if (const int rule = rg_conf_word_check(q.cfg, h->P))
            return rg_fail(RG_ERR_INVALID_ARG, "rgc_apply_conf: record %llu: cfg word %#x is malformed (rule %d: a bit outside the three fields, a slot >= %u, no voter, a voter without a Progress)",
                           (unsigned long long)i, q.cfg, rule, h->P);
        if (int rc = rg_named_once("rgc_apply_conf", seen.emplace(q.group, i), i)) return rc;
    }
    if (n_items) *n_items = 0;
    RG_ENTER_STEP(h, "rgc_apply_conf");
    if (n == 0) return RG_OK;
    // staged: recs | resp | count -- and behind them, never uploaded, room for the items the caller can take
    const u64 dev_cap = h->ins_arena ? (item_cap < n * h->P ? item_cap : n * h->P) : 0;
    RgLayout lay;
    lay.add(n * sizeof(rgc_conf_rec));
    const size_t off_resp = lay.add(n * sizeof(rgc_conf_resp)), off_count = lay.add(8), staged = lay.total, off_items = lay.add(dev_cap * sizeof(rg_send_item));
    if (int rc = rg_stage_reserve(h, lay.total)) return rc;
    std::vector<char> stage(staged, 0);
    memcpy(stage.data(), host_recs, n * sizeof(rgc_conf_rec));
    u32 count = 0;
    const RgLeadCols lc = h->ld ? h->ld->cols : RgLeadCols{};
    int rc = rg_follow_round_trip(h, "rgc_apply_conf", stage.data(), staged, [&](char *d) {
        const RgConfItems o = {reinterpret_cast<rg_send_item *>(d + off_items), dev_cap, reinterpret_cast<u32 *>(d + off_count)};
        RGC_LAUNCH(h, k_conf_list, rg_grid(n, 256), h->st, h->ins, lc, reinterpret_cast<const rgc_conf_rec *>(d), (u64)n, reinterpret_cast<rgc_conf_resp *>(d + off_resp),
                   (u64)max_entries_per_msg, (u32)flags, o);
    }, {{host_resp, off_resp, n * sizeof(rgc_conf_resp)}, {&count, off_count, 4}});
    if (rc) return rc;
    rgc_conf_applied(h);
    for (u64 i = 0; i < n; i++) { // rg_set_config's rule, per word that changed
        if (host_resp[i].status != RGC_CONF_DONE && host_resp[i].status != RGC_CONF_DEMOTED) continue;
        const u64 g = host_recs[i].group;
        if (h->host_cfg_valid) h->host_cfg[g] = host_resp[i].cfg;
        if (!h->cls_stale && h->cls_on && rg_cfg_slots_named(host_resp[i].cfg) > h->cls_host[g / RG_BLOCK]) h->cls_stale = true;
    }
    if (n_items) *n_items = count;
    if (const u64 k = count < dev_cap ? count : dev_cap) { // (the staging is still this call's: nothing ran since the round trip)
        RG_HIP(hipMemcpyAsync(host_items, static_cast<char *>(h->d_recs) + off_items, k * sizeof(rg_send_item), hipMemcpyDeviceToHost, h->stream));
        RG_HIP(hipStreamSynchronize(h->stream));
    }
    return RG_OK;
} RG_ABI_GUARD

extern "C" int rgc_apply_conf_device(rg_engine *h, const uint8_t *dev_sel, const uint32_t *dev_cfg, uint64_t max_entries_per_msg, uint32_t flags,
                                     const rgc_conf_out *dev_out) try {
    if (!h || !dev_sel || !dev_cfg || !dev_out || !dev_out->status) return rg_fail(RG_ERR_INVALID_ARG, "rgc_apply_conf_device: bad argument");
    if (dev_out->item_cap && !dev_out->items) return rg_fail(RG_ERR_INVALID_ARG, "rgc_apply_conf_device: the item list is NULL");
    if (int src = rgc_conf_state(h, flags, dev_out->items || dev_out->item_cap || dev_out->count, "rgc_apply_conf_device")) return src;
    if (h->ins_arena && !dev_out->count) return rg_fail(RG_ERR_INVALID_ARG, "rgc_apply_conf_device: the count word is NULL on an engine with device Inflights");
    RG_ENTER_STEP(h, "rgc_apply_conf_device");
    const RgConfItems o = {dev_out->items, dev_out->item_cap, dev_out->count};
    const RgLeadCols lc = h->ld ? h->ld->cols : RgLeadCols{};
    if (dev_out->count) RG_HIP(hipMemsetAsync(dev_out->count, 0, 4, h->stream));
    RGC_LAUNCH(h, k_conf_dense, rg_grid(h->G, 256), h->st, h->ins, lc, dev_sel, (const u32 *)dev_cfg, dev_out->status, dev_out->events, (u64 *)dev_out->commit,
               (u64)max_entries_per_msg, (u32)flags, o);
    if (int rc = rg_launch_check("rgc_apply_conf_device")) return rc;
    rgc_conf_applied(h);
    h->host_cfg_valid = false; // the host has not seen the words
    h->cls_stale = true;       // ... and the next dense tick derives the classes again
    return RG_OK;
} RG_ABI_GUARD
