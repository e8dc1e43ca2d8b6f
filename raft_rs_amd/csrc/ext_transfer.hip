// ext_transfer.hip -- the batched leader transfer (include/raftgroups_transfer.h, the sixth extension header: its entry points are
// rgm_*): Raft::handle_transfer_leader for many led groups in one launch, the work items into the CALLER's memory. The unit keeps no
// state of its own and touches none of the engine's send-stage bookkeeping.
// There is NO CPU fallback anywhere in this file: without a HIP device every entry point fails.
#include "rg_engine.h"
#pragma GCC visibility push(default) // (the build hides everything else: the exports are the header's declarations, as in rg_engine.h)
#include "../../include/raftgroups_transfer.h"
#pragma GCC visibility pop
#include "rg_kernels_transfer.h"

extern "C" uint32_t rgm_transfer_version(void) { return RGM_TRANSFER_VERSION; }

// What both forms need of the engine, all of it decided on the host; 0 = fine: the rules of the conf change's rgc_conf_state. (Groups
// that still carry RG_OUT_HOST_HINT are refused where every next step refuses them: RG_ENTER_STEP, in front of anything this unit
// stages or launches.)
static int rgm_transfer_state(rg_engine *h, uint32_t flags, bool items, const char *who) {
    if (flags & ~RG_SEND_BYTES) return rg_fail(RG_ERR_INVALID_ARG, "%s: unknown flags %#x", who, flags);
    if (items && !h->ins_arena)
        return rg_fail(RG_ERR_INVALID_ARG, "%s: the engine holds no device Inflights (max_inflight = 0): it produces no work items, the host sends from the events", who);
    if (h->host_mirror) return rg_fail(RG_ERR_STATE, "%s: the engine has a host mirror; rg_set_config is its road", who);
    if ((flags & RG_SEND_BYTES) && !h->esz) return rg_fail(RG_ERR_STATE, "%s: RG_SEND_BYTES needs the entry sizes (rg_log_sizes_enable)", who);
    if (h->ins_arena && h->send_ready)
        return rg_fail(RG_ERR_STATE, "%s: the last tick's send stage is still owed (rg_send_appends): its result words describe windows this call would add to", who);
    if (h->ingested_upper) return rg_fail(RG_ERR_STATE, "%s: records are ingested and not ticked yet (rg_ingest): tick them first", who);
    return RG_OK;
}

// One launch of kernel<P, IX> for the engine's slot count and index width over `blocks` blocks of 256 threads
#define RGM_LAUNCH(h, kernel, blocks, ...)                                                                                  \
    rg_with_p((h)->P, [&](auto p) {                                                                                         \
        constexpr int P_ = decltype(p)::value;                                                                              \
        if (rg_ix32((h)->st, (h)->P)) hipLaunchKernelGGL((kernel<P_, u32>), dim3(blocks), dim3(256), 0, (h)->stream, __VA_ARGS__); \
        else hipLaunchKernelGGL((kernel<P_, u64>), dim3(blocks), dim3(256), 0, (h)->stream, __VA_ARGS__);                    \
    })

extern "C" int rgm_transfer_leader(rg_engine *h, const rgm_transfer_rec *host_recs, uint64_t n, rgm_transfer_resp *host_resp, uint64_t max_entries_per_msg, uint32_t flags,
                                   rg_send_item *host_items, uint64_t item_cap, uint64_t *n_items) try {
    if (!h || (n && (!host_recs || !host_resp)) || (item_cap && !host_items)) return rg_fail(RG_ERR_INVALID_ARG, "rgm_transfer_leader: bad argument");
    if (int src = rgm_transfer_state(h, flags, host_items || item_cap || n_items, "rgm_transfer_leader")) return src;
    if (h->ins_arena && !n_items) return rg_fail(RG_ERR_INVALID_ARG, "rgm_transfer_leader: n_items is NULL on an engine with device Inflights");
    RgSeen seen;
    for (u64 i = 0; i < n; i++) {
        const rgm_transfer_rec &q = host_recs[i];
        if (q.group >= h->G) return rg_fail(RG_ERR_INVALID_ARG, "rgm_transfer_leader: record %llu: group %llu of %llu", (unsigned long long)i, (unsigned long long)q.group, (unsigned long long)h->G);
        if (q.reserved) return rg_fail(RG_ERR_INVALID_ARG, "rgm_transfer_leader: record %llu: reserved is %u", (unsigned long long)i, q.reserved);
        if (q.slot >= h->P) return rg_fail(RG_ERR_INVALID_ARG, "rgm_transfer_leader: record %llu: slot %u of %u", (unsigned long long)i, q.slot, h->P);
        if (int rc = rg_named_once("rgm_transfer_leader", seen.emplace(q.group, i), i)) return rc;
    }
    if (n_items) *n_items = 0;
    RG_ENTER_STEP(h, "rgm_transfer_leader");
    if (n == 0) return RG_OK;
    // staged: recs | resp | count -- and behind them, never uploaded, room for the items the caller can take (one per record at most)
    const u64 dev_cap = h->ins_arena ? (item_cap < n ? item_cap : n) : 0;
    RgLayout lay;
    lay.add(n * sizeof(rgm_transfer_rec));
    const size_t off_resp = lay.add(n * sizeof(rgm_transfer_resp)), off_count = lay.add(8), staged = lay.total, off_items = lay.add(dev_cap * sizeof(rg_send_item));
    if (int rc = rg_stage_reserve(h, lay.total)) return rc;
    std::vector<char> stage(staged, 0);
    memcpy(stage.data(), host_recs, n * sizeof(rgm_transfer_rec));
    u32 count = 0;
    const RgLeadCols lc = h->ld ? h->ld->cols : RgLeadCols{};
    int rc = rg_follow_round_trip(h, "rgm_transfer_leader", stage.data(), staged, [&](char *d) {
        const RgConfItems o = {reinterpret_cast<rg_send_item *>(d + off_items), dev_cap, h->ins_arena ? reinterpret_cast<u32 *>(d + off_count) : nullptr};
        RGM_LAUNCH(h, k_transfer_list, rg_grid(n, 256), h->st, h->ins, lc, reinterpret_cast<const rgm_transfer_rec *>(d), (u64)n, reinterpret_cast<rgm_transfer_resp *>(d + off_resp),
                   (u64)max_entries_per_msg, (u32)flags, o);
    }, {{host_resp, off_resp, n * sizeof(rgm_transfer_resp)}, {&count, off_count, 4}});
    if (rc) return rc;
    if (h->host_cfg_valid) // (a transferee has a Progress: no word names more slots than before, the size classes stand)
        for (u64 i = 0; i < n; i++) h->host_cfg[host_recs[i].group] = host_resp[i].cfg;
    if (n_items) *n_items = count;
    if (const u64 k = count < dev_cap ? count : dev_cap) { // (the staging is still this call's: nothing ran since the round trip)
        RG_HIP(hipMemcpyAsync(host_items, static_cast<char *>(h->d_recs) + off_items, k * sizeof(rg_send_item), hipMemcpyDeviceToHost, h->stream));
        RG_HIP(hipStreamSynchronize(h->stream));
    }
    return RG_OK;
} RG_ABI_GUARD

extern "C" int rgm_transfer_leader_device(rg_engine *h, const uint8_t *dev_to, uint64_t max_entries_per_msg, uint32_t flags, const rgm_transfer_out *dev_out) try {
    if (!h || !dev_to || !dev_out || !dev_out->status) return rg_fail(RG_ERR_INVALID_ARG, "rgm_transfer_leader_device: bad argument");
    if (dev_out->item_cap && !dev_out->items) return rg_fail(RG_ERR_INVALID_ARG, "rgm_transfer_leader_device: the item list is NULL");
    if (int src = rgm_transfer_state(h, flags, dev_out->items || dev_out->item_cap || dev_out->count, "rgm_transfer_leader_device")) return src;
    if (h->ins_arena && !dev_out->count) return rg_fail(RG_ERR_INVALID_ARG, "rgm_transfer_leader_device: the count word is NULL on an engine with device Inflights");
    RG_ENTER_STEP(h, "rgm_transfer_leader_device");
    const RgConfItems o = {dev_out->items, dev_out->item_cap, dev_out->count};
    const RgLeadCols lc = h->ld ? h->ld->cols : RgLeadCols{};
    if (dev_out->count) RG_HIP(hipMemsetAsync(dev_out->count, 0, 4, h->stream));
    RGM_LAUNCH(h, k_transfer_dense, rg_grid(h->G, 256), h->st, h->ins, lc, dev_to, dev_out->status, dev_out->events, (u64)max_entries_per_msg, (u32)flags, o);
    if (int rc = rg_launch_check("rgm_transfer_leader_device")) return rc;
    h->host_cfg_valid = false; // the host has not seen the words
    return RG_OK;
} RG_ABI_GUARD
