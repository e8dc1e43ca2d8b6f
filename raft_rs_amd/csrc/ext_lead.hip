// ext_lead.hip -- the leader's clock (include/raftgroups_lead.h, the extension header: its entry points are rgx_*): Raft::tick of every led group in one launch,
// check-quorum step-down included, and the way back into the follower arena for a group that stepped down.
// There is NO CPU fallback anywhere in this file: without a HIP device every entry point fails.
#include "rg_engine.h"
#include "rg_handoff_host.h"
#include "rg_kernels_lead.h"

extern "C" int rgx_lead_clock_enable(rg_engine *h, const rg_lead_clock_config *cfg) try {
    if (!h || !cfg) return rg_fail(RG_ERR_INVALID_ARG, "rgx_lead_clock_enable: bad argument");
    if (h->ld) return rg_fail(RG_ERR_STATE, "rgx_lead_clock_enable: already enabled (election_tick %u)", h->ld->cols.cfg.election_tick);
    if (const int rule = rg_lead_config_check(cfg->election_tick, cfg->heartbeat_tick, cfg->flags, cfg->reserved))
        return rg_fail(RG_ERR_INVALID_ARG, "rgx_lead_clock_enable: election_tick %u, heartbeat_tick %u, flags %#x, reserved %u break rule %d of rg_lead_config_check",
                       cfg->election_tick, cfg->heartbeat_tick, cfg->flags, cfg->reserved, rule);
    RG_ENTER(h);
    std::unique_ptr<RgLeadEngine> ld(new RgLeadEngine());
    // tag | cell, then the four count words
    ld->bytes = (size_t)h->stride * 12;
    const size_t total = ld->bytes + 32;
    hipError_t e = hipMalloc(&ld->arena, total);
    if (e == hipSuccess) e = hipMemsetAsync(ld->arena, 0, total, h->stream);
    if (e == hipSuccess) {
        ld->cols.tag = reinterpret_cast<u64 *>(ld->arena);
        ld->cols.cell = reinterpret_cast<u32 *>(ld->cols.tag + h->stride);
        ld->cols.cfg.election_tick = cfg->election_tick;
        ld->cols.cfg.heartbeat_tick = cfg->heartbeat_tick;
        ld->cols.cfg.flags = cfg->flags & RG_GATE_CHECK_QUORUM;
        ld->counts = reinterpret_cast<unsigned long long *>(ld->arena + ld->bytes);
        hipLaunchKernelGGL(k_lead_init, dim3(rg_grid(h->stride, 256)), dim3(256), 0, h->stream, ld->cols, (const u64 *)h->st.cur_term, h->G, h->stride,
                           (cfg->flags & RG_LEAD_CLOCK_START_LED) ? 1u : 0u);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        if (ld->arena) (void)hipFree(ld->arena);
        return rg_fail(e == hipErrorOutOfMemory ? RG_ERR_OUT_OF_MEMORY : RG_ERR_NO_DEVICE, "rgx_lead_clock_enable: %s", hipGetErrorString(e));
    }
    h->ld = ld.release();
    h->dev.engine_bytes += total;
    return RG_OK;
} RG_ABI_GUARD

extern "C" uint32_t rgx_lead_version(void) { return RGX_LEAD_VERSION; }

extern "C" const uint64_t *rgx_lead_clock_counts(const rg_engine *h) {
    return h && h->ld ? reinterpret_cast<const uint64_t *>(h->ld->counts) : nullptr;
}

// ---- what the other units call (rg_engine.h) ----
void rg_lead_free(rg_engine *h) {
    if (!h->ld) return;
    if (h->ld->arena) (void)hipFree(h->ld->arena);
    if (h->ld->ckpt) (void)hipFree(h->ld->ckpt);
    delete h->ld;
    h->ld = nullptr;
}

int rg_lead_checkpoint(rg_engine *h) {
    RgLeadEngine *ld = h->ld;
    if (!ld) return RG_OK;
    if (!ld->ckpt) RG_HIP(hipMalloc(&ld->ckpt, ld->bytes));
    RG_HIP(hipMemcpyAsync(ld->ckpt, ld->arena, ld->bytes, hipMemcpyDeviceToDevice, h->stream));
    return RG_OK;
}

int rg_lead_restore(rg_engine *h) {
    RgLeadEngine *ld = h->ld;
    if (!ld || !ld->ckpt) return RG_OK;
    RG_HIP(hipMemcpyAsync(ld->arena, ld->ckpt, ld->bytes, hipMemcpyDeviceToDevice, h->stream));
    return RG_OK;
}

hipError_t rg_lead_place(rg_engine *h, const u64 *d_perm, char *tmp) {
    RgLeadEngine *ld = h->ld;
    hipError_t e = hipMemcpyAsync(tmp, ld->arena, ld->bytes, hipMemcpyDeviceToDevice, h->stream); // (the padding beyond n_groups stays)
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_lead_place, dim3(rg_grid(h->G, 256)), dim3(256), 0, h->stream, ld->cols, reinterpret_cast<u64 *>(tmp),
                       reinterpret_cast<u32 *>(tmp + h->stride * 8), d_perm, h->G);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(ld->arena, tmp, ld->bytes, hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    return e;
}

// ---- the control path ----
extern "C" int rgx_lead_clock_write(rg_engine *h, const rg_lead_clock_cell *host, uint64_t n) try {
    if (!h || (!host && n)) return rg_fail(RG_ERR_INVALID_ARG, "rgx_lead_clock_write: bad argument");
    if (!h->ld) return rg_fail(RG_ERR_STATE, "rgx_lead_clock_write: rgx_lead_clock_enable first");
    RgLeadEngine *ld = h->ld;
    RgSeen seen;
    for (u64 i = 0; i < n; i++) {
        const rg_lead_clock_cell &w = host[i];
        if (w.group >= h->G)
            return rg_fail(RG_ERR_INVALID_ARG, "rgx_lead_clock_write: record %llu: group %llu of %llu", (unsigned long long)i, (unsigned long long)w.group,
                           (unsigned long long)h->G);
        if (const int rule = rg_lead_cell_check(ld->cols.cfg, w))
            return rg_fail(RG_ERR_INVALID_ARG, "rgx_lead_clock_write: record %llu (group %llu) breaks rule %d of rg_lead_cell_check", (unsigned long long)i,
                           (unsigned long long)w.group, rule);
        if (int rc = rg_named_once("rgx_lead_clock_write", seen.emplace(w.group, i), i)) return rc;
    }
    if (n == 0) return RG_OK;
    RG_ENTER(h);
    return rg_follow_round_trip(h, "rgx_lead_clock_write", host, n * sizeof(rg_lead_clock_cell), [&](char *d) {
        hipLaunchKernelGGL(k_lead_clock_write, dim3(rg_grid(n, 256)), dim3(256), 0, h->stream, ld->cols, reinterpret_cast<const rg_lead_clock_cell *>(d), n);
    });
} RG_ABI_GUARD

extern "C" int rgx_lead_clock_read(rg_engine *h, const uint64_t *host_groups, uint64_t n, rg_lead_clock_cell *host_out) try {
    if (!h || (n && (!host_groups || !host_out))) return rg_fail(RG_ERR_INVALID_ARG, "rgx_lead_clock_read: bad argument");
    if (!h->ld) return rg_fail(RG_ERR_STATE, "rgx_lead_clock_read: rgx_lead_clock_enable first");
    RgLeadEngine *ld = h->ld;
    for (u64 i = 0; i < n; i++)
        if (host_groups[i] >= h->G)
            return rg_fail(RG_ERR_INVALID_ARG, "rgx_lead_clock_read: group %llu of %llu", (unsigned long long)host_groups[i], (unsigned long long)h->G);
    if (n == 0) return RG_OK;
    RG_ENTER(h);
    RgLayout lay;
    lay.add(n * 8);
    const size_t off_out = lay.add(n * sizeof(rg_lead_clock_cell));
    ld->stage.assign(lay.total, 0);
    memcpy(ld->stage.data(), host_groups, n * 8);
    return rg_follow_round_trip(h, "rgx_lead_clock_read", ld->stage.data(), ld->stage.size(), [&](char *d) {
        hipLaunchKernelGGL(k_lead_clock_read, dim3(rg_grid(n, 256)), dim3(256), 0, h->stream, ld->cols, reinterpret_cast<const u64 *>(d), n,
                           reinterpret_cast<rg_lead_clock_cell *>(d + off_out));
    }, {{host_out, off_out, n * sizeof(rg_lead_clock_cell)}});
} RG_ABI_GUARD

// ---- one Raft::tick of every led group ----
extern "C" int rgx_lead_clock(rg_engine *h, const rg_lead_clock_out *dev_out, uint64_t *host_counts) try {
    if (!h || !dev_out || !dev_out->events || (dev_out->beat_cap && !dev_out->beat) || (dev_out->down_cap && !dev_out->down))
        return rg_fail(RG_ERR_INVALID_ARG, "rgx_lead_clock: bad argument");
    if (!h->ld) return rg_fail(RG_ERR_STATE, "rgx_lead_clock: rgx_lead_clock_enable first");
    RG_ENTER(h);
    RgLeadEngine *ld = h->ld;
    rg_lead_clock_out out = *dev_out;
    if (!out.beat) out.beat_cap = 0;
    if (!out.down) out.down_cap = 0;
    RG_HIP(hipMemsetAsync(ld->counts, 0, 32, h->stream));
    RG_LAUNCH_IX(h, k_lead_clock, rg_grid(h->G, 256), h->st, ld->cols, h->P, out, ld->counts, rg_read_qterm(h));
    if (int rc = rg_launch_check("rgx_lead_clock")) return rc;
    if (int rc = rg_fetch_counts(h, host_counts, ld->counts, 32)) return rc;
    const bool cfg_written = !host_counts || host_counts[2] || host_counts[3]; // (an asynchronous call cannot know)
    if (cfg_written && h->host_mirror) h->host_cfg_valid = false; // transferee bits may be gone: the mirror re-reads its copy
    return RG_OK;
} RG_ABI_GUARD

// ---- the way back into the arena ----
extern "C" int rgx_follow_step_down(rg_engine *h, const rg_handoff_rec *host_recs, uint64_t n, rg_handoff_resp *host_resp) try {
    if (!h || (n && (!host_recs || !host_resp))) return rg_fail(RG_ERR_INVALID_ARG, "rgx_follow_step_down: bad argument");
    if (int src = rg_elect_enabled(h, "rgx_follow_step_down")) return src;
    if (int crc = rg_walk_pairs(h, "rgx_follow_step_down", host_recs, n, RG_WALK_SIDE_IN_WHO)) return crc;
    if (n == 0) return RG_OK;
    RG_ENTER(h);
    const RgArenaCols c = rg_arena_cols(h);
    return rg_list_round_trip(h, "rgx_follow_step_down", host_recs, n, host_resp, [&](const rg_handoff_rec *d_recs, rg_handoff_resp *d_resp) {
        RG_LAUNCH_IX(h, k_handoff_step_down_list, rg_grid(n, 256), c, d_recs, n, d_resp);
    });
} RG_ABI_GUARD

extern "C" int rgx_follow_step_down_device(rg_engine *h, const uint8_t *dev_events, const uint64_t *dev_lead, const rg_handoff_out *dev_out) try {
    if (!h || !dev_events || !dev_lead || !dev_out) return rg_fail(RG_ERR_INVALID_ARG, "rgx_follow_step_down_device: bad argument");
    if (int src = rg_elect_enabled(h, "rgx_follow_step_down_device")) return src;
    if (h->host_mirror) return rg_fail(RG_ERR_STATE, "rgx_follow_step_down_device: the engine has a host mirror; rgx_follow_step_down");
    if (!rg_handoff_out_complete(*dev_out)) return rg_fail(RG_ERR_INVALID_ARG, "rgx_follow_step_down_device: an output column is NULL");
    RG_ENTER(h);
    RG_LAUNCH_IX(h, k_handoff_step_down_dense, rg_grid(h->fo->cols.n, 256), rg_arena_cols(h), dev_events, dev_lead, *dev_out);
    return rg_launch_check("rgx_follow_step_down_device");
} RG_ABI_GUARD
