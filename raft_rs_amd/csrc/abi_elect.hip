// abi_elect.hip -- the candidate half on the follower arena: campaign, vote responses and poll on the device
// (include/raftgroups.h: "The candidate half"). The election cells live in RgFollowEngine; abi_follow.hip frees, checkpoints and
// restores them with the rest of the arena.
// There is NO CPU fallback anywhere in this file: without a HIP device every entry point fails.
#include "rg_engine.h"
#include "rg_kernels_elect.h"

extern "C" int rg_follow_elect_enable(rg_engine *h) try {
    if (!h) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_elect_enable: null engine");
    if (!h->fo || !h->fo->soft_arena) return rg_fail(RG_ERR_STATE, "rg_follow_elect_enable: rg_follow_gate_enable first");
    RgFollowEngine *fo = h->fo;
    if (fo->elect_arena) return rg_fail(RG_ERR_STATE, "rg_follow_elect_enable: already enabled");
    RG_ENTER(h);
    const u64 F = fo->cols.stride;
    const size_t bytes = (size_t)F * 14; // self_id | conf | votes: all zero = no id, no voters, no votes
    char *a = nullptr;
    hipError_t e = hipMalloc(&a, bytes);
    if (e == hipSuccess) e = hipMemsetAsync(a, 0, bytes, h->stream);
    if (e != hipSuccess) {
        if (a) (void)hipFree(a);
        return rg_fail(e == hipErrorOutOfMemory ? RG_ERR_OUT_OF_MEMORY : RG_ERR_NO_DEVICE, "rg_follow_elect_enable: %s", hipGetErrorString(e));
    }
    fo->elect.self_id = reinterpret_cast<u64 *>(a);
    fo->elect.conf = reinterpret_cast<u32 *>(fo->elect.self_id + F);
    fo->elect.votes = reinterpret_cast<unsigned short *>(fo->elect.conf + F);
    fo->elect_arena = a;
    fo->elect_bytes = bytes;
    h->dev.engine_bytes += bytes;
    return RG_OK;
} RG_ABI_GUARD

extern "C" int rg_follow_elect_write(rg_engine *h, const rg_follow_elect *host, uint64_t n) try {
    if (!h || (!host && n)) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_elect_write: bad argument");
    if (!h->fo || !h->fo->elect_arena) return rg_fail(RG_ERR_STATE, "rg_follow_elect_write: rg_follow_elect_enable first");
    RgFollowEngine *fo = h->fo;
    std::unordered_map<u64, u64> seen;
    for (u64 i = 0; i < n; i++) {
        const rg_follow_elect &w = host[i];
        if (w.group >= fo->cols.n)
            return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_elect_write: record %llu: group %llu of %llu", (unsigned long long)i, (unsigned long long)w.group,
                           (unsigned long long)fo->cols.n);
        const int rule = rg_follow_elect_check(w);
        if (rule)
            return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_elect_write: record %llu (group %llu) breaks rule %d of rg_follow_elect_check", (unsigned long long)i,
                           (unsigned long long)w.group, rule);
        if (!seen.emplace(w.group, i).second)
            return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_elect_write: records %llu and %llu name group %llu", (unsigned long long)seen[w.group],
                           (unsigned long long)i, (unsigned long long)w.group);
    }
    if (n == 0) return RG_OK;
    RG_ENTER(h);
    int rc = rg_stage_records(h, host, n * sizeof(rg_follow_elect));
    if (rc) return rc;
    hipLaunchKernelGGL(k_elect_write, dim3(rg_grid(n, 256)), dim3(256), 0, h->stream, fo->elect, reinterpret_cast<const rg_follow_elect *>(h->d_recs), n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rg_fail(RG_ERR_NO_DEVICE, "rg_follow_elect_write: launch failed: %s", hipGetErrorString(e));
    RG_HIP(hipStreamSynchronize(h->stream)); // control path: the staging is reused by the next call
    return RG_OK;
} RG_ABI_GUARD

extern "C" int rg_follow_elect_read(rg_engine *h, const uint64_t *host_groups, uint64_t n, rg_follow_elect *host_out) try {
    if (!h || (n && (!host_groups || !host_out))) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_elect_read: bad argument");
    if (!h->fo || !h->fo->elect_arena) return rg_fail(RG_ERR_STATE, "rg_follow_elect_read: rg_follow_elect_enable first");
    RgFollowEngine *fo = h->fo;
    for (u64 i = 0; i < n; i++)
        if (host_groups[i] >= fo->cols.n)
            return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_elect_read: group %llu of %llu", (unsigned long long)host_groups[i], (unsigned long long)fo->cols.n);
    if (n == 0) return RG_OK;
    RG_ENTER(h);
    const size_t off_out = rg_align(n * 8);
    fo->stage.assign(off_out + n * sizeof(rg_follow_elect), 0);
    memcpy(fo->stage.data(), host_groups, n * 8);
    int rc = rg_stage_records(h, fo->stage.data(), fo->stage.size());
    if (rc) return rc;
    char *d = static_cast<char *>(h->d_recs);
    hipLaunchKernelGGL(k_elect_read, dim3(rg_grid(n, 256)), dim3(256), 0, h->stream, fo->elect, fo->soft.role, reinterpret_cast<const u64 *>(d), n,
                       reinterpret_cast<rg_follow_elect *>(d + off_out));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rg_fail(RG_ERR_NO_DEVICE, "rg_follow_elect_read: launch failed: %s", hipGetErrorString(e));
    RG_HIP(hipMemcpyAsync(host_out, d + off_out, n * sizeof(rg_follow_elect), hipMemcpyDeviceToHost, h->stream));
    RG_HIP(hipStreamSynchronize(h->stream));
    return RG_OK;
} RG_ABI_GUARD

static bool rg_elect_out_complete(const rg_follow_elect_out &o) {
    return o.result && o.events && o.status && o.req_kind && o.targets && o.flags && o.term && o.req_term && o.req_index && o.req_log_term && o.req_commit &&
           o.req_commit_term;
}

extern "C" int rg_follow_campaign_device(rg_engine *h, const uint64_t *dev_groups, const uint64_t *dev_n, uint64_t cap, const uint8_t *dev_block,
                                         const rg_follow_elect_out *dev_out) try {
    if (!h || !dev_n || !dev_out || (cap && !dev_groups)) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_campaign_device: bad argument");
    if (!h->fo || !h->fo->elect_arena) return rg_fail(RG_ERR_STATE, "rg_follow_campaign_device: rg_follow_elect_enable first");
    if (!rg_elect_out_complete(*dev_out)) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_campaign_device: an output column is NULL");
    if (cap > (1ULL << 32)) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_campaign_device: cap %llu, at most 2^32", (unsigned long long)cap);
    if (cap == 0) return RG_OK;
    RG_ENTER(h);
    RgFollowEngine *fo = h->fo;
    hipLaunchKernelGGL(k_elect_campaign, dim3(rg_grid(cap, 256)), dim3(256), 0, h->stream, fo->cols, fo->soft, fo->elect, dev_groups, dev_n, cap, dev_block,
                       *dev_out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rg_fail(RG_ERR_NO_DEVICE, "rg_follow_campaign_device: launch failed: %s", hipGetErrorString(e));
    return RG_OK;
} RG_ABI_GUARD

// The sparse road of both record calls: fo->elect_recs (n records, any order) sorted by group -- stable, so a group's records
// keep their array order --, cut into runs, staged, applied, answered at the records' original positions.
static int rg_elect_run_list(rg_engine *h, const char *who, u64 n, rg_follow_elect_resp *host_resp) {
    RgFollowEngine *fo = h->fo;
    const std::vector<RgElectStaged> &in = fo->elect_recs;
    std::vector<u32> &order = fo->order;
    order.resize(n);
    for (u64 i = 0; i < n; i++) order[i] = (u32)i;
    std::stable_sort(order.begin(), order.end(), [&](u32 a, u32 b) { return in[a].group < in[b].group; });
    u64 runs = 0;
    for (u64 i = 0; i < n; i++) runs += i == 0 || in[order[i]].group != in[order[i - 1]].group;
    const size_t off_orig = rg_align(n * sizeof(RgElectStaged)), off_runs = off_orig + rg_align(n * 4), off_resp = off_runs + rg_align((runs + 1) * 4);
    fo->stage.assign(off_resp + n * sizeof(rg_follow_elect_resp), 0);
    RgElectStaged *recs = reinterpret_cast<RgElectStaged *>(fo->stage.data());
    u32 *orig = reinterpret_cast<u32 *>(fo->stage.data() + off_orig), *rs = reinterpret_cast<u32 *>(fo->stage.data() + off_runs);
    u64 r = 0;
    for (u64 i = 0; i < n; i++) {
        recs[i] = in[order[i]];
        orig[i] = order[i];
        if (i == 0 || recs[i].group != recs[i - 1].group) rs[r++] = (u32)i;
    }
    rs[r] = (u32)n;
    int rc = rg_stage_records(h, fo->stage.data(), fo->stage.size());
    if (rc) return rc;
    char *d = static_cast<char *>(h->d_recs);
    hipLaunchKernelGGL(k_elect_list, dim3(rg_grid(runs, 256)), dim3(256), 0, h->stream, fo->cols, fo->soft, fo->elect, reinterpret_cast<const RgElectStaged *>(d),
                       reinterpret_cast<const u32 *>(d + off_orig), reinterpret_cast<const u32 *>(d + off_runs), (u32)runs,
                       reinterpret_cast<rg_follow_elect_resp *>(d + off_resp));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rg_fail(RG_ERR_NO_DEVICE, "%s: launch failed: %s", who, hipGetErrorString(e));
    RG_HIP(hipMemcpyAsync(host_resp, d + off_resp, n * sizeof(rg_follow_elect_resp), hipMemcpyDeviceToHost, h->stream));
    RG_HIP(hipStreamSynchronize(h->stream)); // control path: the staging is reused by the next call
    return RG_OK;
}

extern "C" int rg_follow_campaign(rg_engine *h, const rg_follow_campaign_req *host_reqs, uint64_t n, rg_follow_elect_resp *host_resp) try {
    if (!h || (n && (!host_reqs || !host_resp))) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_campaign: bad argument");
    if (!h->fo || !h->fo->elect_arena) return rg_fail(RG_ERR_STATE, "rg_follow_campaign: rg_follow_elect_enable first");
    if (n >= 0xffffffffULL) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_campaign: %llu records in one call", (unsigned long long)n);
    RgFollowEngine *fo = h->fo;
    std::unordered_map<u64, u64> seen;
    for (u64 i = 0; i < n; i++) {
        const rg_follow_campaign_req &q = host_reqs[i];
        if (q.group >= fo->cols.n || !rg_elect_campaign_well_formed(q.flags, q.term, q.from))
            return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_campaign: record %llu: group %llu of %llu, flags %#x, term %llu, from %llu", (unsigned long long)i,
                           (unsigned long long)q.group, (unsigned long long)fo->cols.n, q.flags, (unsigned long long)q.term, (unsigned long long)q.from);
        if (!seen.emplace(q.group, i).second)
            return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_campaign: records %llu and %llu name group %llu", (unsigned long long)seen[q.group],
                           (unsigned long long)i, (unsigned long long)q.group);
    }
    if (n == 0) return RG_OK;
    RG_ENTER(h);
    fo->elect_recs.resize(n);
    for (u64 i = 0; i < n; i++) {
        const rg_follow_campaign_req &q = host_reqs[i];
        RgElectStaged &s = fo->elect_recs[i];
        const bool tn = (q.flags & RG_CAMPAIGN_TIMEOUT_NOW) != 0;
        s.group = q.group;
        s.r.term = tn ? q.term : 0;
        s.r.from = tn ? q.from : 0;
        s.r.commit = s.r.commit_term = 0;
        s.r.kind = tn ? RG_ELECT_K_TIMEOUT_NOW : RG_ELECT_K_HUP;
        s.r.flags = (q.flags & RG_CAMPAIGN_BLOCKED) ? RG_ELECT_F_BLOCKED : 0u;
    }
    return rg_elect_run_list(h, "rg_follow_campaign", n, host_resp);
} RG_ABI_GUARD

extern "C" int rg_follow_vote_resps(rg_engine *h, const rg_follow_vote_rec *host_recs, uint64_t n, rg_follow_elect_resp *host_resp) try {
    if (!h || (n && (!host_recs || !host_resp))) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_vote_resps: bad argument");
    if (!h->fo || !h->fo->elect_arena) return rg_fail(RG_ERR_STATE, "rg_follow_vote_resps: rg_follow_elect_enable first");
    if (n >= 0xffffffffULL) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_vote_resps: %llu records in one call", (unsigned long long)n);
    RgFollowEngine *fo = h->fo;
    for (u64 i = 0; i < n; i++) {
        const rg_follow_vote_rec &q = host_recs[i];
        if (q.group >= fo->cols.n || !rg_elect_resp_well_formed(q.kind, q.term, q.from_slot))
            return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_vote_resps: record %llu: group %llu of %llu, kind %#x, term %llu, slot %u", (unsigned long long)i,
                           (unsigned long long)q.group, (unsigned long long)fo->cols.n, (unsigned)q.kind, (unsigned long long)q.term, (unsigned)q.from_slot);
    }
    if (n == 0) return RG_OK;
    RG_ENTER(h);
    fo->elect_recs.resize(n);
    for (u64 i = 0; i < n; i++) {
        const rg_follow_vote_rec &q = host_recs[i];
        RgElectStaged &s = fo->elect_recs[i];
        s.group = q.group;
        s.r.term = q.term;
        s.r.from = q.from_slot;
        s.r.commit = q.commit;
        s.r.commit_term = q.commit_term;
        s.r.kind = q.kind;
        s.r.flags = q.reject ? RG_ELECT_F_REJECT : 0u;
    }
    return rg_elect_run_list(h, "rg_follow_vote_resps", n, host_resp);
} RG_ABI_GUARD

extern "C" int rg_follow_vote_resps_device(rg_engine *h, const rg_follow_vote_cols *dev_msgs, const rg_follow_elect_out *dev_out) try {
    if (!h || !dev_msgs || !dev_out) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_vote_resps_device: bad argument");
    if (!h->fo || !h->fo->elect_arena) return rg_fail(RG_ERR_STATE, "rg_follow_vote_resps_device: rg_follow_elect_enable first");
    const rg_follow_vote_cols &m = *dev_msgs;
    if (!m.kind || !m.slot || !m.reject || !m.term || !m.commit || !m.commit_term)
        return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_vote_resps_device: a message column is NULL");
    if (!rg_elect_out_complete(*dev_out)) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_vote_resps_device: an output column is NULL");
    RG_ENTER(h);
    RgFollowEngine *fo = h->fo;
    hipLaunchKernelGGL(k_elect_dense, dim3(rg_grid(fo->cols.n, 256)), dim3(256), 0, h->stream, fo->cols, fo->soft, fo->elect, m, *dev_out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rg_fail(RG_ERR_NO_DEVICE, "rg_follow_vote_resps_device: launch failed: %s", hipGetErrorString(e));
    return RG_OK;
} RG_ABI_GUARD
