// abi_elect.hip -- the candidate half on the follower arena: campaign, vote responses and poll on the device
// (include/raftgroups.h: "The candidate half"). The election cells live in RgFollowEngine; abi_follow.hip frees, checkpoints and
// restores them with the rest of the arena.
// There is NO CPU fallback anywhere in this file: without a HIP device every entry point fails.
#include "rg_engine.h"
#include "rg_kernels_elect.h"

extern "C" int rg_follow_elect_enable(rg_engine *h) try {
    if (!h) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_elect_enable: null engine");
    if (!h->fo || !h->fo->has(RG_FL_SOFT)) return rg_fail(RG_ERR_STATE, "rg_follow_elect_enable: rg_follow_gate_enable first");
    RgFollowEngine *fo = h->fo;
    if (fo->has(RG_FL_ELECT)) return rg_fail(RG_ERR_STATE, "rg_follow_elect_enable: already enabled");
    RG_ENTER(h);
    const u64 F = fo->cols.stride;
    const size_t bytes = (size_t)F * 14; // self_id | conf | votes: all zero = no id, no voters, no votes
    if (int rc = rg_follow_layer_alloc(h, "rg_follow_elect_enable", &fo->layer[RG_FL_ELECT], bytes, bytes)) return rc;
    fo->elect.self_id = reinterpret_cast<u64 *>(fo->layer[RG_FL_ELECT].arena);
    fo->elect.conf = reinterpret_cast<u32 *>(fo->elect.self_id + F);
    fo->elect.votes = reinterpret_cast<unsigned short *>(fo->elect.conf + F);
    h->dev.engine_bytes += bytes;
    return RG_OK;
} RG_ABI_GUARD

extern "C" int rg_follow_elect_write(rg_engine *h, const rg_follow_elect *host, uint64_t n) try {
    if (!h || (!host && n)) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_elect_write: bad argument");
    if (!h->fo || !h->fo->has(RG_FL_ELECT)) return rg_fail(RG_ERR_STATE, "rg_follow_elect_write: rg_follow_elect_enable first");
    RgFollowEngine *fo = h->fo;
    RgSeen seen;
    for (u64 i = 0; i < n; i++) {
        const rg_follow_elect &w = host[i];
        if (w.group >= fo->cols.n)
            return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_elect_write: record %llu: group %llu of %llu", (unsigned long long)i, (unsigned long long)w.group,
                           (unsigned long long)fo->cols.n);
        const int rule = rg_follow_elect_check(w);
        if (rule)
            return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_elect_write: record %llu (group %llu) breaks rule %d of rg_follow_elect_check", (unsigned long long)i,
                           (unsigned long long)w.group, rule);
        if (int rc = rg_named_once("rg_follow_elect_write", seen.emplace(w.group, i), i)) return rc;
    }
    if (n == 0) return RG_OK;
    RG_ENTER(h);
    return rg_follow_round_trip(h, "rg_follow_elect_write", host, n * sizeof(rg_follow_elect), [&](char *d) {
        hipLaunchKernelGGL(k_elect_write, dim3(rg_grid(n, 256)), dim3(256), 0, h->stream, fo->elect, reinterpret_cast<const rg_follow_elect *>(d), n);
    });
} RG_ABI_GUARD

extern "C" int rg_follow_elect_read(rg_engine *h, const uint64_t *host_groups, uint64_t n, rg_follow_elect *host_out) try {
    if (!h || (n && (!host_groups || !host_out))) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_elect_read: bad argument");
    if (!h->fo || !h->fo->has(RG_FL_ELECT)) return rg_fail(RG_ERR_STATE, "rg_follow_elect_read: rg_follow_elect_enable first");
    return rg_follow_gather(h, "rg_follow_elect_read", host_groups, n, host_out, [&](const u64 *d_groups, rg_follow_elect *d_out) {
        hipLaunchKernelGGL(k_elect_read, dim3(rg_grid(n, 256)), dim3(256), 0, h->stream, h->fo->elect, h->fo->soft.role, d_groups, n, d_out);
    });
} RG_ABI_GUARD

static bool rg_elect_out_complete(const rg_follow_elect_out &o) {
    return o.result && o.events && o.status && o.req_kind && o.targets && o.flags && o.term && o.req_term && o.req_index && o.req_log_term && o.req_commit &&
           o.req_commit_term;
}

extern "C" int rg_follow_campaign_device(rg_engine *h, const uint64_t *dev_groups, const uint64_t *dev_n, uint64_t cap, const uint8_t *dev_block,
                                         const rg_follow_elect_out *dev_out) try {
    if (!h || !dev_n || !dev_out || (cap && !dev_groups)) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_campaign_device: bad argument");
    if (!h->fo || !h->fo->has(RG_FL_ELECT)) return rg_fail(RG_ERR_STATE, "rg_follow_campaign_device: rg_follow_elect_enable first");
    if (!rg_elect_out_complete(*dev_out)) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_campaign_device: an output column is NULL");
    if (cap > (1ULL << 32)) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_campaign_device: cap %llu, at most 2^32", (unsigned long long)cap);
    if (cap == 0) return RG_OK;
    RG_ENTER(h);
    RgFollowEngine *fo = h->fo;
    hipLaunchKernelGGL(k_elect_campaign, dim3(rg_grid(cap, 256)), dim3(256), 0, h->stream, fo->cols, fo->soft, fo->elect, dev_groups, dev_n, cap, dev_block,
                       *dev_out);
    return rg_launch_check("rg_follow_campaign_device");
} RG_ABI_GUARD

// The sparse road of both record calls: fo->elect_recs (n records, any order) sorted by group -- stable, so a group's records
// keep their array order --, cut into runs, staged, applied, answered at the records' original positions.
static int rg_elect_run_list(rg_engine *h, const char *who, u64 n, rg_follow_elect_resp *host_resp) {
    RgFollowEngine *fo = h->fo;
    const std::vector<RgElectStaged> &in = fo->elect_recs;
    const auto group_of = [&](u64 i) { return in[i].group; };
    const u64 runs = rg_runs_sort(fo->order, n, group_of);
    RgLayout lay;
    lay.add(n * sizeof(RgElectStaged));
    const size_t off_orig = lay.add(n * 4), off_runs = lay.add((runs + 1) * 4), off_resp = lay.add(n * sizeof(rg_follow_elect_resp));
    fo->stage.assign(lay.total, 0);
    char *s = fo->stage.data();
    rg_runs_cut(fo->order, group_of, reinterpret_cast<u32 *>(s + off_orig), reinterpret_cast<u32 *>(s + off_runs));
    for (u64 i = 0; i < n; i++) reinterpret_cast<RgElectStaged *>(s)[i] = in[fo->order[i]];
    return rg_follow_round_trip(h, who, s, lay.total, [&](char *d) {
        hipLaunchKernelGGL(k_elect_list, dim3(rg_grid(runs, 256)), dim3(256), 0, h->stream, fo->cols, fo->soft, fo->elect, reinterpret_cast<const RgElectStaged *>(d),
                           reinterpret_cast<const u32 *>(d + off_orig), reinterpret_cast<const u32 *>(d + off_runs), (u32)runs,
                           reinterpret_cast<rg_follow_elect_resp *>(d + off_resp));
    }, {{host_resp, off_resp, n * sizeof(rg_follow_elect_resp)}});
}

extern "C" int rg_follow_campaign(rg_engine *h, const rg_follow_campaign_req *host_reqs, uint64_t n, rg_follow_elect_resp *host_resp) try {
    if (!h || (n && (!host_reqs || !host_resp))) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_campaign: bad argument");
    if (!h->fo || !h->fo->has(RG_FL_ELECT)) return rg_fail(RG_ERR_STATE, "rg_follow_campaign: rg_follow_elect_enable first");
    if (n >= 0xffffffffULL) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_campaign: %llu records in one call", (unsigned long long)n);
    RgFollowEngine *fo = h->fo;
    RgSeen seen;
    for (u64 i = 0; i < n; i++) {
        const rg_follow_campaign_req &q = host_reqs[i];
        if (q.group >= fo->cols.n || !rg_elect_campaign_well_formed(q.flags, q.term, q.from))
            return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_campaign: record %llu: group %llu of %llu, flags %#x, term %llu, from %llu", (unsigned long long)i,
                           (unsigned long long)q.group, (unsigned long long)fo->cols.n, q.flags, (unsigned long long)q.term, (unsigned long long)q.from);
        if (int rc = rg_named_once("rg_follow_campaign", seen.emplace(q.group, i), i)) return rc;
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
    if (!h->fo || !h->fo->has(RG_FL_ELECT)) return rg_fail(RG_ERR_STATE, "rg_follow_vote_resps: rg_follow_elect_enable first");
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
    if (!h->fo || !h->fo->has(RG_FL_ELECT)) return rg_fail(RG_ERR_STATE, "rg_follow_vote_resps_device: rg_follow_elect_enable first");
    const rg_follow_vote_cols &m = *dev_msgs;
    if (!m.kind || !m.slot || !m.reject || !m.term || !m.commit || !m.commit_term)
        return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_vote_resps_device: a message column is NULL");
    if (!rg_elect_out_complete(*dev_out)) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_vote_resps_device: an output column is NULL");
    RG_ENTER(h);
    RgFollowEngine *fo = h->fo;
    hipLaunchKernelGGL(k_elect_dense, dim3(rg_grid(fo->cols.n, 256)), dim3(256), 0, h->stream, fo->cols, fo->soft, fo->elect, m, *dev_out);
    return rg_launch_check("rg_follow_vote_resps_device");
} RG_ABI_GUARD
