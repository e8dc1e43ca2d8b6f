// abi_follow.hip -- the follower half: MsgAppend / MsgHeartbeat steps on the device (include/raftgroups.h: "The follower half"),
// and behind rg_follow_gate_enable the term gate of Raft::step, the vote step and the election clock ("The follower's term gate ...")
// There is NO CPU fallback anywhere in this file: without a HIP device every entry point fails.
#include "rg_engine.h"
#include "rg_kernels_follow.h"

extern "C" int rg_follow_enable(rg_engine *h, uint64_t n_follow) try {
    if (!h) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_enable: null engine");
    if (h->fo) return rg_fail(RG_ERR_STATE, "rg_follow_enable: already enabled (%llu groups)", (unsigned long long)h->fo->cols.n);
    if (n_follow < 1 || n_follow > (1ULL << 32)) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_enable: %llu groups, 1..2^32", (unsigned long long)n_follow);
    RG_ENTER(h);
    RgFollowEngine *fo = new RgFollowEngine();
    fo->arena = fo->ckpt = fo->soft_arena = fo->soft_ckpt = nullptr;
    fo->soft_bytes = 0;
    fo->clock_counts = nullptr;
    const u64 F = (n_follow + 255) & ~255ULL;
    // committed | last | tail_first | tail_term | dummy_idx | dummy_term | run_first[RG_TERM_RUNS] | run_term[RG_TERM_RUNS] | n_old
    const size_t col = (size_t)F * 8;
    fo->bytes = col * (6 + 2 * RG_TERM_RUNS) + (size_t)F;
    hipError_t e = hipMalloc(&fo->arena, fo->bytes);
    if (e == hipSuccess) e = hipMemsetAsync(fo->arena, 0, fo->bytes, h->stream);
    if (e != hipSuccess) {
        if (fo->arena) (void)hipFree(fo->arena);
        delete fo;
        return rg_fail(e == hipErrorOutOfMemory ? RG_ERR_OUT_OF_MEMORY : RG_ERR_NO_DEVICE, "rg_follow_enable: %s", hipGetErrorString(e));
    }
    u64 *a = reinterpret_cast<u64 *>(fo->arena);
    fo->cols.committed = a;
    fo->cols.last = a + F;
    fo->cols.tail_first = a + 2 * F;
    fo->cols.tail_term = a + 3 * F;
    fo->cols.dummy_idx = a + 4 * F;
    fo->cols.dummy_term = a + 5 * F;
    fo->cols.run_first = a + 6 * F;
    fo->cols.run_term = a + (6 + RG_TERM_RUNS) * F;
    fo->cols.n_old = reinterpret_cast<u8 *>(a + (6 + 2 * RG_TERM_RUNS) * F);
    fo->cols.stride = F;
    fo->cols.n = n_follow;
    hipLaunchKernelGGL(k_follow_init, dim3(rg_grid(F, 256)), dim3(256), 0, h->stream, fo->cols);
    e = hipGetLastError();
    if (e != hipSuccess) {
        (void)hipFree(fo->arena);
        delete fo;
        return rg_fail(RG_ERR_NO_DEVICE, "rg_follow_enable: launch failed: %s", hipGetErrorString(e));
    }
    h->fo = fo;
    h->dev.engine_bytes += fo->bytes;
    return RG_OK;
} RG_ABI_GUARD

extern "C" uint64_t rg_follow_stride(const rg_engine *h) { return h && h->fo ? h->fo->cols.stride : 0; }

// ---- what the other units call (rg_engine.h) ----
void rg_follow_free(rg_engine *h) {
    RgFollowEngine *fo = h->fo;
    if (!fo) return;
    if (fo->arena) (void)hipFree(fo->arena);
    if (fo->ckpt) (void)hipFree(fo->ckpt);
    if (fo->soft_arena) (void)hipFree(fo->soft_arena);
    if (fo->soft_ckpt) (void)hipFree(fo->soft_ckpt);
    if (fo->elect_arena) (void)hipFree(fo->elect_arena);
    if (fo->elect_ckpt) (void)hipFree(fo->elect_ckpt);
    delete fo;
    h->fo = nullptr;
}

int rg_follow_checkpoint(rg_engine *h) {
    RgFollowEngine *fo = h->fo;
    if (!fo) return RG_OK;
    if (!fo->ckpt) RG_HIP(hipMalloc(&fo->ckpt, fo->bytes));
    RG_HIP(hipMemcpyAsync(fo->ckpt, fo->arena, fo->bytes, hipMemcpyDeviceToDevice, h->stream));
    if (fo->soft_arena) {
        if (!fo->soft_ckpt) RG_HIP(hipMalloc(&fo->soft_ckpt, fo->soft_bytes));
        RG_HIP(hipMemcpyAsync(fo->soft_ckpt, fo->soft_arena, fo->soft_bytes, hipMemcpyDeviceToDevice, h->stream));
    }
    if (fo->elect_arena) { // (the candidate half, abi_elect.hip)
        if (!fo->elect_ckpt) RG_HIP(hipMalloc(&fo->elect_ckpt, fo->elect_bytes));
        RG_HIP(hipMemcpyAsync(fo->elect_ckpt, fo->elect_arena, fo->elect_bytes, hipMemcpyDeviceToDevice, h->stream));
    }
    return RG_OK;
}

int rg_follow_restore(rg_engine *h) {
    RgFollowEngine *fo = h->fo;
    if (!fo || !fo->ckpt) return RG_OK;
    RG_HIP(hipMemcpyAsync(fo->arena, fo->ckpt, fo->bytes, hipMemcpyDeviceToDevice, h->stream));
    if (fo->soft_ckpt) RG_HIP(hipMemcpyAsync(fo->soft_arena, fo->soft_ckpt, fo->soft_bytes, hipMemcpyDeviceToDevice, h->stream));
    if (fo->elect_ckpt) RG_HIP(hipMemcpyAsync(fo->elect_arena, fo->elect_ckpt, fo->elect_bytes, hipMemcpyDeviceToDevice, h->stream));
    return RG_OK;
}

extern "C" int rg_follow_write(rg_engine *h, const rg_follow_state *host_states, uint64_t n) try {
    if (!h || (!host_states && n)) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_write: bad argument");
    if (!h->fo) return rg_fail(RG_ERR_STATE, "rg_follow_write: rg_follow_enable first");
    RgFollowEngine *fo = h->fo;
    for (u64 i = 0; i < n; i++) {
        const rg_follow_state &s = host_states[i];
        if (s.group >= fo->cols.n)
            return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_write: state %llu: group %llu of %llu", (unsigned long long)i, (unsigned long long)s.group,
                           (unsigned long long)fo->cols.n);
        const int rule = rg_follow_state_check(s);
        if (rule)
            return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_write: state %llu (group %llu) is not canonical (rule %d of rg_follow_state_check)",
                           (unsigned long long)i, (unsigned long long)s.group, rule);
    }
    if (n == 0) return RG_OK;
    RG_ENTER(h);
    // one lane per state: of several states of one group the last one is the group's
    std::unordered_map<u64, u64> last_of;
    for (u64 i = 0; i < n; i++) last_of[host_states[i].group] = i;
    fo->states.clear();
    for (u64 i = 0; i < n; i++)
        if (last_of[host_states[i].group] == i) fo->states.push_back(host_states[i]);
    const u64 k = fo->states.size();
    int rc = rg_stage_records(h, fo->states.data(), k * sizeof(rg_follow_state));
    if (rc) return rc;
    hipLaunchKernelGGL(k_follow_write, dim3(rg_grid(k, 256)), dim3(256), 0, h->stream, fo->cols, reinterpret_cast<const rg_follow_state *>(h->d_recs), k);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rg_fail(RG_ERR_NO_DEVICE, "rg_follow_write: launch failed: %s", hipGetErrorString(e));
    RG_HIP(hipStreamSynchronize(h->stream)); // control path: the staging is reused by the next call
    return RG_OK;
} RG_ABI_GUARD

extern "C" int rg_follow_read(rg_engine *h, const uint64_t *host_groups, uint64_t n, rg_follow_state *host_out) try {
    if (!h || (n && (!host_groups || !host_out))) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_read: bad argument");
    if (!h->fo) return rg_fail(RG_ERR_STATE, "rg_follow_read: rg_follow_enable first");
    RgFollowEngine *fo = h->fo;
    for (u64 i = 0; i < n; i++)
        if (host_groups[i] >= fo->cols.n)
            return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_read: group %llu of %llu", (unsigned long long)host_groups[i], (unsigned long long)fo->cols.n);
    if (n == 0) return RG_OK;
    RG_ENTER(h);
    const size_t off_out = rg_align(n * 8);
    fo->stage.assign(off_out + n * sizeof(rg_follow_state), 0);
    memcpy(fo->stage.data(), host_groups, n * 8);
    int rc = rg_stage_records(h, fo->stage.data(), fo->stage.size());
    if (rc) return rc;
    char *d = static_cast<char *>(h->d_recs);
    hipLaunchKernelGGL(k_follow_read, dim3(rg_grid(n, 256)), dim3(256), 0, h->stream, fo->cols, reinterpret_cast<const u64 *>(d), n,
                       reinterpret_cast<rg_follow_state *>(d + off_out));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rg_fail(RG_ERR_NO_DEVICE, "rg_follow_read: launch failed: %s", hipGetErrorString(e));
    RG_HIP(hipMemcpyAsync(host_out, d + off_out, n * sizeof(rg_follow_state), hipMemcpyDeviceToHost, h->stream));
    RG_HIP(hipStreamSynchronize(h->stream));
    return RG_OK;
} RG_ABI_GUARD

extern "C" int rg_follow_step(rg_engine *h, const rg_follow_msg *host_msgs, uint64_t n, const rg_follow_ent_run *host_ext, uint64_t n_ext,
                              rg_follow_resp *host_resp) try {
    if (!h || (n && (!host_msgs || !host_resp)) || (n_ext && !host_ext)) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_step: bad argument");
    if (!h->fo) return rg_fail(RG_ERR_STATE, "rg_follow_step: rg_follow_enable first");
    if (n >= 0xffffffffULL) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_step: %llu records in one call", (unsigned long long)n);
    RgFollowEngine *fo = h->fo;
    for (u64 i = 0; i < n; i++) {
        const rg_follow_msg &m = host_msgs[i];
        const u64 cnt = m.ext & 0xffu, off = m.ext >> 8;
        if (m.group >= fo->cols.n || (m.flags != RG_FOLLOW_MSG_APPEND && m.flags != RG_FOLLOW_MSG_HEARTBEAT) || (cnt && (off > n_ext || cnt > n_ext - off)))
            return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_step: record %llu: group %llu of %llu, flags %#x, ext %llu + %llu of %llu", (unsigned long long)i,
                           (unsigned long long)m.group, (unsigned long long)fo->cols.n, m.flags, (unsigned long long)off, (unsigned long long)cnt,
                           (unsigned long long)n_ext);
    }
    if (n == 0) return RG_OK;
    RG_ENTER(h);
    // sorted by group -- stable, so a group's records keep their array order --, cut into runs, staged and applied
    std::vector<u32> &order = fo->order;
    order.resize(n);
    for (u64 i = 0; i < n; i++) order[i] = (u32)i;
    std::stable_sort(order.begin(), order.end(), [&](u32 a, u32 b) { return host_msgs[a].group < host_msgs[b].group; });
    u64 runs = 0;
    for (u64 i = 0; i < n; i++) runs += i == 0 || host_msgs[order[i]].group != host_msgs[order[i - 1]].group;
    const size_t off_orig = rg_align(n * sizeof(rg_follow_msg)), off_runs = off_orig + rg_align(n * 4), off_ext = off_runs + rg_align((runs + 1) * 4),
                 off_resp = off_ext + rg_align(n_ext * sizeof(rg_follow_ent_run));
    fo->stage.assign(off_resp + n * sizeof(rg_follow_resp), 0);
    rg_follow_msg *recs = reinterpret_cast<rg_follow_msg *>(fo->stage.data());
    u32 *orig = reinterpret_cast<u32 *>(fo->stage.data() + off_orig), *rs = reinterpret_cast<u32 *>(fo->stage.data() + off_runs);
    u64 r = 0;
    for (u64 i = 0; i < n; i++) {
        recs[i] = host_msgs[order[i]];
        orig[i] = order[i];
        if (i == 0 || recs[i].group != recs[i - 1].group) rs[r++] = (u32)i;
    }
    rs[r] = (u32)n;
    if (n_ext) memcpy(fo->stage.data() + off_ext, host_ext, n_ext * sizeof(rg_follow_ent_run));
    int rc = rg_stage_records(h, fo->stage.data(), fo->stage.size());
    if (rc) return rc;
    char *d = static_cast<char *>(h->d_recs);
    hipLaunchKernelGGL(k_follow_list, dim3(rg_grid(runs, 256)), dim3(256), 0, h->stream, fo->cols, reinterpret_cast<const rg_follow_msg *>(d),
                       reinterpret_cast<const u32 *>(d + off_orig), reinterpret_cast<const u32 *>(d + off_runs), (u32)runs,
                       reinterpret_cast<const rg_follow_ent_run *>(d + off_ext), reinterpret_cast<rg_follow_resp *>(d + off_resp));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rg_fail(RG_ERR_NO_DEVICE, "rg_follow_step: launch failed: %s", hipGetErrorString(e));
    RG_HIP(hipMemcpyAsync(host_resp, d + off_resp, n * sizeof(rg_follow_resp), hipMemcpyDeviceToHost, h->stream));
    RG_HIP(hipStreamSynchronize(h->stream)); // control path: the staging is reused by the next call
    return RG_OK;
} RG_ABI_GUARD

extern "C" int rg_follow_step_device(rg_engine *h, const rg_follow_msgs *dev_msgs, const rg_follow_out *dev_out) try {
    if (!h || !dev_msgs || !dev_out) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_step_device: bad argument");
    if (!h->fo) return rg_fail(RG_ERR_STATE, "rg_follow_step_device: rg_follow_enable first");
    const rg_follow_msgs &m = *dev_msgs;
    const rg_follow_out &o = *dev_out;
    if (!m.flags || !m.index || !m.log_term || !m.commit || !m.ent_term || !m.n_entries)
        return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_step_device: a message column is NULL (only ext / ext_runs may be)");
    if (!o.status || !o.index || !o.commit || !o.conflict || !o.reject_hint || !o.log_term)
        return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_step_device: a response column is NULL");
    RG_ENTER(h);
    RgFollowEngine *fo = h->fo;
    hipLaunchKernelGGL(k_follow_dense, dim3(rg_grid(fo->cols.n, 256)), dim3(256), 0, h->stream, fo->cols, m, o);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rg_fail(RG_ERR_NO_DEVICE, "rg_follow_step_device: launch failed: %s", hipGetErrorString(e));
    return RG_OK;
} RG_ABI_GUARD

// ---- the term gate, the vote step and the election clock ----
extern "C" int rg_follow_gate_enable(rg_engine *h, const rg_follow_gate_config *cfg) try {
    if (!h || !cfg) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_gate_enable: bad argument");
    if (!h->fo) return rg_fail(RG_ERR_STATE, "rg_follow_gate_enable: rg_follow_enable first");
    RgFollowEngine *fo = h->fo;
    if (fo->soft_arena) return rg_fail(RG_ERR_STATE, "rg_follow_gate_enable: already enabled");
    RgGateCfg g;
    g.election_tick = cfg->election_tick;
    g.min_timeout = cfg->min_timeout;
    g.max_timeout = cfg->max_timeout;
    g.flags = cfg->flags;
    g.seed = cfg->seed;
    if (g.election_tick < 1 || g.election_tick > 16383) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_gate_enable: election_tick %u, 1..16383", g.election_tick);
    if (g.min_timeout == 0 && g.max_timeout == 0) {
        g.min_timeout = g.election_tick;
        g.max_timeout = 2 * g.election_tick;
    }
    if (g.min_timeout < g.election_tick || g.min_timeout >= g.max_timeout || g.max_timeout > 32767)
        return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_gate_enable: timeouts [%u, %u): election_tick %u <= min < max <= 32767", g.min_timeout, g.max_timeout,
                       g.election_tick);
    if (g.flags & ~(RG_GATE_CHECK_QUORUM | RG_GATE_PRE_VOTE)) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_gate_enable: flags %#x", g.flags);
    RG_ENTER(h);
    const u64 F = fo->cols.stride;
    // term | lead | vote | priority | clock | role, then the clock's two count words
    const size_t bytes = (size_t)F * 37, total = bytes + 16;
    char *a = nullptr;
    hipError_t e = hipMalloc(&a, total);
    if (e == hipSuccess) e = hipMemsetAsync(a, 0, total, h->stream);
    if (e != hipSuccess) {
        if (a) (void)hipFree(a);
        return rg_fail(e == hipErrorOutOfMemory ? RG_ERR_OUT_OF_MEMORY : RG_ERR_NO_DEVICE, "rg_follow_gate_enable: %s", hipGetErrorString(e));
    }
    RgSoftCols sc;
    sc.term = reinterpret_cast<u64 *>(a);
    sc.lead = sc.term + F;
    sc.vote = sc.term + 2 * F;
    sc.priority = reinterpret_cast<int64_t *>(sc.term + 3 * F);
    sc.clock = reinterpret_cast<u32 *>(sc.term + 4 * F);
    sc.role = reinterpret_cast<u8 *>(sc.clock + F);
    sc.cfg = g;
    hipLaunchKernelGGL(k_follow_soft_init, dim3(rg_grid(F, 256)), dim3(256), 0, h->stream, sc, F);
    e = hipGetLastError();
    if (e != hipSuccess) {
        (void)hipFree(a);
        return rg_fail(RG_ERR_NO_DEVICE, "rg_follow_gate_enable: launch failed: %s", hipGetErrorString(e));
    }
    fo->soft = sc;
    fo->soft_arena = a;
    fo->soft_bytes = bytes;
    fo->clock_counts = reinterpret_cast<unsigned long long *>(a + bytes);
    h->dev.engine_bytes += total;
    return RG_OK;
} RG_ABI_GUARD

extern "C" const uint64_t *rg_follow_clock_counts(const rg_engine *h) {
    return h && h->fo && h->fo->soft_arena ? reinterpret_cast<const uint64_t *>(h->fo->clock_counts) : nullptr;
}

extern "C" int rg_follow_soft_write(rg_engine *h, const rg_follow_soft *host, uint64_t n) try {
    if (!h || (!host && n)) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_soft_write: bad argument");
    if (!h->fo || !h->fo->soft_arena) return rg_fail(RG_ERR_STATE, "rg_follow_soft_write: rg_follow_gate_enable first");
    RgFollowEngine *fo = h->fo;
    std::unordered_map<u64, u64> seen;
    for (u64 i = 0; i < n; i++) {
        const rg_follow_soft &w = host[i];
        if (w.group >= fo->cols.n)
            return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_soft_write: record %llu: group %llu of %llu", (unsigned long long)i, (unsigned long long)w.group,
                           (unsigned long long)fo->cols.n);
        const int rule = rg_follow_soft_check(w, fo->soft.cfg.min_timeout, fo->soft.cfg.max_timeout);
        if (rule)
            return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_soft_write: record %llu (group %llu) breaks rule %d of rg_follow_soft_check", (unsigned long long)i,
                           (unsigned long long)w.group, rule);
        if (!seen.emplace(w.group, i).second)
            return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_soft_write: records %llu and %llu name group %llu", (unsigned long long)seen[w.group],
                           (unsigned long long)i, (unsigned long long)w.group);
    }
    if (n == 0) return RG_OK;
    RG_ENTER(h);
    int rc = rg_stage_records(h, host, n * sizeof(rg_follow_soft));
    if (rc) return rc;
    hipLaunchKernelGGL(k_follow_soft_write, dim3(rg_grid(n, 256)), dim3(256), 0, h->stream, fo->soft, reinterpret_cast<const rg_follow_soft *>(h->d_recs), n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rg_fail(RG_ERR_NO_DEVICE, "rg_follow_soft_write: launch failed: %s", hipGetErrorString(e));
    RG_HIP(hipStreamSynchronize(h->stream)); // control path: the staging is reused by the next call
    return RG_OK;
} RG_ABI_GUARD

extern "C" int rg_follow_soft_read(rg_engine *h, const uint64_t *host_groups, uint64_t n, rg_follow_soft *host_out) try {
    if (!h || (n && (!host_groups || !host_out))) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_soft_read: bad argument");
    if (!h->fo || !h->fo->soft_arena) return rg_fail(RG_ERR_STATE, "rg_follow_soft_read: rg_follow_gate_enable first");
    RgFollowEngine *fo = h->fo;
    for (u64 i = 0; i < n; i++)
        if (host_groups[i] >= fo->cols.n)
            return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_soft_read: group %llu of %llu", (unsigned long long)host_groups[i], (unsigned long long)fo->cols.n);
    if (n == 0) return RG_OK;
    RG_ENTER(h);
    const size_t off_out = rg_align(n * 8);
    fo->stage.assign(off_out + n * sizeof(rg_follow_soft), 0);
    memcpy(fo->stage.data(), host_groups, n * 8);
    int rc = rg_stage_records(h, fo->stage.data(), fo->stage.size());
    if (rc) return rc;
    char *d = static_cast<char *>(h->d_recs);
    hipLaunchKernelGGL(k_follow_soft_read, dim3(rg_grid(n, 256)), dim3(256), 0, h->stream, fo->soft, reinterpret_cast<const u64 *>(d), n,
                       reinterpret_cast<rg_follow_soft *>(d + off_out));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rg_fail(RG_ERR_NO_DEVICE, "rg_follow_soft_read: launch failed: %s", hipGetErrorString(e));
    RG_HIP(hipMemcpyAsync(host_out, d + off_out, n * sizeof(rg_follow_soft), hipMemcpyDeviceToHost, h->stream));
    RG_HIP(hipStreamSynchronize(h->stream));
    return RG_OK;
} RG_ABI_GUARD

extern "C" int rg_follow_step_gated(rg_engine *h, const rg_follow_msg *host_msgs, const rg_follow_hdr *host_hdr, uint64_t n,
                                    const rg_follow_ent_run *host_ext, uint64_t n_ext, rg_follow_resp *host_resp, rg_follow_gate_resp *host_gate) try {
    if (!h || (n && (!host_msgs || !host_hdr || !host_resp || !host_gate)) || (n_ext && !host_ext))
        return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_step_gated: bad argument");
    if (!h->fo || !h->fo->soft_arena) return rg_fail(RG_ERR_STATE, "rg_follow_step_gated: rg_follow_gate_enable first");
    if (n >= 0xffffffffULL) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_step_gated: %llu records in one call", (unsigned long long)n);
    RgFollowEngine *fo = h->fo;
    for (u64 i = 0; i < n; i++) {
        const rg_follow_msg &m = host_msgs[i];
        const u64 cnt = m.ext & 0xffu, off = m.ext >> 8;
        if (m.group >= fo->cols.n || !rg_gate_well_formed(m.flags, host_hdr[i].term, host_hdr[i].from, m.n_entries, (u32)cnt, true) ||
            (cnt && (off > n_ext || cnt > n_ext - off)))
            return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_step_gated: record %llu: group %llu of %llu, flags %#x, term %llu, from %llu, ext %llu + %llu of %llu",
                           (unsigned long long)i, (unsigned long long)m.group, (unsigned long long)fo->cols.n, m.flags, (unsigned long long)host_hdr[i].term,
                           (unsigned long long)host_hdr[i].from, (unsigned long long)off, (unsigned long long)cnt, (unsigned long long)n_ext);
    }
    if (n == 0) return RG_OK;
    RG_ENTER(h);
    // as rg_follow_step: sorted by group (stable), cut into runs, staged and applied
    std::vector<u32> &order = fo->order;
    order.resize(n);
    for (u64 i = 0; i < n; i++) order[i] = (u32)i;
    std::stable_sort(order.begin(), order.end(), [&](u32 a, u32 b) { return host_msgs[a].group < host_msgs[b].group; });
    u64 runs = 0;
    for (u64 i = 0; i < n; i++) runs += i == 0 || host_msgs[order[i]].group != host_msgs[order[i - 1]].group;
    const size_t off_hdr = rg_align(n * sizeof(rg_follow_msg)), off_orig = off_hdr + rg_align(n * sizeof(rg_follow_hdr)), off_runs = off_orig + rg_align(n * 4),
                 off_ext = off_runs + rg_align((runs + 1) * 4), off_resp = off_ext + rg_align(n_ext * sizeof(rg_follow_ent_run)),
                 off_gate = off_resp + rg_align(n * sizeof(rg_follow_resp));
    fo->stage.assign(off_gate + n * sizeof(rg_follow_gate_resp), 0);
    rg_follow_msg *recs = reinterpret_cast<rg_follow_msg *>(fo->stage.data());
    rg_follow_hdr *hdrs = reinterpret_cast<rg_follow_hdr *>(fo->stage.data() + off_hdr);
    u32 *orig = reinterpret_cast<u32 *>(fo->stage.data() + off_orig), *rs = reinterpret_cast<u32 *>(fo->stage.data() + off_runs);
    u64 r = 0;
    for (u64 i = 0; i < n; i++) {
        recs[i] = host_msgs[order[i]];
        hdrs[i] = host_hdr[order[i]];
        orig[i] = order[i];
        if (i == 0 || recs[i].group != recs[i - 1].group) rs[r++] = (u32)i;
    }
    rs[r] = (u32)n;
    if (n_ext) memcpy(fo->stage.data() + off_ext, host_ext, n_ext * sizeof(rg_follow_ent_run));
    int rc = rg_stage_records(h, fo->stage.data(), fo->stage.size());
    if (rc) return rc;
    char *d = static_cast<char *>(h->d_recs);
    hipLaunchKernelGGL(k_follow_gate_list, dim3(rg_grid(runs, 256)), dim3(256), 0, h->stream, fo->cols, fo->soft, reinterpret_cast<const rg_follow_msg *>(d),
                       reinterpret_cast<const rg_follow_hdr *>(d + off_hdr), reinterpret_cast<const u32 *>(d + off_orig),
                       reinterpret_cast<const u32 *>(d + off_runs), (u32)runs, reinterpret_cast<const rg_follow_ent_run *>(d + off_ext),
                       reinterpret_cast<rg_follow_resp *>(d + off_resp), reinterpret_cast<rg_follow_gate_resp *>(d + off_gate));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rg_fail(RG_ERR_NO_DEVICE, "rg_follow_step_gated: launch failed: %s", hipGetErrorString(e));
    RG_HIP(hipMemcpyAsync(host_resp, d + off_resp, n * sizeof(rg_follow_resp), hipMemcpyDeviceToHost, h->stream));
    RG_HIP(hipMemcpyAsync(host_gate, d + off_gate, n * sizeof(rg_follow_gate_resp), hipMemcpyDeviceToHost, h->stream));
    RG_HIP(hipStreamSynchronize(h->stream)); // control path: the staging is reused by the next call
    return RG_OK;
} RG_ABI_GUARD

extern "C" int rg_follow_step_gated_device(rg_engine *h, const rg_follow_msgs *dev_msgs, const uint64_t *dev_term, const uint64_t *dev_from,
                                           const rg_follow_out *dev_out, uint8_t *dev_gate, uint8_t *dev_events, uint64_t *dev_resp_term) try {
    if (!h || !dev_msgs || !dev_out || !dev_term || !dev_from || !dev_gate || !dev_events || !dev_resp_term)
        return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_step_gated_device: bad argument");
    if (!h->fo || !h->fo->soft_arena) return rg_fail(RG_ERR_STATE, "rg_follow_step_gated_device: rg_follow_gate_enable first");
    const rg_follow_msgs &m = *dev_msgs;
    const rg_follow_out &o = *dev_out;
    if (!m.flags || !m.index || !m.log_term || !m.commit || !m.ent_term || !m.n_entries)
        return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_step_gated_device: a message column is NULL (only ext / ext_runs may be)");
    if (!o.status || !o.index || !o.commit || !o.conflict || !o.reject_hint || !o.log_term)
        return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_step_gated_device: a response column is NULL");
    RG_ENTER(h);
    RgFollowEngine *fo = h->fo;
    hipLaunchKernelGGL(k_follow_gate_dense, dim3(rg_grid(fo->cols.n, 256)), dim3(256), 0, h->stream, fo->cols, fo->soft, m, dev_term, dev_from, o, dev_gate,
                       dev_events, dev_resp_term);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rg_fail(RG_ERR_NO_DEVICE, "rg_follow_step_gated_device: launch failed: %s", hipGetErrorString(e));
    return RG_OK;
} RG_ABI_GUARD

extern "C" int rg_follow_clock(rg_engine *h, uint64_t *dev_hup, uint64_t cap, uint64_t *host_n) try {
    if (!h || (cap && !dev_hup)) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_clock: bad argument");
    if (!h->fo || !h->fo->soft_arena) return rg_fail(RG_ERR_STATE, "rg_follow_clock: rg_follow_gate_enable first");
    RG_ENTER(h);
    RgFollowEngine *fo = h->fo;
    RG_HIP(hipMemsetAsync(fo->clock_counts, 0, 16, h->stream));
    hipLaunchKernelGGL(k_follow_clock, dim3(rg_grid(fo->cols.n, 256)), dim3(256), 0, h->stream, fo->soft, fo->cols.n, dev_hup, cap, fo->clock_counts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rg_fail(RG_ERR_NO_DEVICE, "rg_follow_clock: launch failed: %s", hipGetErrorString(e));
    if (host_n) {
        RG_HIP(hipMemcpyAsync(host_n, fo->clock_counts, 8, hipMemcpyDeviceToHost, h->stream));
        RG_HIP(hipStreamSynchronize(h->stream));
    }
    return RG_OK;
} RG_ABI_GUARD
