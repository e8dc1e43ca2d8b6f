// abi_follow.hip -- the follower half: MsgAppend / MsgHeartbeat steps on the device (include/raftgroups.h: "The follower half")
// There is NO CPU fallback anywhere in this file: without a HIP device every entry point fails.
#include "rg_engine.h"
#include "rg_kernels_follow.h"

extern "C" int rg_follow_enable(rg_engine *h, uint64_t n_follow) try {
    if (!h) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_enable: null engine");
    if (h->fo) return rg_fail(RG_ERR_STATE, "rg_follow_enable: already enabled (%llu groups)", (unsigned long long)h->fo->cols.n);
    if (n_follow < 1 || n_follow > (1ULL << 32)) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_enable: %llu groups, 1..2^32", (unsigned long long)n_follow);
    RG_ENTER(h);
    RgFollowEngine *fo = new RgFollowEngine();
    fo->arena = fo->ckpt = nullptr;
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
    delete fo;
    h->fo = nullptr;
}

int rg_follow_checkpoint(rg_engine *h) {
    RgFollowEngine *fo = h->fo;
    if (!fo) return RG_OK;
    if (!fo->ckpt) RG_HIP(hipMalloc(&fo->ckpt, fo->bytes));
    RG_HIP(hipMemcpyAsync(fo->ckpt, fo->arena, fo->bytes, hipMemcpyDeviceToDevice, h->stream));
    return RG_OK;
}

int rg_follow_restore(rg_engine *h) {
    RgFollowEngine *fo = h->fo;
    if (!fo || !fo->ckpt) return RG_OK;
    RG_HIP(hipMemcpyAsync(fo->arena, fo->ckpt, fo->bytes, hipMemcpyDeviceToDevice, h->stream));
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
