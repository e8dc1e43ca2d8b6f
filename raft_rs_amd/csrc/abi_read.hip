// abi_read.hip -- ReadIndex: pending-read queues and the ack quorum on the device (include/raftgroups.h: "ReadIndex")
// There is NO CPU fallback anywhere in this file: without a HIP device every entry point fails.
#include "rg_engine.h"
#include "rg_kernels_read.h"

#define RG_READ_LIST_CAP0 256u

static RgReadList rg_read_list(const RgReadEngine *rd) {
    RgReadList l;
    l.items = rd->items;
    l.count = rd->count;
    l.cap = rd->cap;
    return l;
}

extern "C" int rg_read_index_enable(rg_engine *h, uint32_t depth) try {
    if (!h) return rg_fail(RG_ERR_INVALID_ARG, "rg_read_index_enable: null engine");
    if (depth < 1 || depth > RG_READ_MAX_DEPTH) return rg_fail(RG_ERR_INVALID_ARG, "rg_read_index_enable: depth %u, 1..%u", depth, RG_READ_MAX_DEPTH);
    if (h->rd) return rg_fail(RG_ERR_STATE, "rg_read_index_enable: already enabled (depth %u)", h->rd->cols.depth);
    RG_ENTER(h);
    RgReadEngine *rd = new RgReadEngine();
    rd->arena = rd->ckpt = nullptr;
    rd->items = nullptr;
    rd->count = nullptr;
    rd->off_qterm = rg_align((size_t)h->stride * 4);
    rd->off_ctx = rd->off_qterm + rg_align((size_t)h->stride * 8);
    rd->off_idx = rd->off_ctx + rg_align((size_t)depth * h->stride * 8);
    rd->off_acks = rd->off_idx + rg_align((size_t)depth * h->stride * 8);
    rd->bytes = rd->off_acks + rg_align((size_t)depth * h->stride);
    rd->cap = RG_READ_LIST_CAP0;
    rd->outstanding = rd->ckpt_outstanding = 0;
    hipError_t e = hipMalloc(&rd->arena, rd->bytes);
    if (e == hipSuccess) e = hipMalloc(&rd->items, rd->cap * sizeof(rg_read_state));
    if (e == hipSuccess) e = hipMalloc(&rd->count, 256);
    if (e == hipSuccess) e = hipMemsetAsync(rd->arena, 0, rd->bytes, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(rd->count, 0, 256, h->stream);
    if (e != hipSuccess) {
        if (rd->arena) (void)hipFree(rd->arena);
        if (rd->items) (void)hipFree(rd->items);
        if (rd->count) (void)hipFree(rd->count);
        delete rd;
        return rg_fail(e == hipErrorOutOfMemory ? RG_ERR_OUT_OF_MEMORY : RG_ERR_NO_DEVICE, "rg_read_index_enable: %s", hipGetErrorString(e));
    }
    rd->cols.qw = reinterpret_cast<u32 *>(rd->arena);
    rd->cols.qterm = reinterpret_cast<u64 *>(rd->arena + rd->off_qterm);
    rd->cols.ctx = reinterpret_cast<u64 *>(rd->arena + rd->off_ctx);
    rd->cols.idx = reinterpret_cast<u64 *>(rd->arena + rd->off_idx);
    rd->cols.acks = reinterpret_cast<u8 *>(rd->arena + rd->off_acks);
    rd->cols.stride = h->stride;
    rd->cols.depth = depth;
    h->rd = rd;
    h->dev.engine_bytes += rd->bytes;
    return RG_OK;
} RG_ABI_GUARD

// ---- what the other units call (rg_engine.h) ----
void rg_read_free(rg_engine *h) {
    RgReadEngine *rd = h->rd;
    if (!rd) return;
    if (rd->arena) (void)hipFree(rd->arena);
    if (rd->ckpt) (void)hipFree(rd->ckpt);
    if (rd->items) (void)hipFree(rd->items);
    if (rd->count) (void)hipFree(rd->count);
    delete rd;
    h->rd = nullptr;
}

int rg_read_checkpoint(rg_engine *h) {
    RgReadEngine *rd = h->rd;
    if (!rd) return RG_OK;
    if (!rd->ckpt) RG_HIP(hipMalloc(&rd->ckpt, rd->bytes));
    RG_HIP(hipMemcpyAsync(rd->ckpt, rd->arena, rd->bytes, hipMemcpyDeviceToDevice, h->stream));
    rd->ckpt_outstanding = rd->outstanding;
    return RG_OK;
}

static int rg_read_reserve_list(rg_engine *h, u64 more);
int rg_read_restore(rg_engine *h) {
    RgReadEngine *rd = h->rd;
    if (!rd || !rd->ckpt) return RG_OK;
    RG_HIP(hipMemcpyAsync(rd->arena, rd->ckpt, rd->bytes, hipMemcpyDeviceToDevice, h->stream));
    // the undrained list stays (read states already handed to the host's side of the boundary are not taken back); the reads that
    // were pending at the checkpoint are pending again on top of it, and acks alone can turn them into states: make room now
    rd->outstanding += rd->ckpt_outstanding;
    return rg_read_reserve_list(h, 0);
}

// The list's capacity covers everything that can reach it: raised here, on the control path, before a request call adds `more`.
static int rg_read_reserve_list(rg_engine *h, u64 more) {
    RgReadEngine *rd = h->rd;
    const u64 need = rd->outstanding + more;
    if (need <= rd->cap) return RG_OK;
    u64 cap = rd->cap;
    while (cap < need) cap *= 2;
    rg_read_state *items = nullptr;
    hipError_t e = hipMalloc(&items, cap * sizeof(rg_read_state));
    if (e != hipSuccess) return rg_fail(RG_ERR_OUT_OF_MEMORY, "read states: hipMalloc(%llu items) failed: %s", (unsigned long long)cap, hipGetErrorString(e));
    e = hipMemcpyAsync(items, rd->items, rd->cap * sizeof(rg_read_state), hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream); // (kernels writing the old list)
    if (e != hipSuccess) {
        (void)hipFree(items);
        return rg_fail(RG_ERR_NO_DEVICE, "read states: growing the list failed: %s", hipGetErrorString(e));
    }
    (void)hipFree(rd->items);
    rd->items = items;
    rd->cap = cap;
    return RG_OK;
}

// One batch through k_read_list: rd->recs (any order) is sorted by group -- stable, so a group's records keep their arrival
// order --, cut into runs, staged and applied; status (may be null) receives the requests' RG_READ_* bytes. Synchronises.
static int rg_read_apply(rg_engine *h, const char *who, u8 *host_status) {
    RgReadEngine *rd = h->rd;
    std::vector<RgReadRec> &recs = rd->recs;
    const u64 n = recs.size();
    std::stable_sort(recs.begin(), recs.end(), [](const RgReadRec &a, const RgReadRec &b) { return a.group < b.group; });
    u64 runs = 0;
    for (u64 i = 0; i < n; i++) runs += i == 0 || recs[i].group != recs[i - 1].group;
    const size_t off_runs = n * sizeof(RgReadRec), off_status = off_runs + (runs + 1) * 4;
    rd->stage.assign(off_status + n, 0);
    memcpy(rd->stage.data(), recs.data(), off_runs);
    u32 *rs = reinterpret_cast<u32 *>(rd->stage.data() + off_runs);
    u64 r = 0;
    for (u64 i = 0; i < n; i++)
        if (i == 0 || recs[i].group != recs[i - 1].group) rs[r++] = (u32)i;
    rs[r] = (u32)n;
    int rc = rg_stage_records(h, rd->stage.data(), rd->stage.size());
    if (rc) return rc;
    char *d = static_cast<char *>(h->d_recs);
    hipLaunchKernelGGL(k_read_list, dim3(rg_grid(runs, 256)), dim3(256), 0, h->stream, h->st, rd->cols, reinterpret_cast<const RgReadRec *>(d),
                       reinterpret_cast<const u32 *>(d + off_runs), (u32)runs, reinterpret_cast<u8 *>(d + off_status), rg_read_list(rd));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rg_fail(RG_ERR_NO_DEVICE, "%s: launch failed: %s", who, hipGetErrorString(e));
    if (host_status) RG_HIP(hipMemcpyAsync(host_status, d + off_status, n, hipMemcpyDeviceToHost, h->stream));
    RG_HIP(hipStreamSynchronize(h->stream)); // control path: the staging is reused by the next call
    return RG_OK;
}

extern "C" int rg_read_index(rg_engine *h, const rg_read_req *host_reqs, uint64_t n, uint32_t flags, uint8_t *host_status) try {
    if (!h || (!host_reqs && n)) return rg_fail(RG_ERR_INVALID_ARG, "rg_read_index: bad argument");
    if (!h->rd) return rg_fail(RG_ERR_STATE, "rg_read_index: rg_read_index_enable first");
    if (flags & ~RG_READ_LEASE) return rg_fail(RG_ERR_INVALID_ARG, "rg_read_index: unknown flags %#x", flags);
    if (n >= 0xffffffffULL) return rg_fail(RG_ERR_INVALID_ARG, "rg_read_index: %llu requests in one call", (unsigned long long)n);
    for (u64 i = 0; i < n; i++)
        if (host_reqs[i].group >= h->G || host_reqs[i].ctx == 0)
            return rg_fail(RG_ERR_INVALID_ARG, "rg_read_index: request %llu: group %llu of %llu, ctx %llu (0 is the empty context)", (unsigned long long)i,
                           (unsigned long long)host_reqs[i].group, (unsigned long long)h->G, (unsigned long long)host_reqs[i].ctx);
    if (n == 0) return RG_OK;
    RG_ENTER(h);
    RgReadEngine *rd = h->rd;
    int rc = rg_read_reserve_list(h, n);
    if (rc) return rc;
    rd->recs.resize(n);
    for (u64 i = 0; i < n; i++) {
        RgReadRec &r = rd->recs[i];
        r.group = host_reqs[i].group;
        r.ctx = host_reqs[i].ctx;
        r.slot = 0;
        r.flags = RG_READ_REC_REQUEST | ((flags & RG_READ_LEASE) ? RG_READ_REC_LEASE : 0u);
        r.orig = (u32)i;
        r.pad = 0;
    }
    std::vector<u8> status(n);
    rd->outstanding += n; // (if the call fails half way the bound stays a bound)
    rc = rg_read_apply(h, "rg_read_index", status.data());
    if (rc) return rc;
    u64 accepted = 0;
    for (u64 i = 0; i < n; i++) accepted += status[i] == RG_READ_READY || status[i] == RG_READ_QUEUED;
    rd->outstanding -= n - accepted;
    if (host_status) memcpy(host_status, status.data(), n);
    return RG_OK;
} RG_ABI_GUARD

extern "C" int rg_read_acks(rg_engine *h, const rg_read_ack *host_acks, uint64_t n) try {
    if (!h || (!host_acks && n)) return rg_fail(RG_ERR_INVALID_ARG, "rg_read_acks: bad argument");
    if (!h->rd) return rg_fail(RG_ERR_STATE, "rg_read_acks: rg_read_index_enable first");
    if (n >= 0xffffffffULL) return rg_fail(RG_ERR_INVALID_ARG, "rg_read_acks: %llu records in one call", (unsigned long long)n);
    for (u64 i = 0; i < n; i++)
        if (host_acks[i].group >= h->G || (host_acks[i].flags & ~RG_READ_ACK_LAST_SELF))
            return rg_fail(RG_ERR_INVALID_ARG, "rg_read_acks: record %llu: group %llu of %llu, flags %#x", (unsigned long long)i,
                           (unsigned long long)host_acks[i].group, (unsigned long long)h->G, host_acks[i].flags);
    if (n == 0) return RG_OK;
    RG_ENTER(h);
    RgReadEngine *rd = h->rd;
    rd->recs.resize(n);
    for (u64 i = 0; i < n; i++) {
        RgReadRec &r = rd->recs[i];
        r.group = host_acks[i].group;
        r.ctx = host_acks[i].ctx;
        r.slot = host_acks[i].slot;
        r.flags = host_acks[i].flags;
        r.orig = (u32)i;
        r.pad = 0;
    }
    return rg_read_apply(h, "rg_read_acks", nullptr);
} RG_ABI_GUARD

extern "C" int rg_read_acks_device(rg_engine *h, const uint64_t *dev_ctx) try {
    if (!h || !dev_ctx) return rg_fail(RG_ERR_INVALID_ARG, "rg_read_acks_device: bad argument");
    if (!h->rd) return rg_fail(RG_ERR_STATE, "rg_read_acks_device: rg_read_index_enable first");
    RG_ENTER(h);
    RgReadEngine *rd = h->rd;
    rg_with_p(h->P, [&](auto p) {
        hipLaunchKernelGGL((k_read_acks_dense<decltype(p)::value>), dim3(rg_grid(h->G, 256)), dim3(256), 0, h->stream, h->st, rd->cols,
                           (const u64 *)dev_ctx, rg_read_list(rd));
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rg_fail(RG_ERR_NO_DEVICE, "rg_read_acks_device: launch failed: %s", hipGetErrorString(e));
    return RG_OK;
} RG_ABI_GUARD

extern "C" int rg_read_states(rg_engine *h, rg_read_state *host_items, uint64_t cap, uint64_t *n) try {
    if (!h || !n || (!host_items && cap)) return rg_fail(RG_ERR_INVALID_ARG, "rg_read_states: bad argument");
    if (!h->rd) return rg_fail(RG_ERR_STATE, "rg_read_states: rg_read_index_enable first");
    RG_ENTER(h);
    RgReadEngine *rd = h->rd;
    unsigned long long count = 0;
    RG_HIP(hipMemcpyAsync(&count, rd->count, 8, hipMemcpyDeviceToHost, h->stream));
    RG_HIP(hipStreamSynchronize(h->stream));
    *n = count;
    if (count > rd->cap) // (cannot happen while `outstanding` is a bound; exact or loud, never silently short)
        return rg_fail(RG_ERR_STATE, "rg_read_states: %llu states were emitted into a list of %llu: states were lost", count, (unsigned long long)rd->cap);
    if (cap == 0) return RG_OK;
    const u64 k = count < cap ? count : cap;
    if (k) RG_HIP(hipMemcpyAsync(host_items, rd->items, k * sizeof(rg_read_state), hipMemcpyDeviceToHost, h->stream));
    RG_HIP(hipMemsetAsync(rd->count, 0, 8, h->stream));
    RG_HIP(hipStreamSynchronize(h->stream));
    // what is left of the bound is pending in the queues, and they hold `depth` reads per group at most (reads a term change
    // dropped leave the bound here)
    const u64 left = rd->outstanding > count ? rd->outstanding - count : 0, room = h->G * rd->cols.depth;
    rd->outstanding = left < room ? left : room;
    return RG_OK;
} RG_ABI_GUARD

static int rg_read_pending_impl(rg_engine *h, const char *who, u64 *dev_ctx, u64 *host_ctx, u8 *host_counts) {
    RG_ENTER(h);
    RgReadEngine *rd = h->rd;
    char *tmp = nullptr;
    const size_t ctx_b = rg_align((size_t)h->G * 8);
    if (host_counts || !dev_ctx) RG_HIP(hipMalloc(&tmp, ctx_b + h->G));
    u64 *d_ctx = host_counts ? nullptr : dev_ctx ? dev_ctx : reinterpret_cast<u64 *>(tmp);
    u8 *d_counts = host_counts ? reinterpret_cast<u8 *>(tmp + ctx_b) : nullptr;
    hipLaunchKernelGGL(k_read_pending, dim3(rg_grid(h->G, 256)), dim3(256), 0, h->stream, h->st, rd->cols, d_ctx, d_counts);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && host_ctx) e = hipMemcpyAsync(host_ctx, d_ctx, h->G * 8, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && host_counts) e = hipMemcpyAsync(host_counts, d_counts, h->G, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && (host_ctx || host_counts || tmp)) e = hipStreamSynchronize(h->stream);
    if (tmp) (void)hipFree(tmp);
    if (e != hipSuccess) return rg_fail(RG_ERR_NO_DEVICE, "%s: %s", who, hipGetErrorString(e));
    return RG_OK;
}

extern "C" int rg_read_last_pending(rg_engine *h, uint64_t *dev_ctx_g, uint64_t *host_ctx_g) try {
    if (!h || (!dev_ctx_g && !host_ctx_g)) return rg_fail(RG_ERR_INVALID_ARG, "rg_read_last_pending: no destination");
    if (!h->rd) return rg_fail(RG_ERR_STATE, "rg_read_last_pending: rg_read_index_enable first");
    return rg_read_pending_impl(h, "rg_read_last_pending", dev_ctx_g, host_ctx_g, nullptr);
} RG_ABI_GUARD

extern "C" int rg_read_pending_counts(rg_engine *h, uint8_t *host_counts) try {
    if (!h || !host_counts) return rg_fail(RG_ERR_INVALID_ARG, "rg_read_pending_counts: no destination");
    if (!h->rd) return rg_fail(RG_ERR_STATE, "rg_read_pending_counts: rg_read_index_enable first");
    return rg_read_pending_impl(h, "rg_read_pending_counts", nullptr, nullptr, host_counts);
} RG_ABI_GUARD
