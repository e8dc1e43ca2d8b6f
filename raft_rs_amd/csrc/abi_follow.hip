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
    std::unique_ptr<RgFollowEngine> fo(new RgFollowEngine());
    RgFollowLayer &l = fo->layer[RG_FL_LOG];
    const u64 F = (n_follow + 255) & ~255ULL;
    // committed | last | tail_first | tail_term | dummy_idx | dummy_term | run_first[RG_TERM_RUNS] | run_term[RG_TERM_RUNS] | n_old
    const size_t bytes = (size_t)F * 8 * (6 + 2 * RG_TERM_RUNS) + (size_t)F;
    if (int rc = rg_follow_layer_alloc(h, "rg_follow_enable", &l, bytes, bytes)) return rc;
    u64 *a = reinterpret_cast<u64 *>(l.arena);
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
    if (int rc = rg_launch_check("rg_follow_enable")) {
        rg_follow_layer_drop(&l);
        return rc;
    }
    h->fo = fo.release();
    h->dev.engine_bytes += bytes;
    return RG_OK;
} RG_ABI_GUARD

extern "C" uint64_t rg_follow_stride(const rg_engine *h) { return h && h->fo ? h->fo->cols.stride : 0; }

// ---- what the other units call (rg_engine.h) ----
int rg_follow_layer_alloc(rg_engine *h, const char *who, RgFollowLayer *l, size_t bytes, size_t total) {
    hipError_t e = hipMalloc(&l->arena, total);
    if (e == hipSuccess) e = hipMemsetAsync(l->arena, 0, total, h->stream);
    if (e != hipSuccess) {
        rg_follow_layer_drop(l);
        return rg_fail(e == hipErrorOutOfMemory ? RG_ERR_OUT_OF_MEMORY : RG_ERR_NO_DEVICE, "%s: %s", who, hipGetErrorString(e));
    }
    l->bytes = bytes;
    return RG_OK;
}

void rg_follow_layer_drop(RgFollowLayer *l) {
    if (l->arena) (void)hipFree(l->arena);
    if (l->ckpt) (void)hipFree(l->ckpt);
    *l = RgFollowLayer();
}

void rg_follow_free(rg_engine *h) {
    if (!h->fo) return;
    for (RgFollowLayer &l : h->fo->layer) rg_follow_layer_drop(&l);
    delete h->fo;
    h->fo = nullptr;
}

int rg_follow_checkpoint(rg_engine *h) {
    if (!h->fo) return RG_OK;
    for (RgFollowLayer &l : h->fo->layer) {
        if (!l.arena) continue;
        if (!l.ckpt) RG_HIP(hipMalloc(&l.ckpt, l.bytes));
        RG_HIP(hipMemcpyAsync(l.ckpt, l.arena, l.bytes, hipMemcpyDeviceToDevice, h->stream));
    }
    return RG_OK;
}

int rg_follow_restore(rg_engine *h) {
    if (!h->fo || !h->fo->layer[RG_FL_LOG].ckpt) return RG_OK;
    for (RgFollowLayer &l : h->fo->layer)
        if (l.ckpt) RG_HIP(hipMemcpyAsync(l.arena, l.ckpt, l.bytes, hipMemcpyDeviceToDevice, h->stream));
    return RG_OK;
}

int rg_follow_round_trip(rg_engine *h, const char *who, const void *src, size_t bytes, const std::function<void(char *)> &launch,
                         std::initializer_list<RgFetch> fetch) {
    int rc = rg_stage_records(h, src, bytes);
    if (rc) return rc;
    char *d = static_cast<char *>(h->d_recs);
    launch(d);
    if ((rc = rg_launch_check(who))) return rc;
    for (const RgFetch &f : fetch)
        if (f.dst) RG_HIP(hipMemcpyAsync(f.dst, d + f.off, f.bytes, hipMemcpyDeviceToHost, h->stream));
    RG_HIP(hipStreamSynchronize(h->stream)); // control path: the staging is reused by the next call
    return RG_OK;
}

// The NULL-column checks of both dense steps
static bool rg_follow_msgs_complete(const rg_follow_msgs &m) { return m.flags && m.index && m.log_term && m.commit && m.ent_term && m.n_entries; }
static bool rg_follow_out_complete(const rg_follow_out &o) { return o.status && o.index && o.commit && o.conflict && o.reject_hint && o.log_term; }

// The sparse road of both steps: the n records sorted by group -- stable, so a group's records keep their array order --, cut
// into runs and staged as  msgs | hdrs (gated) | orig | run_start | ext | resp | gate (gated),  applied, answered at the records'
// original positions.
static int rg_follow_run_list(rg_engine *h, const char *who, const rg_follow_msg *host_msgs, const rg_follow_hdr *host_hdr, u64 n,
                              const rg_follow_ent_run *host_ext, u64 n_ext, rg_follow_resp *host_resp, rg_follow_gate_resp *host_gate) {
    RgFollowEngine *fo = h->fo;
    const auto group_of = [&](u64 i) { return host_msgs[i].group; };
    const u64 runs = rg_runs_sort(fo->order, n, group_of);
    RgLayout lay;
    lay.add(n * sizeof(rg_follow_msg));
    const size_t off_hdr = host_hdr ? lay.add(n * sizeof(rg_follow_hdr)) : 0, off_orig = lay.add(n * 4), off_runs = lay.add((runs + 1) * 4),
                 off_ext = lay.add(n_ext * sizeof(rg_follow_ent_run)), off_resp = lay.add(n * sizeof(rg_follow_resp)),
                 off_gate = host_gate ? lay.add(n * sizeof(rg_follow_gate_resp)) : 0;
    fo->stage.assign(lay.total, 0);
    char *s = fo->stage.data();
    rg_runs_cut(fo->order, group_of, reinterpret_cast<u32 *>(s + off_orig), reinterpret_cast<u32 *>(s + off_runs));
    for (u64 i = 0; i < n; i++) {
        reinterpret_cast<rg_follow_msg *>(s)[i] = host_msgs[fo->order[i]];
        if (host_hdr) reinterpret_cast<rg_follow_hdr *>(s + off_hdr)[i] = host_hdr[fo->order[i]];
    }
    if (n_ext) memcpy(s + off_ext, host_ext, n_ext * sizeof(rg_follow_ent_run));
    const auto launch = [&](char *d) {
        const rg_follow_msg *msgs = reinterpret_cast<const rg_follow_msg *>(d);
        const u32 *orig = reinterpret_cast<const u32 *>(d + off_orig), *rs = reinterpret_cast<const u32 *>(d + off_runs);
        const rg_follow_ent_run *ext = reinterpret_cast<const rg_follow_ent_run *>(d + off_ext);
        rg_follow_resp *resp = reinterpret_cast<rg_follow_resp *>(d + off_resp);
        if (host_hdr)
            hipLaunchKernelGGL(k_follow_gate_list, dim3(rg_grid(runs, 256)), dim3(256), 0, h->stream, fo->cols, fo->soft, msgs,
                               reinterpret_cast<const rg_follow_hdr *>(d + off_hdr), orig, rs, (u32)runs, ext, resp, reinterpret_cast<rg_follow_gate_resp *>(d + off_gate));
        else hipLaunchKernelGGL(k_follow_list, dim3(rg_grid(runs, 256)), dim3(256), 0, h->stream, fo->cols, msgs, orig, rs, (u32)runs, ext, resp);
    };
    return rg_follow_round_trip(h, who, s, lay.total, launch,
                                {{host_resp, off_resp, n * sizeof(rg_follow_resp)}, {host_gate, off_gate, n * sizeof(rg_follow_gate_resp)}});
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
    return rg_follow_round_trip(h, "rg_follow_write", fo->states.data(), k * sizeof(rg_follow_state), [&](char *d) {
        hipLaunchKernelGGL(k_follow_write, dim3(rg_grid(k, 256)), dim3(256), 0, h->stream, fo->cols, reinterpret_cast<const rg_follow_state *>(d), k);
    });
} RG_ABI_GUARD

extern "C" int rg_follow_read(rg_engine *h, const uint64_t *host_groups, uint64_t n, rg_follow_state *host_out) try {
    if (!h || (n && (!host_groups || !host_out))) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_read: bad argument");
    if (!h->fo) return rg_fail(RG_ERR_STATE, "rg_follow_read: rg_follow_enable first");
    return rg_follow_gather(h, "rg_follow_read", host_groups, n, host_out, [&](const u64 *d_groups, rg_follow_state *d_out) {
        hipLaunchKernelGGL(k_follow_read, dim3(rg_grid(n, 256)), dim3(256), 0, h->stream, h->fo->cols, d_groups, n, d_out);
    });
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
    return rg_follow_run_list(h, "rg_follow_step", host_msgs, nullptr, n, host_ext, n_ext, host_resp, nullptr);
} RG_ABI_GUARD

extern "C" int rg_follow_step_device(rg_engine *h, const rg_follow_msgs *dev_msgs, const rg_follow_out *dev_out) try {
    if (!h || !dev_msgs || !dev_out) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_step_device: bad argument");
    if (!h->fo) return rg_fail(RG_ERR_STATE, "rg_follow_step_device: rg_follow_enable first");
    if (!rg_follow_msgs_complete(*dev_msgs))
        return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_step_device: a message column is NULL (only ext / ext_runs may be)");
    if (!rg_follow_out_complete(*dev_out)) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_step_device: a response column is NULL");
    RG_ENTER(h);
    RgFollowEngine *fo = h->fo;
    hipLaunchKernelGGL(k_follow_dense, dim3(rg_grid(fo->cols.n, 256)), dim3(256), 0, h->stream, fo->cols, *dev_msgs, *dev_out);
    return rg_launch_check("rg_follow_step_device");
} RG_ABI_GUARD

// ---- the term gate, the vote step and the election clock ----
extern "C" int rg_follow_gate_enable(rg_engine *h, const rg_follow_gate_config *cfg) try {
    if (!h || !cfg) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_gate_enable: bad argument");
    if (!h->fo) return rg_fail(RG_ERR_STATE, "rg_follow_gate_enable: rg_follow_enable first");
    RgFollowEngine *fo = h->fo;
    if (fo->has(RG_FL_SOFT)) return rg_fail(RG_ERR_STATE, "rg_follow_gate_enable: already enabled");
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
    RgFollowLayer &l = fo->layer[RG_FL_SOFT];
    if (int rc = rg_follow_layer_alloc(h, "rg_follow_gate_enable", &l, bytes, total)) return rc;
    RgSoftCols sc;
    sc.term = reinterpret_cast<u64 *>(l.arena);
    sc.lead = sc.term + F;
    sc.vote = sc.term + 2 * F;
    sc.priority = reinterpret_cast<int64_t *>(sc.term + 3 * F);
    sc.clock = reinterpret_cast<u32 *>(sc.term + 4 * F);
    sc.role = reinterpret_cast<u8 *>(sc.clock + F);
    sc.cfg = g;
    hipLaunchKernelGGL(k_follow_soft_init, dim3(rg_grid(F, 256)), dim3(256), 0, h->stream, sc, F);
    if (int rc = rg_launch_check("rg_follow_gate_enable")) {
        rg_follow_layer_drop(&l);
        return rc;
    }
    fo->soft = sc;
    fo->clock_counts = reinterpret_cast<unsigned long long *>(l.arena + bytes);
    h->dev.engine_bytes += total;
    return RG_OK;
} RG_ABI_GUARD

extern "C" const uint64_t *rg_follow_clock_counts(const rg_engine *h) {
    return h && h->fo ? reinterpret_cast<const uint64_t *>(h->fo->clock_counts) : nullptr; // (null until the gate is enabled)
}

extern "C" int rg_follow_soft_write(rg_engine *h, const rg_follow_soft *host, uint64_t n) try {
    if (!h || (!host && n)) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_soft_write: bad argument");
    if (!h->fo || !h->fo->has(RG_FL_SOFT)) return rg_fail(RG_ERR_STATE, "rg_follow_soft_write: rg_follow_gate_enable first");
    RgFollowEngine *fo = h->fo;
    RgSeen seen;
    for (u64 i = 0; i < n; i++) {
        const rg_follow_soft &w = host[i];
        if (w.group >= fo->cols.n)
            return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_soft_write: record %llu: group %llu of %llu", (unsigned long long)i, (unsigned long long)w.group,
                           (unsigned long long)fo->cols.n);
        const int rule = rg_follow_soft_check(w, fo->soft.cfg.min_timeout, fo->soft.cfg.max_timeout);
        if (rule)
            return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_soft_write: record %llu (group %llu) breaks rule %d of rg_follow_soft_check", (unsigned long long)i,
                           (unsigned long long)w.group, rule);
        if (int rc = rg_named_once("rg_follow_soft_write", seen.emplace(w.group, i), i)) return rc;
    }
    if (n == 0) return RG_OK;
    RG_ENTER(h);
    return rg_follow_round_trip(h, "rg_follow_soft_write", host, n * sizeof(rg_follow_soft), [&](char *d) {
        hipLaunchKernelGGL(k_follow_soft_write, dim3(rg_grid(n, 256)), dim3(256), 0, h->stream, fo->soft, reinterpret_cast<const rg_follow_soft *>(d), n);
    });
} RG_ABI_GUARD

extern "C" int rg_follow_soft_read(rg_engine *h, const uint64_t *host_groups, uint64_t n, rg_follow_soft *host_out) try {
    if (!h || (n && (!host_groups || !host_out))) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_soft_read: bad argument");
    if (!h->fo || !h->fo->has(RG_FL_SOFT)) return rg_fail(RG_ERR_STATE, "rg_follow_soft_read: rg_follow_gate_enable first");
    return rg_follow_gather(h, "rg_follow_soft_read", host_groups, n, host_out, [&](const u64 *d_groups, rg_follow_soft *d_out) {
        hipLaunchKernelGGL(k_follow_soft_read, dim3(rg_grid(n, 256)), dim3(256), 0, h->stream, h->fo->soft, d_groups, n, d_out);
    });
} RG_ABI_GUARD

extern "C" int rg_follow_step_gated(rg_engine *h, const rg_follow_msg *host_msgs, const rg_follow_hdr *host_hdr, uint64_t n,
                                    const rg_follow_ent_run *host_ext, uint64_t n_ext, rg_follow_resp *host_resp, rg_follow_gate_resp *host_gate) try {
    if (!h || (n && (!host_msgs || !host_hdr || !host_resp || !host_gate)) || (n_ext && !host_ext))
        return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_step_gated: bad argument");
    if (!h->fo || !h->fo->has(RG_FL_SOFT)) return rg_fail(RG_ERR_STATE, "rg_follow_step_gated: rg_follow_gate_enable first");
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
    return rg_follow_run_list(h, "rg_follow_step_gated", host_msgs, host_hdr, n, host_ext, n_ext, host_resp, host_gate);
} RG_ABI_GUARD

extern "C" int rg_follow_step_gated_device(rg_engine *h, const rg_follow_msgs *dev_msgs, const uint64_t *dev_term, const uint64_t *dev_from,
                                           const rg_follow_out *dev_out, uint8_t *dev_gate, uint8_t *dev_events, uint64_t *dev_resp_term) try {
    if (!h || !dev_msgs || !dev_out || !dev_term || !dev_from || !dev_gate || !dev_events || !dev_resp_term)
        return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_step_gated_device: bad argument");
    if (!h->fo || !h->fo->has(RG_FL_SOFT)) return rg_fail(RG_ERR_STATE, "rg_follow_step_gated_device: rg_follow_gate_enable first");
    if (!rg_follow_msgs_complete(*dev_msgs))
        return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_step_gated_device: a message column is NULL (only ext / ext_runs may be)");
    if (!rg_follow_out_complete(*dev_out)) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_step_gated_device: a response column is NULL");
    RG_ENTER(h);
    RgFollowEngine *fo = h->fo;
    hipLaunchKernelGGL(k_follow_gate_dense, dim3(rg_grid(fo->cols.n, 256)), dim3(256), 0, h->stream, fo->cols, fo->soft, *dev_msgs, dev_term, dev_from, *dev_out,
                       dev_gate, dev_events, dev_resp_term);
    return rg_launch_check("rg_follow_step_gated_device");
} RG_ABI_GUARD

extern "C" int rg_follow_clock(rg_engine *h, uint64_t *dev_hup, uint64_t cap, uint64_t *host_n) try {
    if (!h || (cap && !dev_hup)) return rg_fail(RG_ERR_INVALID_ARG, "rg_follow_clock: bad argument");
    if (!h->fo || !h->fo->has(RG_FL_SOFT)) return rg_fail(RG_ERR_STATE, "rg_follow_clock: rg_follow_gate_enable first");
    RG_ENTER(h);
    RgFollowEngine *fo = h->fo;
    RG_HIP(hipMemsetAsync(fo->clock_counts, 0, 16, h->stream));
    hipLaunchKernelGGL(k_follow_clock, dim3(rg_grid(fo->cols.n, 256)), dim3(256), 0, h->stream, fo->soft, fo->cols.n, dev_hup, cap, fo->clock_counts);
    if (int rc = rg_launch_check("rg_follow_clock")) return rc;
    if (host_n) {
        RG_HIP(hipMemcpyAsync(host_n, fo->clock_counts, 8, hipMemcpyDeviceToHost, h->stream));
        RG_HIP(hipStreamSynchronize(h->stream));
    }
    return RG_OK;
} RG_ABI_GUARD
