// rg_handoff_host.h -- the host half that the units on the roads between the follower arena and the leader engine share
// (abi_handoff.hip, ext_lead.hip, ext_term.hip, ext_vote.hip): what they ask of the engine, the walk of a sparse call's records, its
// round trip, the launch of a kernel of either index width, the fetch of a dense call's count words.
#pragma once
#include "rg_engine.h"
#include "rg_kernels_handoff.h"

// The term stamps of the ReadIndex queues, which a group that stops leading drops its pending reads through; null while that layer is
// off (looked up per call: either enable order)
static inline u64 *rg_read_qterm(rg_engine *h) { return h->rd ? h->rd->cols.qterm : nullptr; }

// The layers' columns as the kernels take them: the one place that knows that a clock layer that is off gives empty RgLeadCols
// (cell == nullptr).
static inline RgArenaCols rg_arena_cols(rg_engine *h) {
    RgArenaCols c;
    c.st = h->st;
    c.fc = h->fo->cols;
    c.sc = h->fo->soft;
    c.ec = h->fo->elect;
    c.lc = h->ld ? h->ld->cols : RgLeadCols{};
    c.read_qterm = rg_read_qterm(h);
    return c;
}

// What every such road needs of the engine: the arena with its election layer; 0 = fine.
static inline int rg_elect_enabled(rg_engine *h, const char *who) {
    if (!h->fo || !h->fo->has(RG_FL_ELECT)) return rg_fail(RG_ERR_STATE, "%s: rg_follow_elect_enable first", who);
    return RG_OK;
}

static inline bool rg_handoff_out_complete(const rg_handoff_out &o) { return o.status && o.term && o.last_index; }

// The host side of a promotion (abi_handoff.hip, ext_handoff.hip). On an engine with a host mirror, events queued for a lead group
// belong to the old term (rg_local_become_leader's rule): -> the first record whose lead group has some, n where none has
static inline u64 rg_handoff_first_queued(const rg_engine *h, const rg_handoff_rec *recs, u64 n) {
    if (!h->host_mirror) return n;
    for (u64 i = 0; i < n; i++) {
        u64 row = 0;
        memcpy(&row, &h->q_mf[recs[i].lead_group * 8], 8);
        if (row) return i;
    }
    return n;
}
// ... what a launched promotion leaves behind
static inline void rg_handoff_promoted(rg_engine *h) {
    if (h->pub) h->pub->local_lost = true; // RG_COL_COMMIT was written outside a tick: the published advances no longer describe it
    h->host_res_valid = false;
}
// ... and a sparse one per DONE record
static inline void rg_handoff_registered(rg_engine *h, const rg_handoff_rec *recs, const rg_handoff_resp *resp, u64 n) {
    for (u64 i = 0; i < n; i++) {
        if (resp[i].status != RG_HANDOFF_DONE) continue;
        const u64 L = recs[i].lead_group;
        if (h->host_mirror) h->terms[L] = resp[i].term; // RG_COL_CUR_TERM and the registered term of a group belong together
        if (h->host_cfg_valid) h->host_cfg[L] &= ~(0xfu << 20); // (the transferee, if there was one, is gone)
    }
}

// One launch of kernel<IX> with the engine's index width over `blocks` blocks of 256 threads: the argument list is written once.
#define RG_LAUNCH_IX(h, kernel, blocks, ...)                                                                       \
    do {                                                                                                           \
        if (rg_ix32((h)->st, (h)->P)) hipLaunchKernelGGL(kernel<u32>, dim3(blocks), dim3(256), 0, (h)->stream, __VA_ARGS__); \
        else hipLaunchKernelGGL(kernel<u64>, dim3(blocks), dim3(256), 0, (h)->stream, __VA_ARGS__);               \
    } while (0)

// The walk of a sparse call's (follow_group, lead_group) records, in array order and per record: range, the caller's rule(record, i)
// (0 = fine), follow group seen before, lead group seen before -- so of several faults the first record's is reported.
enum {
    RG_WALK_NO_LEAD_OK = 1,  // a record may name RG_HANDOFF_NO_LEAD, any number of times
    RG_WALK_SIDE_IN_WHO = 2, // a repeat reads "<who> (follow): ... name group N" (the extension calls), else "<who>: ... name follow group N"
};
template <typename Rec, typename Rule>
static inline int rg_walk_pairs(rg_engine *h, const char *who, const Rec *recs, u64 n, unsigned flags, Rule rule) {
    const bool no_lead_ok = flags & RG_WALK_NO_LEAD_OK, side_in_who = flags & RG_WALK_SIDE_IN_WHO;
    RgSeen seen_f, seen_l;
    const auto once = [&](const char *side, const std::pair<RgSeen::iterator, bool> &ins, u64 i) {
        if (ins.second) return (int)RG_OK;
        const unsigned long long first = ins.first->second, group = ins.first->first;
        if (side_in_who) return rg_fail(RG_ERR_INVALID_ARG, "%s (%s): records %llu and %llu name group %llu", who, side, first, (unsigned long long)i, group);
        return rg_fail(RG_ERR_INVALID_ARG, "%s: records %llu and %llu name %s group %llu", who, first, (unsigned long long)i, side, group);
    };
    for (u64 i = 0; i < n; i++) {
        const Rec &q = recs[i];
        const bool no_lead = no_lead_ok && q.lead_group == RG_HANDOFF_NO_LEAD;
        if (q.follow_group >= h->fo->cols.n || (q.lead_group >= h->G && !no_lead))
            return rg_fail(RG_ERR_INVALID_ARG, "%s: record %llu: follow group %llu of %llu, lead group %llu of %llu", who, (unsigned long long)i,
                           (unsigned long long)q.follow_group, (unsigned long long)h->fo->cols.n, (unsigned long long)q.lead_group, (unsigned long long)h->G);
        if (int rc = rule(q, i)) return rc;
        if (int rc = once("follow", seen_f.emplace(q.follow_group, i), i)) return rc;
        if (!no_lead)
            if (int rc = once("lead", seen_l.emplace(q.lead_group, i), i)) return rc;
    }
    return RG_OK;
}
template <typename Rec> static inline int rg_walk_pairs(rg_engine *h, const char *who, const Rec *recs, u64 n, unsigned flags) { // (no rule of its own)
    return rg_walk_pairs(h, who, recs, n, flags, [](const Rec &, u64) { return (int)RG_OK; });
}

// The round trip of a sparse call: the records staged, launch(device records, device answers), the answers fetched. Synchronises:
// the staging is reused by the next call.
template <typename Rec, typename Resp, typename Launch>
static inline int rg_list_round_trip(rg_engine *h, const char *who, const Rec *recs, u64 n, Resp *host_resp, Launch launch) {
    RgFollowEngine *fo = h->fo;
    RgLayout lay;
    lay.add(n * sizeof(Rec));
    const size_t off_resp = lay.add(n * sizeof(Resp));
    fo->stage.assign(lay.total, 0);
    memcpy(fo->stage.data(), recs, n * sizeof(Rec));
    return rg_follow_round_trip(h, who, fo->stage.data(), lay.total,
                                [&](char *d) { launch(reinterpret_cast<const Rec *>(d), reinterpret_cast<Resp *>(d + off_resp)); },
                                {{host_resp, off_resp, n * sizeof(Resp)}});
}

// The count words of a dense call, copied to the host where it asks for them -- which synchronises.
static inline int rg_fetch_counts(rg_engine *h, uint64_t *host_counts, const unsigned long long *counts, size_t bytes) {
    if (!host_counts) return RG_OK;
    RG_HIP(hipMemcpyAsync(host_counts, counts, bytes, hipMemcpyDeviceToHost, h->stream));
    RG_HIP(hipStreamSynchronize(h->stream));
    return RG_OK;
}
