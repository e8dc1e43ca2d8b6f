// rg_engine.h -- what the ABI units (abi_*.hip) share: the engine object, error plumbing, entry discipline, and the internal
// functions one unit provides to another. Nothing here is exported: the library is built with -fvisibility=hidden and only
// the entry points include/raftgroups.h declares are visible (tests/test_abi.py compares the two lists).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <memory>
#include <new>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <vector>

#pragma GCC visibility push(default)
#include "../../include/raftgroups.h"
#include "../../include/raftgroups_lead.h"
#include "../../include/raftgroups_term.h"
#pragma GCC visibility pop

#include "rg_group.h"
#include "rg_send.h"
#include "rg_wire.h"
#include "rg_workload.h"
#include "rg_read.h"
#include "rg_follow.h"
#include "rg_elect.h"
#include "rg_lead.h"

#include "rg_tick_kernels.h"
#include "rg_grow.h"
#include "rg_runs.h"

// live engines of this process PER DEVICE: the Infinity Cache is one per device, and a range of ONE engine only stays
// resident there (k_tick_split) while no other engine's traffic goes through it. Looked at ONCE, by rg_create, when the cache
// policy of the new engine is decided (RG_CACHE_AUTO grants a resident range only to an engine that is alone on its device);
// a live engine's kernel never changes because another engine comes or goes.
#define RG_MAX_DEVICES 64

// ---- error plumbing (abi_state.hip): rg_fail, RG_ABI_GUARD ----
#include "rg_abi_guard.h"

#define RG_HIP(expr)                                                                               \
    do {                                                                                           \
        hipError_t e__ = (expr);                                                                   \
        if (e__ != hipSuccess)                                                                     \
            return rg_fail(e__ == hipErrorOutOfMemory ? RG_ERR_OUT_OF_MEMORY : RG_ERR_NO_DEVICE,   \
                           "%s failed: %s", #expr, hipGetErrorString(e__));                        \
    } while (0)

struct rg_engine;
int rg_mailbox_quiesce(rg_engine *h);            // abi_mirror.hip
int rg_require_hints_resolved(rg_engine *h, const char *who); // abi_tick.hip
// abi_tick.hip: one step of the read mirror's host state (rg_mirror_host.h) for a call of class `call` that launches no mirror
// kernel itself; where the step asks for it, the settle kernel goes onto the engine's stream. -> RG_OK or the launch's error
int rg_mirror_settle(rg_engine *h, RgMirrorCall call);
// Every entry point that puts work on the engine's stream starts here: select the device and, if the resident mailbox
// kernel is on the stream (rg_mailbox_start), tell it to leave -- stream order would make the call wait for it anyway
// (until its idle timeout), this makes the wait a few microseconds.
// It also drops the read mirror of the dense lane tick (rg_engine::mirror_valid, rg_mirror.h): whatever this call does, the next
// dense tick rebuilds the plane from the columns. Dropping is always right; the few entry points that are KNOWN to write none of
// RG_COL_MATCH / RG_COL_PR_COMMIT / RG_COL_COMMIT -- the dense tick itself, rg_results, rg_result_counts, rg_sync, rg_msg_stats,
// rg_read_column, the workload generator -- enter through RG_ENTER_KEEP / RG_ENTER_STEP_KEEP, which put the flag back.
#define RG_ENTER_BASE(h)                                                                           \
    do {                                                                                           \
        (h)->mirror_valid = false;                                                                 \
        (h)->pub_tick_evt = -1; /* (whatever this call enqueues comes behind the last tick's event) */ \
        RG_HIP(hipSetDevice((h)->cfg.device));                                                     \
        int rc__ = rg_mailbox_quiesce(h);                                                          \
        if (rc__) return rc__;                                                                     \
    } while (0)
// ... behind the SETTLE: where write-behind launches left the two columns behind the plane (rg_engine::cols_behind, rg_mirror.h),
// they are written back before the call does anything else -- on the stream the engine has at that moment -- and the packed
// streak ends (rg_mirror_host.h: RG_MC_DROP).
#define RG_ENTER(h)                                                                                \
    do {                                                                                           \
        const int src__ = rg_mirror_settle(h, RG_MC_DROP);                                         \
        if (src__) return src__;                                                                   \
        RG_ENTER_BASE(h);                                                                          \
    } while (0)
// ... and the entry points that start the NEXT step (device Inflights: nothing of it is enqueued while a host hint of the last
// one is unanswered)
#define RG_ENTER_STEP(h, who)                                                                      \
    do {                                                                                           \
        RG_ENTER(h);                                                                               \
        const int hrc__ = rg_require_hints_resolved(h, who);                                       \
        if (hrc__) return hrc__;                                                                   \
    } while (0)
// (a failed entry leaves the mirror dropped; the KEEP forms neither settle nor end a write-behind streak -- a KEEP call that
// reads match or committed_index settles by itself, rg_mirror_settle(h, RG_MC_KEEP_LOOK))
#define RG_ENTER_KEEP(h)                                                                           \
    do {                                                                                           \
        const bool mv__ = (h)->mirror_valid;                                                       \
        RG_ENTER_BASE(h);                                                                          \
        (h)->mirror_valid = mv__;                                                                  \
    } while (0)
#define RG_ENTER_STEP_KEEP(h, who)                                                                 \
    do {                                                                                           \
        const bool mv__ = (h)->mirror_valid;                                                       \
        RG_ENTER_BASE(h);                                                                          \
        const int hrc__ = rg_require_hints_resolved(h, who);                                       \
        if (hrc__) return hrc__;                                                                   \
        (h)->mirror_valid = mv__;                                                                  \
    } while (0)

// The one switch on the slot count: f(std::integral_constant<int, P>{}), for the launches templated on it that live in the ABI
// units (everything of tick_inst.hip goes through RgTickLaunch instead).
template <typename F> static inline auto rg_with_p(u32 P, F &&f) {
    switch (P) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    default: return f(std::integral_constant<int, 8>{});
    }
}

// rg_refresh_classes: per block of RG_BLOCK groups (= one workgroup of the lane kernels), the number of slots the block's cfg
// words name: 1 + the highest slot that is present, a voter of either majority, the leader's own, or the transferee.
RG_HD u32 rg_cfg_slots_named(u32 cfg) {
    const u32 tr = RG_CFG_TRANSFEREE(cfg);
    const u32 m = RG_CFG_PRESENT(cfg) | RG_CFG_INCOMING(cfg) | RG_CFG_OUTGOING(cfg) | (1u << RG_CFG_SELF(cfg)) | (tr ? 1u << (tr - 1u) : 0u);
    return 32u - (u32)__builtin_clz(m | 1u);
}
// the smallest body k_tick_classes<P> has for k slots (3, 5, 7 below P; P)
RG_HD u32 rg_class_body(u32 k, u32 P) { return (P > 3 && k <= 3) ? 3u : (P > 5 && k <= 5) ? 5u : (P > 7 && k <= 7) ? 7u : P; }

// ReadIndex (abi_read.hip; rg_permute_groups gathers the columns): the optional arena -- absent until rg_read_index_enable, like
// the entry-size windows of rg_log_sizes_enable -- and the list of read states.
struct RgReadEngine {
    RgReadCols cols;
    char *arena, *ckpt; // qw | qterm | ctx | idx | acks; the checkpoint copy (lazy)
    size_t bytes;
    size_t off_qterm, off_ctx, off_idx, off_acks;
    rg_read_state *items;      // the compact list of read states
    u64 cap;                   // ... its capacity, items
    unsigned long long *count; // device: states in the list
    // An upper bound of (states in the list + reads pending in the queues): every state answers exactly one request that was
    // accepted (READY or QUEUED), so the list cannot outgrow it -- the capacity is raised on the control path, before a request
    // call, and no kernel ever has to drop or to size per group for the worst case.
    u64 outstanding, ckpt_outstanding;
    std::vector<char> stage;   // host staging of one batch: RgReadRec[n] | u32 run_start[runs + 1] | u8 status[n]
    std::vector<RgReadRec> recs;
};

// The follower half (abi_follow.hip): the optional arena of the groups this store follows -- its own index space, absent until
// rg_follow_enable; no tick, flush, publication or rg_permute_groups touches it. It is built in layers, each absent (arena ==
// nullptr) until its enable call:
enum {
    RG_FL_LOG,   // rg_follow_enable: the columns of RgFollowCols, [stride] each
    RG_FL_SOFT,  // rg_follow_gate_enable (term gate, vote step, election clock): the columns of RgSoftCols, [stride] each, then --
                 // behind `bytes`, so no checkpoint carries them -- the two count words of rg_follow_clock
    RG_FL_ELECT, // rg_follow_elect_enable (the candidate half, abi_elect.hip): the columns of RgElectCols, [stride] each
    RG_FL_COUNT
};
struct RgFollowLayer {
    char *arena = nullptr, *ckpt = nullptr; // the columns; their checkpoint copy (lazy)
    size_t bytes = 0;                       // of the columns
};
struct RgFollowEngine {
    RgFollowLayer layer[RG_FL_COUNT];
    RgFollowCols cols{};
    RgSoftCols soft{};
    RgElectCols elect{};
    unsigned long long *clock_counts = nullptr; // device u64 [2]: groups appended, groups due
    std::vector<char> stage;                    // host staging of one sparse batch / one read
    std::vector<u32> order;                     // ... its records' positions, sorted by group
    std::vector<rg_follow_state> states;        // ... of one rg_follow_write
    std::vector<RgElectStaged> elect_recs;      // ... of one batch of election records
    bool has(int l) const { return layer[l].arena != nullptr; }
};

// The leader's clock (ext_lead.hip): the optional per-group cells of the LEADER engine -- absent until rgx_lead_clock_enable --, over
// the engine's stride; rg_permute_groups moves them with their groups.
struct RgLeadCols {
    u64 *tag;  // [stride] the RG_COL_CUR_TERM value the clock cell belongs to
    u32 *cell; // [stride] heartbeat_elapsed | election_elapsed << 14 | STOPPED << 31 (rg_lead.h)
    RgLeadCfg cfg;
};
struct RgLeadEngine {
    RgLeadCols cols{};
    char *arena = nullptr, *ckpt = nullptr; // tag | cell, then -- behind `bytes`, so no checkpoint carries them -- the four count words
    size_t bytes = 0;
    unsigned long long *counts = nullptr;   // device u64 [4]: beats, check-quorum runs, step-downs, transfers aborted
    std::vector<char> stage;                // host staging of one write / read
};

// The layout of rg_engine::d_counts, in u64 words. Each user clears its own words before it counts and nobody else's, so what a
// dense call left there stays until its next call.
enum {
    RG_COUNTS_REDUCE = 0, RG_COUNTS_REDUCE_N = 5, // the reductions of abi_tick.hip (the most: rg_msg_stats)
    RG_COUNTS_TERM = 8, RG_COUNTS_TERM_N = 3,     // rgt_lead_gate_device: groups deposed, stale records, records of groups not led
    RG_COUNTS_HINT = 16, RG_COUNTS_HINT_N = 1,    // rg_engine::d_hint_raised (a u32: the word's low half)
    RG_COUNTS_VOTE = 24, RG_COUNTS_VOTE_N = 6,    // rgv_follow_vote_device: requests, grants, rejects, ignored, deposed; the answered list's cursor
    RG_COUNTS_WORDS = 32                          // what rg_create sets aside
};
static_assert(RG_COUNTS_REDUCE + RG_COUNTS_REDUCE_N <= RG_COUNTS_TERM && RG_COUNTS_TERM + RG_COUNTS_TERM_N <= RG_COUNTS_HINT &&
                  RG_COUNTS_HINT + RG_COUNTS_HINT_N <= RG_COUNTS_VOTE && RG_COUNTS_VOTE + RG_COUNTS_VOTE_N <= RG_COUNTS_WORDS,
              "the users of d_counts overlap");

// ------------------------------------------------------------------------------------------------
// engine object
// ------------------------------------------------------------------------------------------------
struct rg_engine {
    rg_config cfg;
    rg_device_info dev;
    u64 G, stride;
    u32 P;
    const RgTickLaunch *launch; // the launchers of the kernels instantiated for P slots (rg_tick_launch)
    hipStream_t stream;
    char *arena;      // state columns
    size_t state_bytes;
    char *ckpt;       // checkpoint copy of the state columns (lazy)
    char *msg_arena;  // device staging for rg_tick(host msgs) / rg_flush (lazy)
    u64 *zero_col;    // [P][stride] zeros, substituted for NULL m_hint / m_rs
    u64 *rhint;       // [P][stride] reject hints after find_conflict_by_term (pre-pass output)
    u64 *d_counts;    // scratch for reductions and the dense calls' count words: RG_COUNTS_WORDS x u64, laid out by the RG_COUNTS_* enum above
    void *d_scratch;  // G x 8 B scratch for host<->device result shuttles
    size_t col_off[RG_COL_COUNT];
    RgState st;
    RgMsgs staged;    // views into msg_arena
    bool ticked;
    // commit publication: the slot b whose ev_tick[b] rode on the dispatch packet of the LAST dense tick (rg_tick_impl), -1 if
    // none or if any entry point has run since (RG_ENTER): rg_publish_commit right behind that tick need not record an event
    int pub_tick_evt;
    u64 tick_launches; // ticks enqueued so far (rg_flush: did a failed flush already change device state?)
    // sparse path (rg_ingest / rg_tick_ingested)
    char *sparse_arena;       // gmark | list | res_list | res_commit | res_out | counters
    u32 *gmark, *counters, *counters_base, *res_out;
    u64 *list, *res_list, *res_commit;
    // single-sync flush of the host mirror: pinned staging for the records, one packed D2H copy of the results
    rg_wire_msg *pin_records; // hipHostMalloc
    u64 pin_records_cap;
    char *d_packed, *pin_packed; // device / pinned host: header + rg_res_rec[]
    u64 packed_cap;           // records
    std::vector<u64> host_res_groups, host_res_commit;
    std::vector<u32> host_res_out;
    bool host_res_valid;      // the vectors hold the results of the last tick (served by rg_ingested_results)
    rg_cell_write *d_cells;   // device staging for rg_write_cells
    u64 d_cells_cap;
    rg_wire_msg *d_records;   // device staging for records
    u64 d_records_cap;
    u32 epoch;
    u64 ingested_upper;       // records accepted for upload since the last sparse tick (>= touched groups)
    u64 last_sparse_n;        // groups of the last rg_tick_ingested (result arrays are valid for them)
    bool out_is_dense;        // RG_COL_OUT was last written by a dense tick
    // send stage (rg_config.max_inflight > 0): Inflights rings, work items
    char *ins_arena;   // meta | head | tail | ring | items | counter
    char *ins_ckpt;    // checkpoint copy of meta | ring (lazy)
    u32 *esz, *esz_ckpt; // entry sizes for RG_SEND_BYTES (rg_log_sizes_enable), u32 [G][esz_w]; checkpoint copy (lazy)
    struct RgReadEngine *rd; // ReadIndex: pending-read queues and the list of read states (rg_read_index_enable), nullptr = off
    struct RgFollowEngine *fo; // the follower half: the followed groups' log summaries (rg_follow_enable), nullptr = off
    struct RgLeadEngine *ld;   // the leader's clock (rgx_lead_clock_enable), nullptr = off
    void *d_recs;      // staging for rg_log_sizes_write / rg_update_state / rg_read_index / rg_follow_* records
    size_t d_recs_cap;
    // resident small-batch path (rg_mailbox_start): request / answer block in pinned host memory, whether the feature is
    // on, whether the host has launched an instance it has not seen leave, the last request number
    RgMbox *mbox;
    bool mbox_on, mbox_running;
    u32 mbox_seq;
    u64 mbox_idle_ticks;
    u64 mbox_served, mbox_launches; // flushes the resident workgroup answered / times it was (re)launched
    size_t ins_state_bytes;
    RgIns ins;
    rg_send_item *send_items;
    u32 *send_counter;
    RgSendCols send_cols;  // work items of a dense stage (peer-major columns)
    bool send_cols_fresh;  // ... hold the last stage's items and the compact list has not been materialised from them
    bool send_last_dense;  // the last stage was a dense one (the columns are its output)
    u64 send_bound;    // upper bound of the last stage's work items (groups it walked x peers)
    std::vector<rg_send_item> host_items; // items of the last stage when rg_flush_send fetched them
    bool host_items_valid;
    char *pin_send;    // pinned host: u32 count | pad | rg_send_item[RG_SEND_SPEC] (small stages: one round trip)
    // size classes (k_tick_classes): derived from RG_COL_CFG, lazily, by the first dense tick after anything wrote the column
    u8 *cls_need;      // device: one byte per block of RG_BLOCK groups (k_block_slots), padded to whole words
    std::vector<u8> cls_host; // its host copy
    bool cls_on;       // some block names fewer slots than the engine has: the dense lane tick runs k_tick_classes
    u32 *cls_order;    // device: one word per workgroup of that kernel, in launch order: block | slots << 28 (RgClasses::order)
    bool cls_stale;    // RG_COL_CFG may have changed since the bytes were derived
    bool cls_off;      // never use them: RG_CFGF_NO_SIZE_CLASSES at rg_create, or the cfg column's device pointer was handed out
    bool nt_msgs;      // dense ticks stream their message columns (non-temporal loads): state + one tick's messages > Infinity Cache
    bool nt_all;       // ... and the state columns, loads and stores: the state ALONE is far beyond the cache
    u64 nt_resident;   // ... except those of the first nt_resident workgroups' groups, which stay in the cache (k_tick_split); 0 = off
    bool counted_live;   // this engine is in g_live_on_device
    bool cls_block_order; // RG_CFGF_CLASS_BLOCK_ORDER
    bool hint_check_due; // device Inflights: a tick that may have raised RG_OUT_HOST_HINT (it carried log terms) ran and nobody has
                         // verified since that every hint was resolved (rg_require_hints_resolved)
    // ... and what makes that check free for the ticks that raised none: the pre-pass of a dense log-term tick ORs 1 into
    // d_hint_raised when it leaves a reject to the host; the word is copied to pinned memory behind the pre-pass (BEFORE the
    // tick kernel) and ev_hint recorded, so the next entry point waits for the pre-pass only, never for the tick
    u32 *d_hint_raised, *pin_hint_raised;
    hipEvent_t ev_hint;
    u32 fused_done;          // ticks the last rg_tick_device_fused applied (rg_fused_ticks_done)
    bool hint_probe_pending; // the last log-term tick went through the probe and nobody has looked at its word yet
    bool send_ready;   // a tick ran since the last rg_send_appends
    u64 stage_max_entries; // limit and flags of the last send stage (any form): rg_resolve_host_hints runs the stage of the
    u32 stage_flags;       // groups that stage skipped (RG_OUT_HOST_HINT) with the same ones
    bool ckpt_send_ready;
    bool ckpt_hint_check_due;
    bool ckpt_any_group_commit;
    bool any_group_commit; // some group's cfg word has RG_CFG_GROUP_COMMIT (tracked on cfg loads)
    // host mirror of RawNode::step (rg_set_peers / rg_step / rg_flush)
    std::vector<u64> peer_ids; // [G][8], 0 = unused
    std::vector<u64> terms;    // [G]
    std::vector<u64> q_mi, q_mc, q_mh, q_mrs, q_mlt; // [P][stride] host queues
    std::vector<u8> q_mf;                      // [G][8]
    std::vector<u64> q_dirty;                  // groups touched since the last flush
    bool q_any_logterm;                        // some queued message carries Message.log_term
    struct RgQueuedElection { u64 group, old_term; };
    std::vector<RgQueuedElection> q_elections; // rg_local_become_leader calls of the pending flush: group, the term its gate had
    std::vector<u32> host_cfg;                 // host copy of RG_COL_CFG for the mirror (self slots)
    bool host_cfg_valid;
    bool host_mirror;
    struct RgPub *pub; // commit publication across ranks (rg_comm_init), nullptr = single engine
    // the read mirror of the dense lane tick (rg_mirror.h, k_tick_mirror): engine-internal, no RG_COL_*, in no checkpoint
    u32 *mirror;        // device: [P][stride] packed words; nullptr = this engine keeps none (rg_create: not the lane variant, 64-bit
                        // cell offsets, device Inflights, RG_CFGF_NO_READ_MIRROR)
    bool mirror_valid;  // the plane describes RG_COL_MATCH / RG_COL_PR_COMMIT / RG_COL_COMMIT as they stand: set by the dense tick
                        // that wrote it, cleared by every other entry (RG_ENTER)
    bool cols_behind;   // write-behind launches have run since the last settle: in the blocks whose words hold no escape the plane IS
                        // the state and the two columns are stale (rg_mirror_host.h: RgMirrorHost::behind)
    u32 mirror_streak;  // packed write-through launches since the last build launch or settle point (RgMirrorHost::streak)
    bool mirror_off;    // for good: somebody can write those columns without an entry point -- rg_column_ptr handed one of them out,
                        // or a tick was captured into a graph, which replays it behind the engine's back
    // escapes, watched without a synchronisation (rg_mirror.h: RgMirrorEsc): the device's running count of waves that stored an
    // escape, its copy in pinned host memory, and the window rg_plan_tick compares it over
    RgMirrorEsc mirror_esc;
    u32 mirror_win_base, mirror_win_launches;
    bool mirror_escaping; // too many waves escape: k_tick_lane for good (rgr_mirror_info.off = 2)
    u64 mirror_packed, mirror_build; // launches of k_tick_mirror that read the plane / that (re)built it (rgr_mirror_stats)
};

// RCCL is bound lazily (the library is ~0.5 GB; single-GPU users never load it). The types come from its header.

#include <rccl/rccl.h>

// Send slices in rotation: the ticks of interval i accumulate into slice i % RG_PUB_SEND while the exchanges of the
// previous intervals still read theirs. Re-use is gated on the HOST (hipEventSynchronize on the exchange that last
// read the slice, three publications back: normally long finished), so the engine's stream carries no cross-stream
// wait -- a barrier packet per tick costs ~5 us of a ~58 us tick (profiles/r02_publish_overhead.txt).
#define RG_PUB_SEND 4
struct RgPub {
    u32 rank, world;
    ncclComm_t comm;          // RCCL transport (nullptr with a custom transport)
    rg_allgather_fn transport;
    void *transport_user;
    RgPubLayout lay;
    u32 ring;                 // publications buffered before the replica is brought up to date
    hipStream_t side;         // the exchange runs here; the engine's stream only records / waits events
    char *send[RG_PUB_SEND];  // this rank's slice under construction (a small ring), bytes_per_rank each
    char *ring_buf;           // [ring][world][bytes_per_rank]
    u64 *replica;             // [world][Gpad]
    u64 *full_send;           // [Gpad] snapshot of the commit column for a full publication
    u32 *d_lost;              // device: some gathered slice asked for a resynchronisation (set by the replica update)
    u32 *pin_lost;            // pinned host: [2] copies of d_lost taken at the last two check points
    hipEvent_t ev_tick[RG_PUB_SEND], ev_done[RG_PUB_SEND], ev_chk[2];
    bool done_pending[RG_PUB_SEND], chk_pending[2];
    u64 n_pub;                // publications so far
    int rode_slot;            // rg_publish_commit: the engine's pub_tick_evt as the call found it (-1: record the event)
    u32 pending;              // ring slots gathered and not yet folded into the replica
    bool in_process;          // one of several ranks of ONE process driven by one thread (rg_comm_init_all / rg_publish_commit_all)
    hipEvent_t ev_read;       // ... in-process transport: this rank's side stream has read every rank's slice of the current publication
    bool local_lost;          // this rank's deltas no longer describe its commit column (restore / column load)
    bool lost_announced;      // ... and a slice carrying RG_PUB_LOST has gone out (the full snapshot follows)
    rg_publish_stats stats;
};

static inline size_t rg_col_elem(int c) {
    if (c == RG_COL_PFLAGS) return 8; // one u64 row per group
    if (c == RG_COL_CFG || c == RG_COL_OUT) return 4;
    if (c == RG_COL_HOST_HINT || c == RG_COL_RUN_COUNT) return 1;
    return 8;
}
static inline bool rg_col_per_slot(int c) { return c <= RG_COL_GID; }
static inline bool rg_col_per_run(int c) { return c == RG_COL_RUN_FIRST || c == RG_COL_RUN_TERM; }

#define RG_STR2(x) #x
#define RG_STR(x) RG_STR2(x)
static inline void *rg_col(rg_engine *h, int c) { return h->arena + h->col_off[c]; }
static inline unsigned rg_grid(u64 n, unsigned per_block) { return (unsigned)((n + per_block - 1) / per_block); }

// rg_grow.h over HIP: a device or a pinned host staging buffer of the engine; the stream is drained before an old one goes
static inline hipError_t rg_dev_alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
static inline hipError_t rg_pin_alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
static inline void rg_dev_free(void *p) { (void)hipFree(p); }
static inline void rg_pin_free(void *p) { (void)hipHostFree(p); }
template <typename T> static inline hipError_t rg_grow_dev(rg_engine *h, T **ptr, u64 *cap, u64 need, u64 first, size_t elem, size_t pad = 0) {
    return rg_grow(ptr, cap, need, first, elem, pad, rg_dev_alloc, rg_dev_free, [h] { return hipStreamSynchronize(h->stream); });
}
template <typename T> static inline hipError_t rg_grow_pin(rg_engine *h, T **ptr, u64 *cap, u64 need, u64 first, size_t elem, size_t pad = 0) {
    return rg_grow(ptr, cap, need, first, elem, pad, rg_pin_alloc, rg_pin_free, [h] { return hipStreamSynchronize(h->stream); });
}

#define RG_SEND_SPEC 16384 /* work items copied speculatively with their count (512 KB of pinned memory) */
struct RgSendReq { // a tick or a flush that runs its send stage with it (rg_tick_send, rg_tick_device_send, rg_flush_send)
    u64 max_entries;
    u32 flags;
};

// ---- internal functions one unit provides to the others (hidden visibility: not part of the ABI) ----
// abi_state.hip
void rg_drop(rg_engine *h);
// abi_tick.hip
int rg_settle_send(rg_engine *h);
int rg_refresh_classes(rg_engine *h);
int rg_tick_impl(rg_engine *h, const RgMsgs &ms, const RgSendReq *send = nullptr);
int rg_send_check(rg_engine *h, uint32_t flags, const char *who);
int rg_ensure_msg_arena(rg_engine *h);
int rg_tick_host_impl(rg_engine *h, const rg_msgs *m, const RgSendReq *send);
// abi_send.hip
int rg_send_enqueue(rg_engine *h, uint64_t max_entries_per_msg, uint32_t flags, const u64 *list, u64 n, const u32 *n_ptr);
int rg_stage_records(rg_engine *h, const void *recs, size_t bytes);
int rg_stage_reserve(rg_engine *h, size_t bytes);
int rg_send_materialize(rg_engine *h);
int rg_ensure_pin_send(rg_engine *h);
void rg_list_stage_ran(rg_engine *h, u64 max_entries, u32 flags);
int rg_fix_ins_full(rg_engine *h); // k_fix_ins_full over every group, on the engine's stream
// abi_mirror.hip
int rg_ensure_sparse(rg_engine *h);
// abi_publish.hip
int rg_rccl_load();
// abi_read.hip: the optional ReadIndex arena in the calls that handle every arena (all of them no-ops while it is absent)
void rg_read_free(rg_engine *h);
int rg_read_checkpoint(rg_engine *h);
int rg_read_restore(rg_engine *h);
// abi_follow.hip: the same for the optional follower arena
void rg_follow_free(rg_engine *h);
int rg_follow_checkpoint(rg_engine *h);
int rg_follow_restore(rg_engine *h);
// ext_lead.hip: the same for the optional leader clock; rg_lead_place moves the cells with their groups (rg_permute_groups: d_perm
// is the device copy of the permutation, tmp a device buffer of ld->bytes the caller allocated before anything moved)
void rg_lead_free(rg_engine *h);
int rg_lead_checkpoint(rg_engine *h);
int rg_lead_restore(rg_engine *h);
hipError_t rg_lead_place(rg_engine *h, const u64 *d_perm, char *tmp);
// ... one layer of it: `total` bytes (>= `bytes`, the part a checkpoint carries) allocated and cleared on the engine's stream. The
// caller finishes with rg_follow_layer_drop (its init kernel did not launch) or adds `total` to engine_bytes.
int rg_follow_layer_alloc(rg_engine *h, const char *who, RgFollowLayer *l, size_t bytes, size_t total);
void rg_follow_layer_drop(RgFollowLayer *l);
// ... and the round trip of every sparse call of the follower side, in this order: `bytes` at `src` staged (rg_stage_records),
// launch(device base of the staging), the launch check under `who`, the D2H copies of `fetch` in the order given (a null
// destination is skipped), one hipStreamSynchronize -- the staging is reused by the next call.
struct RgFetch {
    void *dst;
    size_t off, bytes; // device offset in the staging
};
int rg_follow_round_trip(rg_engine *h, const char *who, const void *src, size_t bytes, const std::function<void(char *)> &launch,
                         std::initializer_list<RgFetch> fetch = {});

// What follows a kernel launch of the follower side: 0, or the failure "<who>: launch failed: <HIP's text>".
static inline int rg_launch_check(const char *who) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? RG_OK : rg_fail(RG_ERR_NO_DEVICE, "%s: launch failed: %s", who, hipGetErrorString(e));
}

// "No group twice" in the walk of a sparse call's records (one walk in array order: range, rule, then this, so of several faults
// the first record's is reported): ins = seen.emplace(group, i) -> 0, or the failure naming the record that had the group first.
typedef std::unordered_map<u64, u64> RgSeen;
static inline int rg_named_once(const char *who, const std::pair<RgSeen::iterator, bool> &ins, u64 i) {
    if (ins.second) return RG_OK;
    return rg_fail(RG_ERR_INVALID_ARG, "%s: records %llu and %llu name group %llu", who, (unsigned long long)ins.first->second, (unsigned long long)i,
                   (unsigned long long)ins.first->first);
}

// Groups in, records out (rg_follow_read, rg_follow_soft_read, rg_follow_elect_read): launch(device groups, device records).
template <typename Rec, typename Launch> static inline int rg_follow_gather(rg_engine *h, const char *who, const u64 *host_groups, u64 n, Rec *host_out, Launch launch) {
    RgFollowEngine *fo = h->fo;
    for (u64 i = 0; i < n; i++)
        if (host_groups[i] >= fo->cols.n)
            return rg_fail(RG_ERR_INVALID_ARG, "%s: group %llu of %llu", who, (unsigned long long)host_groups[i], (unsigned long long)fo->cols.n);
    if (n == 0) return RG_OK;
    RG_ENTER(h);
    RgLayout lay;
    lay.add(n * 8);
    const size_t off_out = lay.add(n * sizeof(Rec));
    fo->stage.assign(lay.total, 0);
    memcpy(fo->stage.data(), host_groups, n * 8);
    return rg_follow_round_trip(h, who, fo->stage.data(), fo->stage.size(),
                                [&](char *d) { launch(reinterpret_cast<const u64 *>(d), reinterpret_cast<Rec *>(d + off_out)); },
                                {{host_out, off_out, n * sizeof(Rec)}});
}

