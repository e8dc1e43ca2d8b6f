/* raftgroups_handoff.h -- the promotion into an engine with device Inflights (rg_config.max_inflight > 0): a followed group that won
 * its election becomes a group of the leader engine, its Inflights windows are emptied and its first appends are decided, in ONE
 * launch. A FOURTH extension of include/raftgroups.h, beside raftgroups_lead.h, raftgroups_term.h and raftgroups_vote.h and in a
 * header of its own; it needs the core header only.
 *
 * The four older headers stay as they are: their entry points, struct layouts, RG_ABI_VERSION, RGX_LEAD_VERSION, RGT_TERM_VERSION
 * and RGV_VOTE_VERSION are unchanged, and a caller that does not include this file sees the same library as before. The entry points
 * declared here carry the prefix rgh_; the types and constants are rgh_ / RGH_ too. RGH_HANDOFF_VERSION is bumped whenever a layout
 * or a signature of THIS file changes; rgh_handoff_version() returns what the library was built with. Same rules as raftgroups.h
 * otherwise: C99, no exception leaves an entry point, int results are RG_OK or an RG_ERR_* code with the text in rg_last_error().
 *
 * This header SUPERSEDES, for callers who include it, the note of raftgroups.h ("The hand-off") that on an engine created with
 * max_inflight > 0 "emptying device Inflights windows outside a tick is deliberately left out (such a store takes the host route:
 * rg_follow_read, rg_load_column, RG_MF_BECOME_LEADER in a tick, whose send stage empties the windows)". rg_follow_promote and
 * rg_follow_promote_device still answer RG_ERR_STATE there; the two calls below are the promotion of such an engine, and they answer
 * RG_ERR_STATE on an engine WITHOUT device Inflights (rg_follow_promote* is its promotion). The per-tick loop of a store with device
 * Inflights becomes
 *     rg_follow_clock, rg_follow_campaign_device, rg_follow_vote_resps_device, rgh_follow_promote_device, rg_tick_device_send
 * with no group's state crossing to the host at an election.
 * Citations are relative to the pingcap/raft-rs v0.6.0 tree. */
#ifndef RAFTGROUPS_HANDOFF_H
#define RAFTGROUPS_HANDOFF_H
#include "raftgroups.h"
#ifdef __cplusplus
extern "C" {
#endif

#define RGH_HANDOFF_VERSION 1u
uint32_t rgh_handoff_version(void); /* RGH_HANDOFF_VERSION of the build */

/* ---- Per record (sparse) or per followed group with dev_result[g] == RG_ELECT_WON (dense), all-or-nothing per group ----
 * 1. THE PROMOTION, exactly rg_follow_promote*'s (raftgroups.h, "The hand-off"): the same refusals in the same order (NOT_WON, CONF,
 *    NOT_PERSISTED, FAULT; the dense form also FAULT for a lead group at or beyond n_groups), the same log import, become_leader and
 *    Progress reset, the same answer {term = T, last_index, commit, out = RG_OUT_BECAME_LEADER | RG_OUT_APPENDED}. Every status but
 *    DONE leaves every cell of both sides, every window and the item list as they were.
 * 2. THE WINDOWS. Raft::reset empties every Progress's Inflights (ins.reset(), src/tracker/progress.rs:82-92): the window of every
 *    slot in RG_CFG_PRESENT of the lead group (below the engine's slot count, the own slot included) becomes empty, whatever an
 *    earlier leadership left there -- empty, compact, ring, wrapped or full. Slots without a Progress keep their cells.
 * 3. THE FIRST APPENDS: the bcast_append that follows become_leader (src/raft.rs:2190-2191), decided as the send stage decides it for
 *    a group whose result word is RG_OUT_BECAME_LEADER | RG_OUT_APPENDED. max_entries_per_msg and flags are those of rg_send_appends
 *    (RG_SEND_SKIP_BCAST_COMMIT, RG_SEND_BYTES) and are checked like them. Every peer was reset to Probe with next = the index of
 *    the empty entry, so each gets ONE message that carries that one entry -- no limit can split a single entry, and
 *    util::limit_size keeps the first entry whatever its size (src/util.rs:52-76) -- and Progress::update_state pauses it
 *    (progress.rs:231-243), applied in place: the peers end up Probe and RG_PF_PAUSED. One work item per peer that gets a message:
 *    {group = the lead group, slot, prev_index = last_index - 1, last_index, n_msgs = 1, kind = RG_SEND_APPEND}. Learners get one;
 *    the own slot and absent slots do not.
 * 4. THE EMPTY ENTRY'S SIZE RECORD, only on an engine with rg_log_sizes_enable: with hi = the new last_index, T the term and w the
 *    window,  esz[L][hi & (w - 1)] = esz[L][(hi - 1) & (w - 1)] + Entry::compute_size({term T, index hi}),  the size being
 *    (T ? 1 + varint_len(T) : 0) + (hi ? 1 + varint_len(hi) : 0) -- what rg_entry_size answers for that entry. Written before anything
 *    reads it. This closes the hole raftgroups.h describes at rg_log_sizes_*: a host that does not know last_index cannot write the
 *    record of the entry become_leader appends in time. The records of OLDER entries stay the host's duty: the cell the sum starts
 *    from is read as it stands, and a later stage that reaches behind the empty entry needs the records rg_log_sizes_write owes.
 *
 * WHERE THE ITEMS GO: to the CALLER's memory, not to the engine's work-item list or item columns. The engine's send-stage
 * bookkeeping is not touched -- rg_send_items, rg_send_columns and rg_send_tail_column return for every other group what they
 * returned before the call, and the limit and flags of the last stage stay those rg_resolve_host_hints uses. RG_COL_OUT and
 * RG_COL_HOST_HINT are not written. *n_items / *count is the TOTAL number of items; only item_cap of them are written (the rule of
 * rg_send_items), nothing beyond item_cap is touched; item order is unspecified.
 *
 * COST. The dense form reads one byte and writes one byte per followed group that is not selected; a promoted group moves the
 * promotion's ~485 B plus 4 B per window and 32 B per item. profiles/promote_send.txt (1 M x 3 groups, max_inflight 8, one MI355X):
 * against the host route's 3.8 / 3.9 / 17 / 213 ms for 1 / 1 000 / 65 536 / 1 M promoted groups the dense form takes 10 / 20 / 116 /
 * 113 us and the sparse form 66 us / 143 us / 4.4 ms / 110 ms -- both ahead at every K, the sparse form by only 1.9 x at 1 M, where its
 * host-side record walk, staging and item copy dominate. */

/* The sparse form: staged like rg_follow_promote, synchronises, answers per record. host_items may be NULL when item_cap is 0.
 * RG_ERR_INVALID_ARG, and nothing applied, for a follow group at or beyond n_follow, a lead group at or beyond n_groups, or two
 * records naming the same follow group or the same lead group. On an engine with a host mirror (rg_set_peers) it keeps
 * rg_follow_promote's rules: RG_ERR_SLOT_BUSY for a lead group with queued mirror events, and T registered as the group's term after
 * a DONE. */
int rgh_follow_promote(rg_engine *h, const rg_handoff_rec *host_recs, uint64_t n, rg_handoff_resp *host_resp,
                       uint64_t max_entries_per_msg, uint32_t flags,
                       rg_send_item *host_items, uint64_t item_cap, uint64_t *n_items);

/* The dense form: dev_result / dev_lead / dev_persisted and out as rg_follow_promote_device's (dev_persisted may be NULL: the host
 * vouches that persisted == last_index; CONTRACT: the selected groups name pairwise different lead groups). *count is zeroed on the
 * engine's stream before the launch; items may be NULL when item_cap is 0. Asynchronous: a tick queued after the call sees the new
 * leader and its paused peers. RG_ERR_STATE on an engine with a host mirror (the sparse form serves it). */
typedef struct {
    rg_handoff_out out;
    rg_send_item *items;
    uint64_t item_cap;
    uint32_t *count;
} rgh_promote_out; /* all DEVICE memory */
int rgh_follow_promote_device(rg_engine *h, const uint8_t *dev_result, const uint64_t *dev_lead, const uint64_t *dev_persisted,
                              uint64_t max_entries_per_msg, uint32_t flags, const rgh_promote_out *dev_out);

/* State rules, all checked on the host before anything is staged or launched. RG_ERR_STATE: the engine has no device Inflights
 * (rg_follow_promote* is its promotion); rg_follow_elect_enable has not run; a tick's send stage is still owed (rg_send_appends, or
 * the next tick settles it: its result words still describe the windows); groups still carry RG_OUT_HOST_HINT
 * (rg_resolve_host_hints); RG_SEND_BYTES without rg_log_sizes_enable; the dense form on an engine with a host mirror.
 * RG_ERR_INVALID_ARG: unknown flags, a required pointer that is NULL, a bad record (above). With commit publication on, a call
 * counts as a reloaded commit column, as rg_follow_promote* does. The calls keep no state: checkpoint, restore and rg_permute_groups
 * need nothing. */

#ifdef __cplusplus
}
#endif
#endif /* RAFTGROUPS_HANDOFF_H */
