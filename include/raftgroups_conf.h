/* raftgroups_conf.h -- the batched conf change: what follows the validation of a membership change -- ProgressTracker::apply_conf
 * (src/tracker.rs:380-397) and Raft::post_conf_change (src/raft.rs:2604-2673) -- for many led groups in ONE launch. A FIFTH extension
 * of include/raftgroups.h, beside raftgroups_lead.h, raftgroups_term.h, raftgroups_vote.h and raftgroups_handoff.h and in a header
 * of its own; it needs the core header only.
 *
 * The five older headers stay as they are: their entry points, struct layouts and versions are unchanged, and a caller that does
 * not include this file sees the same library as before. The entry points declared here carry the prefix rgc_; the types and
 * constants are rgc_ / RGC_ too. RGC_CONF_VERSION is bumped whenever a layout or a signature of THIS file changes;
 * rgc_conf_version() returns what the library was built with. Same rules as raftgroups.h otherwise: C99, no exception leaves an
 * entry point, int results are RG_OK or an RG_ERR_* code with the text in rg_last_error().
 *
 * WHY. rg_set_config writes the WHOLE cfg word of ONE group and synchronises; but the TRANSFEREE bits of that word are cleared on
 * the device (rgx_lead_clock at a step-down, rgt_* at a deposition, rgv_* at a deposing vote) and SELF and GROUP_COMMIT are engine
 * state, so a host that does not know a group's term has to read the word back before it can write it again -- and a store that
 * joins or leaves changes every group that has a replica on it, twice through joint consensus. The calls below take the three
 * membership fields only and keep the others as the device holds them. rg_set_config keeps its behaviour and stays the road of an
 * engine with a host mirror and of a change that removes the leader's own Progress.
 *
 * Changer::{simple, enter_joint, leave_joint} and its invariants (src/confchange/changer.rs) stay on the host: they are
 * control-plane work over ids. What the device checks of them is what it needs to stay in bounds and consistent (FAULT below).
 * Citations are relative to the pingcap/raft-rs v0.6.0 tree. */
#ifndef RAFTGROUPS_CONF_H
#define RAFTGROUPS_CONF_H
#include "raftgroups.h"
#ifdef __cplusplus
extern "C" {
#endif

#define RGC_CONF_VERSION 1u
uint32_t rgc_conf_version(void); /* RGC_CONF_VERSION of the build */

/* status */
#define RGC_CONF_NONE 0u    /* the dense form: the group was not selected */
#define RGC_CONF_DONE 1u    /* applied: apply_conf, maybe_commit, the sends, the transfer check */
#define RGC_CONF_DEMOTED 2u /* apply_conf only: the leader is no voter of the new configuration */
#define RGC_CONF_NOT_LED 3u /* refused: the group is not led (the leader's clock is enabled and says so) */
#define RGC_CONF_HOST 4u    /* refused: the change removes the leader's own Progress; rg_set_config is its road */
#define RGC_CONF_FAULT 5u   /* refused: a malformed word */
/* events */
#define RGC_CONF_EV_COMMITTED 0x1u        /* maybe_commit on the new configuration advanced the commit index */
#define RGC_CONF_EV_TRANSFER_ABORTED 0x2u /* the transferee is no voter any more: abort_leader_transfer (raft.rs:2666-2671) */

/* cfg = RG_CFG_MAKE(incoming, outgoing, 0, 0, 0, present): ONLY these three fields; every other bit 0 */
typedef struct {
    uint64_t group;
    uint32_t cfg;
    uint32_t reserved; /* 0 */
} rgc_conf_rec;

typedef struct {
    uint64_t commit, last_index;
    uint32_t cfg;     /* the word now in RG_COL_CFG (unchanged on a refusal) */
    uint32_t out;     /* RG_OUT_CHANGED or 0 */
    uint32_t n_items; /* work items of this group (counted whether or not item_cap had room for them) */
    uint8_t status, events, added, removed; /* RGC_CONF_*, RGC_CONF_EV_*; slot masks: Progresses created / dropped */
} rgc_conf_resp;

/* ---- Per selected group, all or nothing ----
 * Let W be the record's word, old = RG_COL_CFG[g], self = RG_CFG_SELF(old), hi = last_index. Refusals come in this order, and each
 * leaves every cell, every window and the item list as it was:
 *   1. FAULT: W has a bit outside the three fields; a mask names a slot >= the engine's slot count; incoming == 0;
 *      (incoming | outgoing) is not inside present (check_invariants, changer.rs:285-355: every voter has a Progress); self is not in
 *      RG_CFG_PRESENT(old).
 *   2. NOT_LED: rgx_lead_clock_enable has run and the group is not led -- the test the term gate uses (the clock's STOPPED bit under
 *      a tag equal to RG_COL_CUR_TERM). A stepped-down group's leader columns are without meaning and its membership is the follower
 *      arena's business. Without the clock layer every group of the engine is led.
 *   3. HOST: self is not in W's present. Removing the leader's own Progress stays the host's road (rg_set_config): the tick's
 *      self-slot rules assume that Progress.
 * Then:
 *   apply_conf (tracker.rs:380-397). added = Wp & ~oldp, removed = oldp & ~Wp. Every added slot becomes Progress::new(hi + 1) with
 *      recent_active = true: match 0, next hi + 1, committed_index, pending_snapshot, pending_request_snapshot and commit_group_id 0,
 *      flag byte exactly RG_STATE_PROBE | RG_PF_RECENT_ACTIVE, and on an engine with device Inflights an empty window. A slot in both
 *      keeps every cell whatever happened to its role (a learner promoted to voter is not reset); a removed slot keeps its cells and
 *      window, which are without meaning until it is added again. The new word is W's three fields plus old SELF, GROUP_COMMIT and
 *      TRANSFEREE.
 *   DEMOTED: self is in present but in neither majority (raft.rs:2609-2622): only apply_conf is stored -- no commit, no sends, no
 *      transfer abort, because the reference returns before them.
 *   maybe_commit on the new configuration (raft.rs:2630), as rg_recompute does it for one group: absent voters ack 0, joint quorums,
 *      group commit; the own slot's committed_index is raised, the publication byte is kept when commit publication is on. If it
 *      advanced: RGC_CONF_EV_COMMITTED and out = RG_OUT_CHANGED.
 *   the sends (engines with max_inflight > 0 only): every slot of W's present but self, in slot order, gets ONE call of
 *      maybe_send_append(to, allow_empty) (raft.rs:773-819) with allow_empty = COMMITTED: with it the bcast_append of raft.rs:2633,
 *      without it the probe of :2634-2646. The bcast_append is unconditional here (the reference does not ask should_bcast_commit()
 *      at this place): RG_SEND_SKIP_BCAST_COMMIT is accepted and has NO effect. One call, never the `while` loop of the send stage:
 *      n_msgs <= 1 (the two differ only for a peer that a limit splits; the next stage sends the rest). is_paused, a pending snapshot
 *      request first, Compacted (a snapshot with allow_empty, nothing without), max_entries_per_msg / RG_SEND_BYTES and RG_SEND_HOST
 *      are the send stage's (rg_send_appends). Progress::update_state(last) is applied in place: Replicate does next = last + 1 and
 *      ins.add(last), Probe sets paused; RG_PF_INS_FULL is kept exact.
 *   the transfer: if RG_CFG_TRANSFEREE(old) names a slot that is no voter of W, the bits are cleared and
 *      RGC_CONF_EV_TRANSFER_ABORTED is set (raft.rs:2666-2671).
 * NOT folded in: the ReadIndex re-check of raft.rs:2648-2664 (a smaller quorum may release pending reads). A read-ack call with
 * RG_READ_ACK_LAST_SELF (rg_read_acks), for the groups whose status is DONE, after this call, does it.
 *
 * WHERE THE ITEMS GO: to the CALLER's memory, by the rule of rgh_* (raftgroups_handoff.h): *n_items / *count is the TOTAL, only
 * item_cap items are written, nothing beyond item_cap is touched, item order is unspecified. The engine's own item list, item
 * columns, RG_COL_OUT and RG_COL_HOST_HINT are not touched. On an engine WITHOUT device Inflights the item arguments must be NULL / 0:
 * the host sends from `events`, as it does after rg_recompute today.
 *
 * COST. The dense form reads one byte and writes one byte per group that is not selected. profiles/conf_change.txt (1 M x 5 groups, K
 * of them alternately removing and adding back one voter per call, one MI355X; the host route is rg_read_groups, rg_set_config per
 * group, rg_write_cells for the added peers and rg_recompute, its 1 M figure EXTRAPOLATED from 65 536): for K = 1 / 1 000 / 65 536 /
 * 1 M the route takes 66 us / 14.0 ms / 898 ms / 13.7 s (extrapolated) with max_inflight 0 and 79 us / 13.9 ms / 883 ms / 13.5 s
 * (extrapolated) with max_inflight 8; the sparse form 49 us / 96 us / 2.4 ms / 61 ms and 50 us / 109 us / 2.4 ms / 55 ms; the dense
 * form 6.9 / 11.5 / 26 / 27 us and 8.6 / 20 / 57 / 58 us. */

/* The sparse form: staged, synchronises, answers per record. RG_ERR_INVALID_ARG, and nothing applied, for a group at or beyond
 * n_groups, two records of one group, a non-zero `reserved`, or a record the FAULT rules above refuse (the malformed record is
 * refused on the host; FAULT is then left to "self is not in RG_CFG_PRESENT(old)"). Afterwards the host's copy of the cfg column, if
 * it holds one, is updated. */
int rgc_apply_conf(rg_engine *h, const rgc_conf_rec *host_recs, uint64_t n, rgc_conf_resp *host_resp,
                   uint64_t max_entries_per_msg, uint32_t flags,
                   rg_send_item *host_items, uint64_t item_cap, uint64_t *n_items);

/* The dense form: dev_sel u8[n_groups], 0 = not selected; dev_cfg u32[n_groups], read only where selected. Writes status[g] for
 * EVERY group (RGC_CONF_NONE where not selected: such a group costs its selector byte and its status byte); events and commit, where
 * given, are written for selected groups only. *count is zeroed on the engine's stream before the launch; items may be NULL when
 * item_cap is 0. Asynchronous: a tick queued after the call sees the new configuration. */
typedef struct {
    uint8_t *status, *events; /* [n_groups]; status mandatory */
    uint64_t *commit;         /* [n_groups] */
    rg_send_item *items;
    uint64_t item_cap;
    uint32_t *count;
} rgc_conf_out; /* all DEVICE memory */
int rgc_apply_conf_device(rg_engine *h, const uint8_t *dev_sel, const uint32_t *dev_cfg,
                          uint64_t max_entries_per_msg, uint32_t flags, const rgc_conf_out *dev_out);

/* State rules, all checked on the host before anything is staged or launched. RG_ERR_STATE: a tick's send stage is still owed
 * (rg_send_appends); groups still carry RG_OUT_HOST_HINT (rg_resolve_host_hints); ingested records are not ticked yet; RG_SEND_BYTES
 * without rg_log_sizes_enable; the engine has a host mirror (rg_set_peers), in both forms: its peer-id tables map ids to slots, and
 * rg_set_config stays its road. RG_ERR_INVALID_ARG: unknown flags, a required pointer that is NULL, item arguments on an engine
 * without device Inflights, a bad record (above). After the dense form the host has not seen the words: its copy of the cfg column
 * is dropped, and the next dense tick derives the size classes again (after the sparse form only where a word names more slots than
 * its block's class, rg_set_config's rule). With commit publication on, a call counts as a reloaded commit column. The calls keep no
 * state: checkpoint, restore and rg_permute_groups need nothing. */

#ifdef __cplusplus
}
#endif
#endif /* RAFTGROUPS_CONF_H */
