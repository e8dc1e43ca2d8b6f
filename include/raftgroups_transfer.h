/* raftgroups_transfer.h -- the batched leader transfer: Raft::handle_transfer_leader (src/raft.rs:1821-1889), what a leader does
 * with a MsgTransferLeader, for many led groups in ONE launch. A SIXTH extension of include/raftgroups.h, beside raftgroups_lead.h,
 * raftgroups_term.h, raftgroups_vote.h, raftgroups_handoff.h and raftgroups_conf.h and in a header of its own; it needs the core
 * header only.
 *
 * The six older headers stay as they are: their entry points, struct layouts and versions are unchanged, and a caller that does
 * not include this file sees the same library as before. The entry points declared here carry the prefix rgm_; the types and
 * constants are rgm_ / RGM_ too. RGM_TRANSFER_VERSION is bumped whenever a layout or a signature of THIS file changes;
 * rgm_transfer_version() returns what the library was built with. Same rules as raftgroups.h otherwise: C99, no exception leaves an
 * entry point, int results are RG_OK or an RG_ERR_* code with the text in rg_last_error().
 *
 * WHY. The device already handles every stage of a leader transfer but its start: the tick sends MsgTimeoutNow when the transferee
 * catches up (RG_OUT_TIMEOUT_NOW), and the transfer is aborted by rgx_lead_clock at the election timeout and at a step-down, by
 * rgt_* at a deposition, by rgv_* at a deposing vote and by rgc_apply_conf* when the transferee stops being a voter. SETTING the
 * transferee had one road, rg_set_config: a host read-modify-write of the WHOLE cfg word of ONE group with a synchronisation, of a
 * word whose TRANSFEREE bits the device clears -- and the host then owed election_elapsed = 0 (rgx_lead_clock_write) and the first
 * send_append or MsgTimeoutNow by hand. Transfers come in batches: a store drained for an upgrade, or a rebalance of leaders,
 * transfers every group the store leads, each to a different peer. rg_set_config keeps its behaviour and stays the road of an
 * engine with a host mirror.
 *
 * What stays on the host: dropping proposals while a transfer is in progress (tracked from RGM_XFER_STARTED and the existing
 * *_TRANSFER_ABORTED events), a follower forwarding MsgTransferLeader to its leader, and building the MsgTimeoutNow message.
 * Citations are relative to the pingcap/raft-rs v0.6.0 tree. */
#ifndef RAFTGROUPS_TRANSFER_H
#define RAFTGROUPS_TRANSFER_H
#include "raftgroups.h"
#ifdef __cplusplus
extern "C" {
#endif

#define RGM_TRANSFER_VERSION 1u
uint32_t rgm_transfer_version(void); /* RGM_TRANSFER_VERSION of the build */

/* status */
#define RGM_XFER_NONE 0u        /* the dense form: the group was not selected */
#define RGM_XFER_STARTED 1u     /* the transfer is set: the TRANSFEREE bits, election_elapsed = 0, the first message */
#define RGM_XFER_SELF 2u        /* ignored: the transferee is the leader itself (a previous transfer is aborted all the same) */
#define RGM_XFER_IN_PROGRESS 3u /* ignored: a transfer to this very slot is in progress; the election counter is NOT reset */
#define RGM_XFER_LEARNER 4u     /* ignored: the transferee is a learner */
#define RGM_XFER_NO_PROGRESS 5u /* ignored: the transferee has no Progress */
#define RGM_XFER_NOT_LED 6u     /* refused: the group is not led (the leader's clock is enabled and says so) */
#define RGM_XFER_FAULT 7u       /* refused: a slot >= the engine's slot count, or a cfg word whose SELF names no Progress */
/* events */
#define RGM_XFER_EV_TIMEOUT_NOW 0x1u      /* STARTED: the transferee is up to date: the host sends MsgTimeoutNow (raft.rs:1879-1885) */
#define RGM_XFER_EV_APPEND 0x2u           /* STARTED: send_append(transferee) is due (raft.rs:1887) */
#define RGM_XFER_EV_ABORTED_PREVIOUS 0x4u /* STARTED, SELF: a transfer to another slot was aborted first (raft.rs:1852) */

typedef struct {
    uint64_t group;
    uint32_t slot;     /* the transferee, Message.from */
    uint32_t reserved; /* 0 */
} rgm_transfer_rec;

typedef struct {
    uint64_t last_index, matched; /* last_index and the transferee's matched as the call saw them (matched 0 where there is no Progress) */
    uint32_t cfg;                 /* the word now in RG_COL_CFG (unchanged unless STARTED, or SELF with a previous transfer) */
    uint32_t n_items;             /* 0 or 1 (counted whether or not item_cap had room for it) */
    uint8_t status, events, previous, reserved; /* RGM_XFER_*, RGM_XFER_EV_*; slot + 1 of a transfer this call aborted, else 0; 0 */
    uint32_t reserved2;           /* 0 */
} rgm_transfer_resp;

/* ---- Per selected group ----
 * Let old = RG_COL_CFG[g], self = RG_CFG_SELF(old), hi = last_index, t = the record's slot. The checks run in the reference's order;
 * every status but STARTED, and SELF with a previous transfer, leaves every cell, every window, the clock cell and the item list
 * as it was:
 *   1. FAULT: t >= the engine's slot count; self >= the slot count; self is not in RG_CFG_PRESENT(old).
 *   2. NOT_LED: rgx_lead_clock_enable has run and the group is not led -- the test the term gate uses (the clock's STOPPED bit under
 *      a tag equal to RG_COL_CUR_TERM). Without the clock layer every group of the engine is led.
 *   3. NO_PROGRESS: t is not in RG_CFG_PRESENT(old) (raft.rs:1822-1829).
 *   4. LEARNER: t has a Progress and is in neither majority (conf().learners, :1832-1839; a voter of the outgoing majority alone is
 *      no learner). A leader demoted to learner that names itself gets LEARNER, not SELF.
 *   5. IN_PROGRESS: RG_CFG_TRANSFEREE(old) == t + 1 (:1841-1851). election_elapsed is NOT reset.
 *   A transfer to another slot is aborted here (:1852): the bits are cleared, RGM_XFER_EV_ABORTED_PREVIOUS is set, `previous` names it.
 *   6. SELF: t == self (:1860-1866). Nothing else happens.
 *   7. STARTED otherwise:
 *      TRANSFEREE becomes t + 1; every other bit of the word is kept.
 *      election_elapsed = 0 (:1876), with the leader's clock enabled: where the group's tag equals RG_COL_CUR_TERM the cell keeps its
 *      heartbeat counter and gets election_elapsed 0; where the tag differs -- a leadership the clock has not armed yet -- the cell
 *      is NOT touched, the next rgx_lead_clock zeroes both counters before its increment anyway. The tag is never written. Without
 *      the clock layer the counter is the host's, and STARTED tells it to reset.
 *      the first message: matched[t] == hi gives RGM_XFER_EV_TIMEOUT_NOW (:1879-1885), nothing else is written and there is no item.
 *      Otherwise RGM_XFER_EV_APPEND: send_append(t) = maybe_send_append(t, allow_empty = true) (:1887) is due. On an engine with
 *      max_inflight == 0 the event is all and the host sends, as it does after rg_recompute. On an engine with device Inflights ONE
 *      pass of maybe_send_append runs for that peer -- the pass of rgc_apply_conf* (raftgroups_conf.h) with allow_empty = true:
 *      is_paused, a pending snapshot request first, Compacted (a snapshot), max_entries_per_msg / RG_SEND_BYTES / RG_SEND_HOST are
 *      the send stage's (rg_send_appends); Progress::update_state(last) is applied in place: Replicate does next = last + 1 and
 *      ins.add(last), Probe sets paused; RG_PF_INS_FULL is kept exact. A paused peer gets no item; EV_APPEND is set all the same.
 *
 * WHERE THE ITEM GOES: to the CALLER's memory, by the rule of rgh_* / rgc_*: *n_items / *count is the TOTAL, only item_cap items are
 * written, nothing beyond item_cap is touched, item order is unspecified. The engine's own item list, item columns, RG_COL_OUT and
 * RG_COL_HOST_HINT are not touched; RG_COL_COMMIT is not written. On an engine WITHOUT device Inflights the item arguments must be
 * NULL / 0.
 *
 * `flags` takes RG_SEND_BYTES only.
 *
 * COST. The dense form reads one byte and writes one byte per group that is not selected. profiles/transfer.txt holds the measured
 * table (1 M x 5 groups, K of them alternately starting a transfer to a lagging voter and having it cleared, one MI355X; the host
 * route is rg_read_groups, rg_set_config per group and rgx_lead_clock_write): for K = 1 / 1 000 / 65 536 the
 * route takes 72 us / 14.1 ms / 888 ms with max_inflight 0 and 64 us / 13.9 ms / 885 ms with max_inflight 8; the sparse form 49 us /
 * 89 us / 2.3 ms and 55 us / 98 us / 3.0 ms; the dense form 6.6 / 4.9 / 10 us and 7.4 / 11.7 / 36 us. With nothing selected the dense
 * form takes 4.7 us (7.2 us with max_inflight 8, which adds the memset of the count word). */

/* The sparse form: staged, synchronises, answers per record. RG_ERR_INVALID_ARG, and nothing applied, for a group at or beyond
 * n_groups, two records of one group, a slot >= the engine's slot count, or a non-zero `reserved`. Afterwards the host's copy of
 * the cfg column, if it holds one, is updated from the answers. */
int rgm_transfer_leader(rg_engine *h, const rgm_transfer_rec *host_recs, uint64_t n, rgm_transfer_resp *host_resp,
                        uint64_t max_entries_per_msg, uint32_t flags,
                        rg_send_item *host_items, uint64_t item_cap, uint64_t *n_items);

/* The dense form: dev_to u8[n_groups], 0 = not selected, else the transferee's slot + 1 (a cell beyond the slot count is answered
 * with FAULT). Writes status[g] for EVERY group (RGM_XFER_NONE where not selected: such a group costs its dev_to byte and its status
 * byte); events, where given, are written for selected groups only. *count is zeroed on the engine's stream before the launch;
 * items may be NULL when item_cap is 0. Asynchronous: a tick queued after the call sees the transferee. */
typedef struct {
    uint8_t *status, *events; /* [n_groups]; status mandatory */
    rg_send_item *items;
    uint64_t item_cap;
    uint32_t *count;
} rgm_transfer_out; /* all DEVICE memory */
int rgm_transfer_leader_device(rg_engine *h, const uint8_t *dev_to,
                               uint64_t max_entries_per_msg, uint32_t flags, const rgm_transfer_out *dev_out);

/* State rules, all checked on the host before anything is staged or launched. RG_ERR_STATE: a tick's send stage is still owed
 * (rg_send_appends); groups still carry RG_OUT_HOST_HINT (rg_resolve_host_hints); ingested records are not ticked yet; RG_SEND_BYTES
 * without rg_log_sizes_enable; the engine has a host mirror (rg_set_peers), in both forms: rg_set_config stays its road.
 * RG_ERR_INVALID_ARG: unknown flags, a required pointer that is NULL, item arguments on an engine without device Inflights, a NULL
 * count on an engine with them, a bad record (above). A transferee always has a Progress, so no word names more slots than before
 * and the dense tick's size classes stay valid. After the dense form the host has not seen the words: its copy of the cfg column is
 * dropped. The calls keep no state: checkpoint, restore and rg_permute_groups need nothing. */

#ifdef __cplusplus
}
#endif
#endif /* RAFTGROUPS_TRANSFER_H */
