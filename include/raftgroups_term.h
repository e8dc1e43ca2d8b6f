/* raftgroups_term.h -- the leader's term gate and the deposition: a SECOND extension of include/raftgroups.h, beside
 * raftgroups_lead.h and in a header of its own.
 *
 * raftgroups.h and raftgroups_lead.h stay as they are: their entry points, struct layouts, RG_ABI_VERSION and RGX_LEAD_VERSION are
 * unchanged, and a caller that does not include this file sees the same library as before. The entry points declared here carry the
 * prefix rgt_; the types and constants are rgt_ / RGT_ too. RGT_TERM_VERSION is bumped whenever a layout or a signature of THIS file
 * changes; rgt_term_version() returns what the library was built with. Same rules as raftgroups.h otherwise: C99, no exception
 * leaves an entry point, int results are RG_OK or an RG_ERR_* code with the text in rg_last_error().
 *
 * This header SUPERSEDES the note of raftgroups_lead.h that "ONLY the device's own step-down is covered: a leader deposed by a higher
 * term is the host's to stop": with the calls below the device stops such a group itself, drops its pending reads in the same call
 * and takes it back into the follower arena at the new term. The per-tick loop of a store becomes
 *     rg_follow_clock, rgx_lead_clock, rgt_lead_gate_device, rg_tick_device, rgt_follow_depose_device
 * and the host keeps no group's term. What stays with the host: vote requests that reach a leader (the lease test needs the
 * leader's election_elapsed; the sparse flow rg_follow_demote -> rg_follow_step_gated -> rgx_lead_clock_write(led = 0) serves them). */
#ifndef RAFTGROUPS_TERM_H
#define RAFTGROUPS_TERM_H
#include "raftgroups_lead.h"
#ifdef __cplusplus
extern "C" {
#endif

#define RGT_TERM_VERSION 1u
uint32_t rgt_term_version(void); /* RGT_TERM_VERSION of the build */

/* ---- The gate: the term check of Raft::step (src/raft.rs:1282-1411) for the two kinds of record a dense leader tick carries,
 *      MsgAppendResponse (RG_MF_VALID) and MsgHeartbeatResponse (RG_MF_HEARTBEAT), for every group of the leader engine in one
 *      launch, IN FRONT of rg_tick_device ----
 * rg_msgs has no term column: dev_m_term is that column, u64 [P][stride] like m_index, the Message.term of the record staged in the
 * slot. Only m_flags of dev_msgs is read (8-byte aligned, like dev_out->flags). A RECORD is a slot below the engine's slot count
 * whose flag byte has RG_MF_VALID or RG_MF_HEARTBEAT; dev_m_term is loaded for records of led groups only, and RG_COL_CFG is not
 * read to judge one: a response staged in a slot without a Progress is the host's error (RawNode::step answers StepPeerNotFound
 * before the term check, src/raw_node.rs:402-411). Flag bytes at or beyond the slot count pass unchanged unless the row is zeroed.
 * Per group, with cur = RG_COL_CUR_TERM[g]:
 *   led = (clock tag != cur) || !STOPPED(clock cell) -- the lazy-arming rule of rgx_lead_clock, READ ONLY: the gate never arms a group.
 *   NOT LED: the whole flag row becomes 0 (a follower has no arm for these responses, and the group's Progress cells are without
 *     meaning): RGT_GATE_EV_NOT_LED; its records are counted in counts[2].
 *   LED, per record with t = its term:
 *     t == 0 || t == cur  passes. A term of 0 is a local message (raft.rs:1282-1283): the own slot's events (the persist ack,
 *                         RG_MF_APPEND, RG_MF_BECOME_LEADER) carry 0 BY CONTRACT.
 *     t < cur             ignored (raft.rs:1349-1410: a response of a lower term is dropped, nothing is sent): the byte loses
 *                         RG_MF_VALID | _REJECT | _HAS_RS | _HAS_LOGTERM | _HEARTBEAT and KEEPS RG_MF_SENT and RG_MF_INS_FULL --
 *                         they are the host's facts, not the message's, and the tick applies a SENT-only byte on its own.
 *                         RGT_GATE_EV_STALE; counted in counts[1].
 *     t > cur             the group is DEPOSED: become_follower(m.term, INVALID_ID) (raft.rs:1346; neither kind is a pre-vote
 *                         grant, so the exception of :1319-1330 never applies). new_term = the maximum over such records, the
 *                         WHOLE row becomes 0, RGT_GATE_EV_DEPOSED (| RGT_GATE_EV_TRANSFER_ABORTED if a transferee was set). Nothing
 *                         else of the row is reported: no STALE bit, no count in counts[1].
 * THE ORDER RULE. The deposing record is taken as the FIRST of the group's records of the tick -- the same kind of rule as
 * "RG_MF_BECOME_LEADER runs before every other event". After become_follower, step_follower ignores responses; among several
 * higher terms only the maximum matters (a lower one is stale afterwards, a higher one runs become_follower again), so the outcome
 * does not depend on the order among the remaining records.
 * WHAT A DEPOSITION DOES TO THE LEADER ENGINE is what a check-quorum step-down does there: the clock cell is set STOPPED and the
 * tag becomes cur (both counters 0 where the tag was stale); the TRANSFEREE bits of RG_COL_CFG are cleared (reset, raft.rs:952);
 * where rg_read_index_enable has run the group's pending reads are dropped from this call on, in stream order (reset's
 * ReadOnly::new, :957 -- the term stamp of the queue, as rgx_lead_clock's step-down stores it). RG_COL_CUR_TERM, the Progress cells
 * and the Inflights are left alone, as a demotion leaves them. The gate keeps NO state of its own: checkpoint, restore and
 * rg_permute_groups need nothing.
 * A steady group costs 8 B of flags, 8 + 8 + 4 B of term, tag and clock cell and 8 B per record read, 8 + 1 B written; only a
 * deposed group touches RG_COL_CFG, the clock cells, the queue's term cell and new_term.
 * RG_ERR_STATE before rgx_lead_clock_enable (the clock's STOPPED bit is the only record of "led" on the device) and on an engine
 * with a host mirror (rg_step gates by its own table). Engines with max_inflight > 0 are allowed. */
#define RGT_GATE_EV_TRANSFER_ABORTED 0x08u /* the deposed group had a transferee (the value of RG_LEAD_EV_TRANSFER_ABORTED) */
#define RGT_GATE_EV_STALE 0x20u            /* at least one record of a lower term was dropped */
#define RGT_GATE_EV_NOT_LED 0x40u          /* the group is not led: its row was zeroed */
#define RGT_GATE_EV_DEPOSED 0x80u          /* a record of a higher term: the group is stopped, its row was zeroed */
typedef struct {
    uint8_t *flags;     /* [n_groups][8] the filtered RG_MF_* rows, written for every group; MAY alias dev_msgs->m_flags */
    uint8_t *events;    /* [n_groups] mandatory, written for every group (0 = led, nothing dropped) */
    uint64_t *new_term; /* [n_groups] mandatory, written ONLY where DEPOSED */
    uint64_t *down;     /* optional compact list of the deposed groups, order unspecified, as rgx_lead_clock's; NULL / cap 0 = none */
    uint64_t down_cap;
} rgt_lead_gate_out;    /* all DEVICE memory */
/* host_counts: u64 [3] = groups deposed, stale records dropped, records of not-led groups dropped -- the true totals whatever
 * down_cap is; NULL keeps the call asynchronous (the counts are in the device words of rgt_lead_gate_counts). */
int rgt_lead_gate_device(rg_engine *h, const rg_msgs *dev_msgs, const uint64_t *dev_m_term, const rgt_lead_gate_out *dev_out,
                         uint64_t *host_counts);
const uint64_t *rgt_lead_gate_counts(const rg_engine *h); /* device u64 [3] the last gate call wrote; NULL for a NULL engine */

/* ---- The deposition: the way back into the arena AT THE NEW TERM -- rgx_follow_step_down* with become_follower(T, INVALID_ID) in
 *      the place of become_follower(term, INVALID_ID) ----
 * One launch, all-or-nothing per group. Refusals, in this order: NOT_WON -- the arena does not hold what a win left; FAULT --
 * soft.term != RG_COL_CUR_TERM[L], or T <= soft.term, or anything rg_follow_demote answers FAULT to (the dense form also for a
 * dev_lead value at or beyond n_groups that is not RG_HANDOFF_NO_LEAD). On DONE the demotion's log import runs;
 * become_follower(T, 0) runs on the soft cells -- term = T, vote = 0, leader_id = 0, election_elapsed = 0 with a fresh timeout draw
 * chained at term T, the role stays Follower --; the election cells are not touched; the lead-side stop of the gate (clock cell,
 * tag, TRANSFEREE bits, pending reads) is applied idempotently -- the sparse form runs without a gate call, the dense form repeats
 * it harmlessly. The answer is {term = T, last_index, commit, out = 0}: the host persists the HardState before it answers anyone.
 * The dense form selects the follow groups F with dev_lead[F] < n_groups && (dev_events[dev_lead[F]] & RGT_GATE_EV_DEPOSED) and
 * takes T = dev_new_term[dev_lead[F]]: the two columns the gate wrote. Unselected groups cost what rgx_follow_step_down_device's
 * cost. Both forms need rg_follow_elect_enable (RG_ERR_STATE before it); the clock and ReadIndex layers are optional. The dense
 * form answers RG_ERR_STATE on an engine with a host mirror; the sparse form refuses on the host a follow group at or beyond
 * n_follow, a lead group at or beyond n_groups, a non-zero reserved word and two records naming the same follow or lead group, and
 * on a mirror engine makes the mirror re-read its cached cfg copy. CONTRACT of the dense forms: the selected groups name pairwise
 * different lead groups. */
typedef struct {
    uint64_t follow_group, lead_group, term, reserved; /* term: T, the higher term; reserved: 0 */
} rgt_depose_rec;
int rgt_follow_depose(rg_engine *h, const rgt_depose_rec *host_recs, uint64_t n, rg_handoff_resp *host_resp);
int rgt_follow_depose_device(rg_engine *h, const uint8_t *dev_events, const uint64_t *dev_new_term, const uint64_t *dev_lead,
                             const rg_handoff_out *dev_out);
/* The other road: a NEW LEADER's record (MsgAppend / MsgHeartbeat / TOUCH) of a higher term arrives in the follower stream for a
 * group this store leads. Run IN FRONT of rg_follow_step_gated_device with that call's own columns: dev_msg_flags =
 * rg_follow_msgs.flags, dev_term = its dev_term. Follow group F is selected when it has a message of one of the three kinds,
 * dev_lead[F] < n_groups, the arena holds the win state, soft.term == RG_COL_CUR_TERM[L] and dev_term[F] > soft.term; every other
 * group answers RG_HANDOFF_NONE and nothing of it changes (a dev_lead value at or beyond n_groups that is not RG_HANDOFF_NO_LEAD:
 * FAULT). A selected group gets the demotion's log import and the lead-side stop above, and NO soft-cell change: the gated step
 * that follows runs become_follower(m.term, from) itself, against the refreshed log. FAULT where rg_follow_demote refuses. The
 * answer's term is dev_term[F]. State rules as the dense deposition's. The sparse vote kinds stay with the host. */
int rgt_follow_depose_scan_device(rg_engine *h, const uint8_t *dev_msg_flags, const uint64_t *dev_term, const uint64_t *dev_lead,
                                  const rg_handoff_out *dev_out);

#ifdef __cplusplus
}
#endif
#endif /* RAFTGROUPS_TERM_H */
