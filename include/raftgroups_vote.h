/* raftgroups_vote.h -- the dense vote step: MsgRequestVote / MsgRequestPreVote for every followed group in one launch, the groups
 * this store LEADS included. A THIRD extension of include/raftgroups.h, beside raftgroups_lead.h and raftgroups_term.h and in a
 * header of its own.
 *
 * The three older headers stay as they are: their entry points, struct layouts, RG_ABI_VERSION, RGX_LEAD_VERSION and
 * RGT_TERM_VERSION are unchanged, and a caller that does not include this file sees the same library as before. The entry points
 * declared here carry the prefix rgv_; the types and constants are rgv_ / RGV_ too. RGV_VOTE_VERSION is bumped whenever a layout or a
 * signature of THIS file changes; rgv_vote_version() returns what the library was built with. Same rules as raftgroups.h otherwise:
 * C99, no exception leaves an entry point, int results are RG_OK or an RG_ERR_* code with the text in rg_last_error().
 *
 * This header SUPERSEDES the note of raftgroups_term.h that "vote requests that reach a leader" stay with the host "(the lease
 * test needs the leader's election_elapsed ...)". It does not need it:
 *   in_lease = check_quorum && leader_id != INVALID_ID && election_elapsed < election_timeout      (src/raft.rs:1289-1291)
 *   a leader has leader_id == id != 0; only tick_heartbeat advances a leader's election_elapsed, and it resets it to 0 the moment
 *   it reaches election_timeout (:1051-1079); become_leader -> reset zeroes it. Between any two steps a leader therefore has
 *   election_elapsed < election_timeout, and  in_lease == check_quorum  (rgx_lead_clock_write refuses election_elapsed >=
 *   election_tick for the same reason).
 * So the calls below judge a request at a led group without the counters of its clock cell. The per-tick loop of a store becomes
 *     rg_follow_clock, rgx_lead_clock, rgv_follow_vote_device, rgt_lead_gate_device, rg_tick_device, rgt_follow_depose_device
 * -- the vote step IN FRONT of the leader's term gate, which then finds a group a vote deposed NOT_LED and zeroes its row. The
 * sparse flow rgx_lead_clock_read, rg_follow_demote, rg_follow_step_gated, rgx_lead_clock_write(led = 0) is no longer needed.
 * rg_follow_step_gated_device still answers RG_FOLLOW_FAULT to the two vote kinds: they are this header's.
 * Citations are relative to the pingcap/raft-rs v0.6.0 tree. */
#ifndef RAFTGROUPS_VOTE_H
#define RAFTGROUPS_VOTE_H
#include "raftgroups_term.h"
#ifdef __cplusplus
extern "C" {
#endif

#define RGV_VOTE_VERSION 1u
uint32_t rgv_vote_version(void); /* RGV_VOTE_VERSION of the build */

/* ---- Per group: Raft::step of one MsgRequestVote / MsgRequestPreVote (the gate src/raft.rs:1282-1411, the vote step :1418-1461) ----
 * NOT LED -- dev_lead is NULL, the group's dev_lead cell is RG_HANDOFF_NO_LEAD, or the arena does not hold the win state (Follower
 *   with leader_id == self_id, self_id != 0): the answer and every cell are exactly rg_follow_step_gated's for the same record,
 *   the undo to RG_FOLLOW_HOST included. A dev_lead value at or beyond n_groups that is not RG_HANDOFF_NO_LEAD: status FAULT.
 * LED -- the win state holds and soft.term == RG_COL_CUR_TERM[L]. A different term is FAULT (as rg_lead_step_down_check answers);
 *   where the clock layer is on and the cell is STOPPED under the tag of the current term the lead side has stopped the group
 *   already and the host called out of order: FAULT. The leader's log is computed in registers from the leader columns with the
 *   demotion's arithmetic (a log rg_follow_demote refuses: FAULT). With cur = soft.term:
 *     m.term <  cur            PREVOTE: PREVOTE_LOW, term = cur. VOTE: IGNORED (:1349-1410). Nothing changes.
 *     m.term == cur            VOTE_REJECT: can_vote is false (:1420-1426 -- the leader voted for itself and knows a leader).
 *                              term = cur, commit / log_term = commit_info() of the LEADER's log; maybe_commit_by_vote does NOT
 *                              run (self.state == Leader, :2131). Nothing changes. ONE departure: a request whose `from` is the
 *                              id in the vote cell (the leader's own id) answers FAULT. The reference would find can_vote true
 *                              and could grant -- a leader that records a vote and restarts its election_elapsed while it
 *                              goes on leading; no node sends itself a request, so such a record is forged or corrupted and
 *                              is handed to the host instead of inventing that state.
 *     m.term >  cur, RG_GATE_CHECK_QUORUM and no RG_GATE_FORCE: IGNORED, the lease (:1285-1317). Nothing changes.
 *     m.term >  cur otherwise, PREVOTE: the term is not changed (:1319-1330 "never change our term in response to a pre-vote") and the
 *                              group stays led; can_vote is true. GRANT iff is_up_to_date(m.index, m.log_term) against the leader's
 *                              log and (m.index > last_index || priority <= m.priority), the priority being the arena's cell.
 *                              GRANT: term = m.term. REJECT: term = cur, commit_info(), no maybe_commit_by_vote. Nothing changes.
 *     m.term >  cur otherwise, VOTE: become_follower(m.term, INVALID_ID) (:1346) -- a DEPOSITION, all in this launch: the
 *                              demotion's log import is stored; the soft cells take term = m.term, vote 0, leader_id 0,
 *                              election_elapsed 0 with a fresh chained timeout draw; the lead-side stop of raftgroups_term.h is
 *                              applied (clock cell STOPPED under tag = cur, TRANSFEREE bits cleared, pending reads dropped by
 *                              the queue's term stamp); then the vote step runs as the Follower it now is on the imported
 *                              log: GRANT records vote = from, election_elapsed = 0; REJECT takes commit_info() and THEN
 *                              runs maybe_commit_by_vote. All or nothing: where a term lookup falls in a dropped gap the
 *                              status is RG_FOLLOW_HOST, gate PASS, events 0 and nothing changes, the deposition included.
 * events: RG_GATE_EV_* with their values, and the three bits below. A deposition reports HARD_STATE | LEADER_CHANGED | LED |
 * DEPOSED (| TRANSFER_ABORTED). RG_COL_CUR_TERM, the Progress cells and the Inflights are left alone, as a demotion leaves them. */
#define RGV_VOTE_EV_LED 0x20u              /* the request was judged as a leader's (every answer of a led group but FAULT / HOST) */
#define RGV_VOTE_EV_TRANSFER_ABORTED 0x40u /* the deposed group had a transferee */
#define RGV_VOTE_EV_DEPOSED 0x80u          /* the group was led and is a Follower of m.term now: the lead side is stopped */

/* ---- The dense form: one launch over the follower arena, asynchronous when host_counts == NULL ----
 * The request columns are those of rg_follow_step_gated_device, staged once: of dev_msgs flags, index, log_term, commit and ent_term
 * (= Message.commit_term) are read; dev_term / dev_from as there. A group is a REQUEST when its flag byte is exactly
 * RG_FOLLOW_MSG_VOTE or RG_FOLLOW_MSG_PREVOTE; every other value, the other kinds included, is no request here: status 0, gate 0,
 * events 0. A request with a term or a from of 0 answers status RG_FOLLOW_FAULT, gate 0, and nothing of the group changes (the rule
 * of the gated step). dev_priority (Message.priority) may be NULL: 0 everywhere. dev_hdr_flags, one byte per group holding
 * RG_GATE_FORCE, may be NULL: nothing is forced. dev_lead is the u64 [n_follow] map the depositions use (RG_HANDOFF_NO_LEAD or a
 * lead group; CONTRACT: the requests name pairwise different lead groups); NULL = no group is led.
 * status / gate / events are written for every group below n_follow, the u64 columns only where there was a request (FAULT: zeros).
 * A block of 256 groups without a request costs its flag bytes and its three answer bytes. */
typedef struct {
    uint8_t *status;      /* [n_follow] RG_FOLLOW_NONE, RG_FOLLOW_FAULT or RG_FOLLOW_HOST */
    uint8_t *gate;        /* [n_follow] RG_GATE_* */
    uint8_t *events;      /* [n_follow] RG_GATE_EV_* | RGV_VOTE_EV_* */
    uint64_t *term;       /* [n_follow] the term the response carries */
    uint64_t *commit;     /* [n_follow] committed / commit_info().0 */
    uint64_t *log_term;   /* [n_follow] commit_info().1 of a reject, else 0 */
    uint64_t *answered;   /* optional compact list of the groups whose gate is VOTE_GRANT, VOTE_REJECT or PREVOTE_LOW (a response is
                           * due), order unspecified, as rgx_lead_clock's lists; NULL / cap 0 = none */
    uint64_t answered_cap;
} rgv_vote_out; /* all DEVICE memory */
/* host_counts: u64 [5] = requests, grants, rejects (PREVOTE_LOW included), ignored, deposed -- the true totals whatever
 * answered_cap is. */
int rgv_follow_vote_device(rg_engine *h, const rg_follow_msgs *dev_msgs, const uint64_t *dev_term, const uint64_t *dev_from,
                           const int64_t *dev_priority, const uint8_t *dev_hdr_flags, const uint64_t *dev_lead,
                           const rgv_vote_out *dev_out, uint64_t *host_counts);
const uint64_t *rgv_follow_vote_counts(const rg_engine *h); /* device u64 [5] the last dense call wrote; NULL for a NULL engine */

/* ---- The sparse form: the same per-record device function over a list, one synchronising round trip ----
 * Refused on the host, with nothing staged: a follow group at or beyond n_follow, a lead group at or beyond n_groups that is not
 * RG_HANDOFF_NO_LEAD, a kind that is not exactly one vote kind, a term or a from of 0, unknown flag bits, two records naming the
 * same follow group or the same lead group. On an engine with a host mirror the mirror re-reads its cached cfg copy. */
typedef struct {
    uint64_t follow_group, lead_group; /* lead_group: RG_HANDOFF_NO_LEAD = the store does not lead the group */
    uint64_t term, from;               /* Message.term, Message.from: never 0 */
    uint64_t index, log_term;          /* the candidate's last entry */
    uint64_t commit, commit_term;      /* Message.commit, Message.commit_term */
    int64_t priority;                  /* Message.priority */
    uint32_t kind, flags;              /* RG_FOLLOW_MSG_VOTE or RG_FOLLOW_MSG_PREVOTE; RG_GATE_FORCE */
} rgv_vote_rec;
typedef struct {
    uint64_t term, commit, log_term, last_index; /* last_index: of the log the request was judged against (0 with FAULT) */
    uint32_t gate, events, status, reserved;
} rgv_vote_resp;
int rgv_follow_vote(rg_engine *h, const rgv_vote_rec *host_recs, uint64_t n, rgv_vote_resp *host_resp);

/* State rules. Both int calls need rg_follow_elect_enable (RG_ERR_STATE before it); the clock and ReadIndex layers are optional, as
 * for the deposition. Where the clock layer is enabled and its RG_GATE_CHECK_QUORUM flag differs from the arena gate's both forms
 * answer RG_ERR_STATE: a store has ONE Config. The dense form with a non-NULL dev_lead answers RG_ERR_STATE on an engine with a host
 * mirror (the sparse form serves it). Engines with max_inflight > 0 are allowed. The calls keep no state but the five count words:
 * checkpoint, restore and rg_permute_groups need nothing. */

#ifdef __cplusplus
}
#endif
#endif /* RAFTGROUPS_VOTE_H */
