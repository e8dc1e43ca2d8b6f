/* raftgroups_lead.h -- the leader's clock: an EXTENSION of include/raftgroups.h, in a header of its own.
 *
 * raftgroups.h stays as it is: its 129 entry points, its struct layouts and RG_ABI_VERSION 12 are unchanged, and a caller that
 * does not include this file sees the same library as before. The seven entry points declared here carry the prefix rgx_ (the
 * library's rg_* exports remain exactly the functions raftgroups.h declares); the types and constants keep the rg_ / RG_ names of
 * the rest of the interface. RGX_LEAD_VERSION is bumped whenever a layout or a signature of THIS file changes;
 * rgx_lead_version() returns what the library was built with. Same rules as raftgroups.h otherwise: C99, no exception leaves an
 * entry point, int results are RG_OK or an RG_ERR_* code with the text in rg_last_error(). */
#ifndef RAFTGROUPS_LEAD_H
#define RAFTGROUPS_LEAD_H
#include "raftgroups.h"
#ifdef __cplusplus
extern "C" {
#endif

#define RGX_LEAD_VERSION 1u
uint32_t rgx_lead_version(void); /* RGX_LEAD_VERSION of the build */

/* ---- The leader's clock: Raft::tick of a leader (Raft::tick_heartbeat, src/raft.rs:1051-1079; the MsgBeat / MsgCheckQuorum arms
 *      of step_leader, :1959-1973; ProgressTracker::quorum_recently_active, src/tracker.rs:346-361; send_heartbeat's commit,
 *      raft.rs:829-839; the reset of a step-down, :942-971) ----
 * Optional, like ReadIndex and the arena's layers: per group of the LEADER engine, struct-of-arrays over the engine's stride, a
 * term tag (u64) and one u32 clock cell (heartbeat_elapsed in bits 0..13, election_elapsed in bits 14..27, STOPPED in bit 31): 12
 * bytes per group of the stride. While a group is led both counters stay below their timeouts.
 * ARMING IS LAZY, as the ReadIndex queues empty lazily: when rgx_lead_clock runs and a group's tag differs from RG_COL_CUR_TERM[g],
 * that is a new leadership -- Raft::reset ran inside become_leader --: the tag takes the column's value, both counters become 0
 * and STOPPED is cleared, BEFORE this call's increment. Only rgx_lead_clock advances the counters, so this is exact, and no tick,
 * hand-off or other entry point knows of the clock: RG_MF_BECOME_LEADER in a tick and rg_follow_promote* change RG_COL_CUR_TERM.
 * At enable the tag is the column's current value. A host that loads RG_COL_CUR_TERM with rg_load_column for another reason (a
 * restart: the column changes, the leadership does not begin) corrects the cells with rgx_lead_clock_write afterwards.
 * Every call of this section before rgx_lead_clock_enable returns RG_ERR_STATE (rgx_lead_clock_counts: NULL), so does a second
 * enable. rg_checkpoint / rg_restore carry the cells, rg_permute_groups moves them with their groups, rg_destroy frees them,
 * rg_device_info.engine_bytes grows by their size. Engines with max_inflight > 0 are allowed. An image taken BEFORE the enable call
 * does not hold the layer: rg_restore to it leaves the cells alone, and a group whose RG_COL_CUR_TERM went back with the image no
 * longer equals its tag, so by the rule above the next rgx_lead_clock reports RG_LEAD_EV_NEW_TERM for it and restarts its counters. */
#define RG_LEAD_CLOCK_START_LED 0x100u /* every group starts as led, both counters 0; else every group starts stopped */
typedef struct {
    uint32_t election_tick;  /* Config::election_tick, 2..16383 */
    uint32_t heartbeat_tick; /* Config::heartbeat_tick, 1..election_tick-1 (Config::validate, src/config.rs:162-171) */
    uint32_t flags;          /* RG_GATE_CHECK_QUORUM | RG_LEAD_CLOCK_START_LED */
    uint32_t reserved;       /* 0 */
} rg_lead_clock_config;
int rgx_lead_clock_enable(rg_engine *h, const rg_lead_clock_config *cfg); /* once; second call RG_ERR_STATE */
typedef struct {
    uint64_t group, term; /* term: the tag */
    uint32_t election_elapsed, heartbeat_elapsed;
    uint8_t led, reserved[7];
} rg_lead_clock_cell;
/* Control path; synchronises. RG_ERR_INVALID_ARG, and nothing written, for a group at or beyond n_groups, election_elapsed >=
 * election_tick, heartbeat_elapsed >= heartbeat_tick, led above 1, non-zero reserved bytes, or two records of one group (the
 * read: a group at or beyond n_groups). All of it is refused on the host. */
int rgx_lead_clock_write(rg_engine *h, const rg_lead_clock_cell *host, uint64_t n);
int rgx_lead_clock_read(rg_engine *h, const uint64_t *host_groups, uint64_t n, rg_lead_clock_cell *host_out);
/* One Raft::tick of every led group in one launch. Per led group, in the reference's order: (1) both counters += 1. (2) If
 * election_elapsed >= election_tick: election_elapsed = 0; under RG_GATE_CHECK_QUORUM quorum_recently_active(self) runs on the
 * group's flag row and RG_COL_CFG -- the arithmetic of rg_quorum_recently_active, its effects on RG_PF_RECENT_ACTIVE included --
 * and a group whose quorum was not active STEPS DOWN: STOPPED is set, both counters become 0, the TRANSFEREE bits are cleared
 * (reset aborts the transfer, raft.rs:952), CHECK_QUORUM | STEPPED_DOWN is reported and there is no beat in this call
 * (raft.rs:1068-1070); a group that is still leader and has a transferee loses it (TRANSFER_ABORTED). (3) If heartbeat_elapsed >=
 * heartbeat_tick: heartbeat_elapsed = 0 and BEAT is reported. Without RG_GATE_CHECK_QUORUM no flag byte is read or written.
 *   A stopped group costs its tag, clock cell and RG_COL_CUR_TERM reads and one event byte; a led group between timeouts those
 *   reads, one 4-byte store and one event byte. RG_COL_CFG and RG_COL_PFLAGS are touched only at an election timeout,
 *   RG_COL_MATCH and RG_COL_COMMIT (and the cfg word) only on a beat with hb_commit.
 *   The lists are conveniences: a group that does not fit is still in `events` and was still ticked; the counts are the totals.
 * What a step-down does NOT do: the Progress cells of the group are not reset (they are without meaning until the next
 * become_leader, which resets them; a demotion leaves the leader columns alone too); device Inflights are emptied by the next
 * RG_MF_BECOME_LEADER tick as today; the ReadIndex context a bcast_heartbeat attaches stays a separate call over the beat list.
 * What it DOES to the ReadIndex layer, where rg_read_index_enable has run (before or after the clock's enable): the group's pending
 * reads are dropped unanswered, as reset's `self.read_only = ReadOnly::new(..)` drops them although the term stays (raft.rs:957).
 * Once the rgx_lead_clock call that reports STEPPED_DOWN has run, in stream order, every ReadIndex entry point finds that group's
 * queue empty and emits nothing for it: rg_read_pending_counts and rg_read_last_pending report 0, a late heartbeat ack of the same
 * term releases nothing, and the whole depth is free for the next leadership. The call stores one word for such a group, into the
 * queue's term cell (a stamp RG_COL_CUR_TERM does not equal), and the queue's own lazy reset does the rest; the stamp travels with
 * rg_checkpoint / rg_restore and rg_permute_groups like the rest of the queue, and no other group loads or stores a byte more.
 * ONLY the device's own step-down is covered: a leader deposed by a higher term is the host's to stop (rgx_lead_clock_write,
 * led = 0), and it keeps its queue until the host's next change of RG_COL_CUR_TERM empties it.
 * Entry conditions are those of rg_quorum_recently_active. On an engine with a host mirror the cached cfg copy is re-read after a
 * call that may have cleared transferee bits. */
#define RG_LEAD_EV_BEAT 0x1u             /* MsgBeat: bcast_heartbeat is due (raft.rs:1072-1077, :1959-1962) */
#define RG_LEAD_EV_CHECK_QUORUM 0x2u     /* MsgCheckQuorum was stepped (raft.rs:1058-1062) */
#define RG_LEAD_EV_STEPPED_DOWN 0x4u     /* ... and the quorum was not active: become_follower(term, 0) (raft.rs:1963-1972) */
#define RG_LEAD_EV_TRANSFER_ABORTED 0x8u /* still leader at the election timeout with a transferee: abort_leader_transfer (raft.rs:1063-1065) */
#define RG_LEAD_EV_NEW_TERM 0x10u        /* the lazy reset above was applied in this call */
typedef struct {
    uint8_t *events;    /* [n_groups], mandatory; written for EVERY group, 0 = stopped / nothing happened */
    uint64_t *beat;     /* optional compact list of the groups with EV_BEAT, order unspecified; NULL / cap 0 = none */
    uint64_t beat_cap;
    uint64_t *down;     /* ... of the groups with EV_STEPPED_DOWN */
    uint64_t down_cap;
    uint64_t *hb_commit; /* optional u64 [P][stride]: min(matched, committed) per slot, 0 without a Progress, written ONLY for the
                            groups with EV_BEAT (send_heartbeat, raft.rs:829-839); every other cell keeps its value */
} rg_lead_clock_out;    /* all DEVICE memory */
/* host_counts: u64 [4] = beats, check-quorum runs, step-downs, transfers aborted of this call; NULL keeps the call asynchronous
 * (the counts are in the device words of rgx_lead_clock_counts). */
int rgx_lead_clock(rg_engine *h, const rg_lead_clock_out *dev_out, uint64_t *host_counts);
const uint64_t *rgx_lead_clock_counts(const rg_engine *h); /* device u64 [4] the last rgx_lead_clock wrote; NULL before the enable */
/* The way back into the arena: demotion (rg_follow_demote*) plus the become_follower(term, INVALID_ID) that no record will ever
 * bring, in one launch and all-or-nothing per group. Refusals, in this order: NOT_WON -- the arena does not hold "Follower with
 * leader_id == self_id, self_id != 0", what a win left; FAULT -- soft.term != RG_COL_CUR_TERM[L], or anything rg_follow_demote
 * answers FAULT to (the dense form also for a dev_lead value at or beyond n_groups that is not RG_HANDOFF_NO_LEAD). On success
 * the demotion's log import runs; become_follower(term, 0) runs on the soft cells -- term and vote are kept, leader_id becomes 0,
 * election_elapsed 0 with a fresh timeout draw chained as everywhere else, the role stays Follower --; if the clock layer is
 * enabled the lead group's cell is set STOPPED (idempotent) and its tag becomes RG_COL_CUR_TERM[L], so that a promotion the clock has
 * not seen yet cannot re-arm the group on the next rgx_lead_clock. The election cells are not touched (the votes are read only while
 * role != Follower). The answer is {term, last_index, commit, out = 0}.
 * The dense form selects the follow groups F with dev_lead[F] < n_groups && (dev_events[dev_lead[F]] & RG_LEAD_EV_STEPPED_DOWN):
 * dev_events is what rgx_lead_clock wrote. RG_HANDOFF_NO_LEAD and unselected groups cost their dev_lead cell, at most one event
 * byte and their status byte. Needs rg_follow_elect_enable (RG_ERR_STATE before it). Contract and mirror rules are those of
 * rg_follow_demote*: the dense form answers RG_ERR_STATE on an engine with a host mirror, the selected groups name pairwise
 * different lead groups; the sparse form refuses on the host what rg_follow_demote refuses. */
#define RG_HANDOFF_NO_LEAD (~0ULL)
int rgx_follow_step_down(rg_engine *h, const rg_handoff_rec *host_recs, uint64_t n, rg_handoff_resp *host_resp);
int rgx_follow_step_down_device(rg_engine *h, const uint8_t *dev_events, const uint64_t *dev_lead, const rg_handoff_out *dev_out);

#ifdef __cplusplus
}
#endif
#endif /* RAFTGROUPS_LEAD_H */
