// rg_lead.h -- the leader's clock (include/raftgroups_lead.h): the per-group arithmetic of one Raft::tick of a
// group this store leads. Restated from Raft::tick_heartbeat (src/raft.rs:1051-1079), the MsgBeat / MsgCheckQuorum arms of
// step_leader (:1959-1973), ProgressTracker::quorum_recently_active (src/tracker.rs:346-361) with has_quorum (:367-372),
// send_heartbeat's commit (raft.rs:829-839) and the part of Raft::reset (:942-971) a record-less step-down runs. Citations are
// relative to the pingcap/raft-rs v0.6.0 tree.
//
// Everything works on values, in two phases, so that a lane loads only what its phase needs: rg_lead_advance sees the clock cell,
// the term tag and RG_COL_CUR_TERM; rg_lead_timeout, reached only at an election timeout, sees the cfg word and the flag row.
// rg_lead_tick is their composition -- what tests/host_check/lead_clock_twin.cpp checks against tests/lead_clock_model.py.
//
// Host/device-clean like rg_handoff.h: the kernels (rg_kernels_lead.h) include it behind rg_common.h, the twin includes it ALONE.
#pragma once
#include "rg_handoff.h"

#include "../../include/raftgroups_lead.h"

// The clock cell: heartbeat_elapsed in bits 0..13, election_elapsed in bits 14..27, STOPPED in bit 31. While a group is led both
// counters stay below their timeouts, which are at most 16383.
#define RG_LEAD_CELL_STOPPED 0x80000000u
#define RG_LEAD_TICK_MAX 0x3fffu
RG_D u32 rg_lead_hb(u32 c) { return c & RG_LEAD_TICK_MAX; }
RG_D u32 rg_lead_el(u32 c) { return (c >> 14) & RG_LEAD_TICK_MAX; }
RG_D bool rg_lead_stopped(u32 c) { return (c & RG_LEAD_CELL_STOPPED) != 0; }
RG_D u32 rg_lead_pack(u32 hb, u32 el, bool stopped) { return hb | (el << 14) | (stopped ? RG_LEAD_CELL_STOPPED : 0u); }

struct RgLeadCfg {
    u32 election_tick, heartbeat_tick, flags; // flags: RG_GATE_CHECK_QUORUM
};
// rg_lead_clock_config as the enable call takes it: 0 = fine, else the number of the rule it breaks (Config::validate,
// src/config.rs:162-171: heartbeat_tick > 0, election_tick > heartbeat_tick)
RG_FOLLOW_HD int rg_lead_config_check(u32 election_tick, u32 heartbeat_tick, u32 flags, u32 reserved) {
    if (election_tick < 2 || election_tick > RG_LEAD_TICK_MAX) return 1;
    if (heartbeat_tick < 1 || heartbeat_tick >= election_tick) return 2;
    if (flags & ~(RG_GATE_CHECK_QUORUM | RG_LEAD_CLOCK_START_LED)) return 3;
    if (reserved) return 4;
    return 0;
}
// rg_lead_clock_cell as rgx_lead_clock_write takes it (the group bound and the duplicate rule are the caller's): 0 = fine
RG_FOLLOW_HD int rg_lead_cell_check(const RgLeadCfg &lc, const rg_lead_clock_cell &w) {
    if (w.election_elapsed >= lc.election_tick) return 1;
    if (w.heartbeat_elapsed >= lc.heartbeat_tick) return 2;
    if (w.led > 1) return 3;
    for (int k = 0; k < 7; k++)
        if (w.reserved[k]) return 4;
    return 0;
}

// ProgressTracker::quorum_recently_active(self) (tracker.rs:346-361) on one group's flag row and cfg word: the own slot becomes
// recent_active, every other slot with a Progress gives its recent_active up; learners count as active ids, and the quorum is
// taken over the voters of both halves by id (has_quorum, :367-372: vote_result == Won, an empty half wins).
RG_D bool rg_quorum_active_row(u32 cfg, u64 &pf) {
    const u32 self = RG_CFG_SELF(cfg), present = RG_CFG_PRESENT(cfg);
    u32 active = 0;
    RG_FOLLOW_UNROLL
    for (u32 p = 0; p < 8; p++) {
        if (!((present >> p) & 1u)) continue;
        const u64 bit = (u64)RG_PF_RECENT_ACTIVE << (8 * p);
        if (p == self) {
            pf |= bit;
            active |= 1u << p;
        } else if (pf & bit) {
            active |= 1u << p;
            pf &= ~bit;
        }
    }
    return rg_elect_majority(RG_CFG_INCOMING(cfg), active, 0) == 2u && rg_elect_majority(RG_CFG_OUTGOING(cfg), active, 0) == 2u;
}

// Phase 1: the lazy arming and the two increments (raft.rs:1052-1053, :1056-1057, :1072-1073).
struct RgLeadAdvance {
    u64 tag;
    u32 cell, events;
    bool led, at_election, at_heartbeat;
};
RG_D RgLeadAdvance rg_lead_advance(const RgLeadCfg &lc, u32 cell, u64 tag, u64 cur_term) {
    RgLeadAdvance a;
    a.tag = tag;
    a.cell = cell;
    a.events = 0;
    if (tag != cur_term) { // a new leadership: Raft::reset ran inside become_leader (raft.rs:944-958)
        a.tag = cur_term;
        a.cell = 0;
        a.events = RG_LEAD_EV_NEW_TERM;
    }
    a.led = !rg_lead_stopped(a.cell);
    a.at_election = a.at_heartbeat = false;
    if (!a.led) return a;
    u32 hb = rg_lead_hb(a.cell) + 1, el = rg_lead_el(a.cell) + 1;
    a.at_election = el >= lc.election_tick;
    a.at_heartbeat = hb >= lc.heartbeat_tick;
    if (a.at_election) el = 0;
    if (a.at_heartbeat) hb = 0; // (a step-down zeroes it as well: reset, raft.rs:950)
    a.cell = rg_lead_pack(hb, el, false);
    return a;
}

// Phase 2, at an election timeout only: MsgCheckQuorum (raft.rs:1058-1062, :1963-1972) and abort_leader_transfer (:1063-1065).
// `pf` is read and written only under RG_GATE_CHECK_QUORUM. Returns the cell; a.events, cfg and pf are updated.
RG_D u32 rg_lead_timeout(const RgLeadCfg &lc, RgLeadAdvance &a, u32 &cfg, u64 &pf) {
    if (lc.flags & RG_GATE_CHECK_QUORUM) {
        a.events |= RG_LEAD_EV_CHECK_QUORUM;
        if (!rg_quorum_active_row(cfg, pf)) { // become_follower(term, INVALID_ID): reset(term) zeroes both counters and aborts the transfer (:950-952)
            a.events |= RG_LEAD_EV_STEPPED_DOWN;
            cfg &= ~(0xfu << 20);
            a.cell = rg_lead_pack(0, 0, true);
            return a.cell;
        }
    }
    if (RG_CFG_TRANSFEREE(cfg)) {
        cfg &= ~(0xfu << 20);
        a.events |= RG_LEAD_EV_TRANSFER_ABORTED;
    }
    return a.cell;
}
// ... and the beat (raft.rs:1068-1077): never in the call that stepped down
RG_D void rg_lead_beat(RgLeadAdvance &a) {
    if (a.at_heartbeat && !(a.events & RG_LEAD_EV_STEPPED_DOWN)) a.events |= RG_LEAD_EV_BEAT;
}

// The step-down's `self.read_only = ReadOnly::new(..)` (Raft::reset, raft.rs:957) at the UNCHANGED term: the stamp the group's
// ReadIndex queue gets in its term cell (RgReadCols::qterm, rg_read.h) in the call that reports STEPPED_DOWN. It differs from
// cur_term whatever cur_term is, so the queue's own lazy path (rg_read_sync_term) empties it at the next entry point that looks.
// A LATER term T' > T could hide behind the stamp only if T' == ~T, which needs T < 2^63 <= T': the nearest case is the election
// from T = 2^63 - 1 to T + 1 = 2^63 == ~T, and no term below 2^63 - 1 has one (log indices end at 2^63 long before a term gets
// there). Stored only on the step-down path: no other group loads or stores a byte more.
RG_D u64 rg_lead_read_stamp(u64 cur_term) { return ~cur_term; }

// One Raft::tick of one group: the composition the kernel runs. Returns the events.
RG_D u32 rg_lead_tick(const RgLeadCfg &lc, u32 &cell, u64 &tag, u64 cur_term, u32 &cfg, u64 &pf) {
    RgLeadAdvance a = rg_lead_advance(lc, cell, tag, cur_term);
    if (a.at_election) rg_lead_timeout(lc, a, cfg, pf);
    rg_lead_beat(a);
    cell = a.cell;
    tag = a.tag;
    return a.events;
}

// send_heartbeat's commit for one slot (raft.rs:829-839): min(pr.matched, raft_log.committed), 0 without a Progress
RG_D u64 rg_lead_hb_commit(u32 cfg, u32 slot, u64 matched, u64 committed) {
    return ((RG_CFG_PRESENT(cfg) >> slot) & 1u) ? (matched < committed ? matched : committed) : 0ULL;
}

// The control path's record <-> the two cells
RG_D u32 rg_lead_cell_of(const rg_lead_clock_cell &w) { return rg_lead_pack(w.heartbeat_elapsed, w.election_elapsed, !w.led); }
RG_D rg_lead_clock_cell rg_lead_record(u64 group, u64 tag, u32 cell) {
    rg_lead_clock_cell w;
    w.group = group;
    w.term = tag;
    w.election_elapsed = rg_lead_el(cell);
    w.heartbeat_elapsed = rg_lead_hb(cell);
    w.led = rg_lead_stopped(cell) ? 0 : 1;
    for (int k = 0; k < 7; k++) w.reserved[k] = 0;
    return w;
}

// The lead group's clock cell after a step-down into the arena: STOPPED, idempotent; the counters of a leadership the clock never saw
// (tag != cur_term; the caller stores cur_term as the tag) are 0 as the lazy arming would have left them.
RG_D u32 rg_lead_stop(u32 cell, u64 tag, u64 cur_term) { return (tag == cur_term ? cell : 0u) | RG_LEAD_CELL_STOPPED; }

// The way back into the arena (rgx_follow_step_down*): what the soft and election cells must hold, then the lead group's term.
// The log half of the refusals is rg_handoff_demote's.
RG_D u32 rg_lead_step_down_check(const RgHandoffWin &w, u64 lead_cur_term) {
    if (w.role != 0 || w.lead != w.self_id || w.self_id == 0) return RG_HANDOFF_NOT_WON;
    if (w.term != lead_cur_term) return RG_HANDOFF_FAULT;
    return RG_HANDOFF_DONE;
}
// ... and become_follower(term, INVALID_ID) (raft.rs:1969-1970) on the soft view of a group that passed the check: term and vote
// stay, leader_id becomes 0, election_elapsed 0 with a fresh timeout draw, the role stays Follower (`s` has its role loaded).
RG_D void rg_lead_step_down_soft(const RgGateCfg &cfg, u64 g, RgSoftView &s) {
    u32 events = 0;
    rg_gate_become_follower(cfg, g, s, s.term, 0, events);
}
