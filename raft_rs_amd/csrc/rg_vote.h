// rg_vote.h -- the dense vote step (include/raftgroups_vote.h): the per-group arithmetic of Raft::step for a MsgRequestVote /
// MsgRequestPreVote that reaches a group this store LEADS -- the gate (src/raft.rs:1282-1411), the vote step (:1418-1461),
// become_follower(m.term, INVALID_ID) (:1346, reset :942-971), maybe_commit_by_vote (:2126-2164) over RaftLog::is_up_to_date /
// commit_info / maybe_commit (src/raft_log.rs:412, :637, :487). Citations are relative to the pingcap/raft-rs v0.6.0 tree.
//
// A group that is NOT led goes through rg_gate_step (rg_follow.h) unchanged; nothing here is reachable from an existing caller.
// The LEADER VARIANT below differs from it in three ways: the lease is check_quorum alone (a leader's election_elapsed is below
// election_timeout between any two steps: tick_heartbeat, :1051-1079, zeroes it the moment it gets there), the log is a VALUE
// (RgHandoffLog: what rg_handoff_demote + rg_handoff_export compute from the leader columns, in registers) and
// maybe_commit_by_vote runs only once the group has been deposed (self.state == Leader returns at :2131). Every array index is a
// compile-time constant once the loops are unrolled.
//
// Host/device-clean like rg_term.h: the kernels (rg_kernels_vote.h) include it behind rg_common.h, tests/host_check/vote_twin.cpp
// includes it ALONE and is checked against tests/vote_step_model.py.
#pragma once
#include "rg_term.h"

#include "../../include/raftgroups_vote.h"

// One request, as both forms hand it to the per-record function
struct RgVoteReq {
    u64 term, from, index, log_term, commit, commit_term;
    int64_t priority;
    u32 kind, hdr_flags;
};
// A REQUEST of the dense form: the flag byte is exactly one of the two vote kinds
RG_FOLLOW_HD bool rg_vote_is_request(u32 flags) { return flags == RG_FOLLOW_MSG_VOTE || flags == RG_FOLLOW_MSG_PREVOTE; }

RG_D rgv_vote_resp rg_vote_answer(u32 status, u32 gate, u32 events, u64 term, u64 commit, u64 log_term, u64 last_index) {
    rgv_vote_resp a;
    a.term = term;
    a.commit = commit;
    a.log_term = log_term;
    a.last_index = last_index;
    a.gate = gate;
    a.events = events;
    a.status = status;
    a.reserved = 0;
    return a;
}
RG_D rgv_vote_resp rg_vote_fault() { return rg_vote_answer(RG_FOLLOW_FAULT, RG_GATE_NONE, 0, 0, 0, 0, 0); }

// RaftLog::term(idx) (raft_log.rs:122-140) on a log summary by value: rg_follow_seg's interval, [lo, hi] with lo == hi everywhere
// but in the dropped gap between the dummy entry and the first known run.
struct RgVoteTerm {
    u64 lo, hi;
};
RG_D RgVoteTerm rg_vote_log_term(const RgHandoffLog &f, u64 idx) {
    RgVoteTerm t;
    t.lo = t.hi = 0;
    if (idx > f.last || idx < f.dummy_idx) return t;
    if (idx >= f.tail_first) {
        t.lo = t.hi = f.tail_term;
        return t;
    }
    if (idx == f.dummy_idx) {
        t.lo = t.hi = f.dummy_term;
        return t;
    }
    const u32 n = f.n_old;
    const u64 known = n ? f.run_first[0] : f.tail_first;
    if (idx < known) {
        t.lo = f.dummy_term;
        t.hi = n ? f.run_term[0] : f.tail_term;
        return t;
    }
    RG_FOLLOW_UNROLL
    for (u32 k = 0; k < RG_TERM_RUNS; k++)
        if (k < n && f.run_first[k] <= idx) t.lo = f.run_term[k]; // (ascending: the last run that starts at or below idx)
    t.hi = t.lo;
    return t;
}

// The vote step (raft.rs:1418-1461) of a request that passed the gate, on a log by value. `leader`: the group is (still) led, so
// maybe_commit_by_vote returns at once (:2131). `s` has its role loaded. Changes s (a recorded vote) and f.committed; `undone` =
// a term lookup fell in the dropped gap and the caller hands the record back with nothing changed.
RG_D rgv_vote_resp rg_vote_on_log(RgSoftView &s, RgHandoffLog &f, const RgVoteReq &m, bool can_vote, bool leader, u32 events, bool &undone) {
    const u64 committed0 = f.committed;
    undone = false;
    bool grant = can_vote;
    if (grant) { // is_up_to_date(m.index, m.log_term) (raft_log.rs:412)
        const RgVoteTerm lt = rg_vote_log_term(f, f.last);
        if (lt.lo != lt.hi) {
            undone = true;
            return rg_vote_fault();
        }
        grant = m.log_term > lt.lo || (m.log_term == lt.lo && m.index >= f.last);
    }
    if (grant) grant = m.index > f.last || *s.ppriority <= m.priority;
    if (grant) {
        if (m.kind == RG_FOLLOW_MSG_VOTE) { // only real votes are recorded (:1437-1441); a led group never gets here
            rg_soft_set_elapsed(s, 0);
            if (rg_soft_vote(s) != m.from) events |= RG_GATE_EV_HARD_STATE;
            rg_soft_set_vote(s, m.from);
        }
        return rg_vote_answer(RG_FOLLOW_NONE, RG_GATE_VOTE_GRANT, events, m.term, committed0, 0, f.last);
    }
    const RgVoteTerm ct = rg_vote_log_term(f, f.committed); // commit_info (raft_log.rs:637)
    if (ct.lo != ct.hi) {
        undone = true;
        return rg_vote_fault();
    }
    if (!leader && m.commit != 0 && m.commit_term != 0 && m.commit > f.committed) { // maybe_commit_by_vote -> maybe_commit
        const RgVoteTerm at = rg_vote_log_term(f, m.commit);
        if (at.lo != at.hi && m.commit_term >= at.lo && m.commit_term <= at.hi) {
            undone = true;
            return rg_vote_fault();
        }
        if (at.lo == at.hi && at.lo == m.commit_term) {
            f.committed = m.commit; // (term(m.commit) != 0: m.commit <= last_index)
            events |= RG_GATE_EV_HARD_STATE;
            if (rg_soft_role(s) != 0) events |= RG_GATE_EV_CONF_CHECK;
        }
    }
    return rg_vote_answer(RG_FOLLOW_NONE, RG_GATE_VOTE_REJECT, events, s.term, committed0, ct.lo, f.last);
}

// Is the group led, as far as the arena says? (the win state of rg_lead_step_down_check) -- then the lead group's term and, where
// the clock layer is on (`clock`), its cell decide between LED and FAULT.
RG_D bool rg_vote_win_state(u64 lead, u64 self_id, u32 role) { return role == 0 && self_id != 0 && lead == self_id; }
RG_D bool rg_vote_led_ok(u64 soft_term, u64 lead_cur_term, bool clock, u32 cell, u64 tag) {
    if (soft_term != lead_cur_term) return false;
    return !clock || rg_term_led(cell, tag, lead_cur_term); // stopped under the current tag: the host called out of order
}

// The LEADER VARIANT: one well-formed request at a led group. `s` the arena's soft view (role loaded), `f` the leader's log as the
// demotion computed it. -> the answer; `depose` = s and f hold what the arena takes and the lead side is to be stopped (the caller
// adds RGV_VOTE_EV_TRANSFER_ABORTED from the cfg word). Nothing of s / f is to be stored unless `depose`.
RG_D rgv_vote_resp rg_vote_led(const RgGateCfg &cfg, u64 g, RgSoftView &s, RgHandoffLog &f, const RgVoteReq &m, bool &depose) {
    const u64 cur = s.term;
    const RgSoftView s0 = s;
    const u64 committed0 = f.committed;
    depose = false;
    if (m.term < cur) // :1349-1410: only a pre-vote is answered
        return rg_vote_answer(RG_FOLLOW_NONE, m.kind == RG_FOLLOW_MSG_PREVOTE ? RG_GATE_PREVOTE_LOW : RG_GATE_IGNORED, RGV_VOTE_EV_LED, cur, committed0, 0, f.last);
    if (m.term > cur && (cfg.flags & RG_GATE_CHECK_QUORUM) && !(m.hdr_flags & RG_GATE_FORCE)) // :1285-1317 with in_lease == check_quorum
        return rg_vote_answer(RG_FOLLOW_NONE, RG_GATE_IGNORED, RGV_VOTE_EV_LED, cur, committed0, 0, f.last);
    u32 events = RGV_VOTE_EV_LED;
    bool can_vote, leader = true;
    if (m.term > cur && m.kind == RG_FOLLOW_MSG_VOTE) { // :1346: become_follower(m.term, INVALID_ID)
        rg_gate_become_follower(cfg, g, s, m.term, 0, events);
        events |= RG_GATE_EV_HARD_STATE | RG_GATE_EV_LEADER_CHANGED | RGV_VOTE_EV_DEPOSED;
        can_vote = true; // vote == 0 && leader_id == 0
        leader = false;
    } else if (m.term > cur) {
        can_vote = true; // :1424-1426: a pre-vote of a future term
    } else {
        // The one departure. The reference would find can_vote true here and, where the log test passes, GRANT: a Leader that
        // records a vote and zeroes its election_elapsed at its own term and goes on leading -- a state that needs a store into
        // the lead clock cell of a group that stays led, which no stage of the engine has, for a message no node sends (the only
        // id a leader has voted for at its term is its own, and bcast / campaign skip the own id). A forged or corrupted record is
        // the host's to look at: FAULT, nothing changes.
        if (rg_soft_vote(s) == m.from) return rg_vote_fault();
        can_vote = false;                                      // (leader_id != 0)
    }
    bool undone;
    const rgv_vote_resp a = rg_vote_on_log(s, f, m, can_vote, leader, events, undone);
    if (undone) {
        s = s0;
        f.committed = committed0;
        return rg_vote_answer(RG_FOLLOW_HOST, RG_GATE_PASS, 0, cur, committed0, 0, f.last);
    }
    depose = !leader;
    return a;
}

// The led half of one request on loaded values -- what the kernels and the twin both run: the refusals (the lead group's term, a
// cell the lead side has stopped already, a log the demotion refuses), the demotion's log in `f`, the leader variant.
RG_D rgv_vote_resp rg_vote_led_group(const RgGateCfg &cfg, u64 g, RgSoftView &s, const RgHandoffLead &l, bool clock, u32 cell, u64 tag, const RgVoteReq &m,
                                     RgHandoffLog &f, bool &depose) {
    depose = false;
    if (!rg_vote_led_ok(s.term, l.cur_term, clock, cell, tag)) return rg_vote_fault();
    rg_follow_state fs;
    fs.group = g;
    if (rg_handoff_demote(l, fs) != RG_HANDOFF_DONE) return rg_vote_fault();
    f = rg_handoff_export(fs);
    return rg_vote_led(cfg, g, s, f, m, depose);
}
