// rg_elect.h -- the candidate half (include/raftgroups.h: "The candidate half"): the per-group arithmetic of a MsgHup, a
// MsgTimeoutNow and a vote response on the three layers of the follower arena -- the log summary and the soft cells of
// rg_follow.h and the election cells below. One function per reference function, restated from Raft::hup (src/raft.rs:1472-1525),
// campaign (:1217-1263), become_candidate / become_pre_candidate (:1101-1143), become_leader's reset (:1158-1161), poll
// (:2166-2201), the vote responses of step_candidate (:2230-2244), MsgTimeoutNow (:2245-2251, :2298-2318), maybe_commit_by_vote
// (:2126-2164), ProgressTracker::record_vote / tally_votes / vote_result (src/tracker.rs:307-344) over the majority and joint
// rules (src/quorum/majority.rs:130-154, src/quorum/joint.rs:56-67) -- the mask arithmetic of rg_kernels_quorum.h's rg_vote_*,
// lifted here so that a host compiler can read it. Citations are relative to the pingcap/raft-rs v0.6.0 tree.
//
// A header of its own, so that the gate's host twin keeps compiling the text it always did. Host/device-clean like rg_follow.h:
// the kernels (rg_kernels_elect.h) include it behind rg_common.h, tests/host_check/elect_twin.cpp includes it ALONE and is
// checked against tests/elect_model.py, sanitizers included.
#pragma once
#include "rg_follow.h"

// The election cells, F = stride groups each: 14 bytes per group.
struct RgElectCols {
    u64 *self_id;          // Raft.id
    u32 *conf;             // RG_ELECT_CONF_*
    unsigned short *votes; // yes | no << 8
};
struct RgElectView {
    u64 self_id;
    u32 conf, votes;
};
RG_D RgElectView rg_elect_open(const RgElectCols &c, u64 g) {
    RgElectView e;
    e.self_id = c.self_id[g];
    e.conf = c.conf[g];
    e.votes = c.votes[g];
    return e;
}
RG_D void rg_elect_close(const RgElectCols &c, u64 g, const RgElectView &e, const RgElectView &o) {
    if (e.votes != o.votes) c.votes[g] = (unsigned short)e.votes;
}

// One record. kind: RG_FOLLOW_MSG_VOTE / RG_FOLLOW_MSG_PREVOTE = a response to that request (from = the sender's slot), or one
// of the two below (from = Message.from, used by nothing but the well-formedness check).
#define RG_ELECT_K_HUP 0x20u
#define RG_ELECT_K_TIMEOUT_NOW 0x40u
#define RG_ELECT_F_REJECT 0x1u  /* Message.reject */
#define RG_ELECT_F_BLOCKED 0x2u /* num_pending_conf != 0 (hup) */
struct RgElectRec {
    u64 term, from, commit, commit_term;
    u32 kind, flags;
};
// ... as the sparse calls stage it
struct RgElectStaged {
    u64 group;
    RgElectRec r;
};
// A well-formed response record? (what the dense kernel answers FAULT to and the sparse call refuses on the host)
RG_FOLLOW_HD bool rg_elect_resp_well_formed(u32 kind, u64 term, u32 slot) {
    return (kind == RG_FOLLOW_MSG_VOTE || kind == RG_FOLLOW_MSG_PREVOTE) && term != 0 && slot <= 7u;
}
// A well-formed rg_follow_campaign_req? (flags: RG_CAMPAIGN_*)
RG_FOLLOW_HD bool rg_elect_campaign_well_formed(u32 flags, u64 term, u64 from) {
    if (flags & ~(RG_CAMPAIGN_TIMEOUT_NOW | RG_CAMPAIGN_BLOCKED)) return false;
    return !(flags & RG_CAMPAIGN_TIMEOUT_NOW) || (term != 0 && from != 0);
}

// MajorityConfig::vote_result (majority.rs:130-154) over slot masks: 0 Pending, 1 Lost, 2 Won
RG_D u32 rg_elect_majority(u32 M, u32 yes, u32 no) {
    const u32 n = (u32)__builtin_popcount(M);
    if (n == 0) return 2u; // an empty config wins
    const u32 q = n / 2u + 1u, y = (u32)__builtin_popcount(yes & M), missing = n - y - (u32)__builtin_popcount(no & M);
    if (y >= q) return 2u;
    if (y + missing >= q) return 0u;
    return 1u;
}
// tally_votes / vote_result (tracker.rs:313-344) -> JointConfig::vote_result (joint.rs:56-67): a vote of a slot outside the
// voters is in the cell and does not count
RG_D u32 rg_elect_vote_result(u32 conf, u32 votes) {
    const u32 yes = votes & 0xffu, no = votes >> 8;
    const u32 i = rg_elect_majority(RG_ELECT_CONF_INCOMING(conf), yes, no), o = rg_elect_majority(RG_ELECT_CONF_OUTGOING(conf), yes, no);
    if (i == 2u && o == 2u) return 2u;
    if (i == 1u || o == 1u) return 1u;
    return 0u;
}
// record_vote (tracker.rs:307-309): the first vote of a slot stays
RG_D void rg_elect_record_vote(RgElectView &e, u32 slot, bool granted) {
    const u32 bit = 1u << slot;
    if (!((e.votes | (e.votes >> 8)) & bit)) e.votes |= granted ? bit : bit << 8;
}

RG_D rg_follow_elect_resp rg_elect_answer(u64 term, u32 result, u32 events, u32 status) {
    rg_follow_elect_resp a;
    a.term = term;
    a.req_term = a.req_index = a.req_log_term = a.req_commit = a.req_commit_term = 0;
    a.result = result;
    a.events = events;
    a.req_kind = a.targets = a.flags = 0;
    a.status = status;
    return a;
}

RG_D void rg_elect_set_role(RgSoftView &s, u32 role) {
    s.role = role;
    s.have |= 10u; // loaded, to be stored
}
// the timeout draw and election_elapsed = 0 of reset (raft.rs:948-949), at the term `s` has now
RG_D void rg_elect_reset_clock(const RgGateCfg &cfg, u64 g, RgSoftView &s) {
    const u32 timeout = rg_follow_draw(cfg.seed, g, s.term, rg_clock_timeout(s.clock), cfg.min_timeout, cfg.max_timeout);
    s.clock = rg_clock_pack(0, rg_clock_promotable(s.clock), timeout);
}

#define RG_ELECT_C_NONE 0u /* no campaign: come in with a poll's result */
#define RG_ELECT_C_PRE 1u  /* CAMPAIGN_PRE_ELECTION */
#define RG_ELECT_C_REAL 2u /* CAMPAIGN_ELECTION, CAMPAIGN_TRANSFER */
// campaign(type) if there is one, then what poll does with the vote result (`res` of the caller's poll where type is NONE) --
// the reference's campaign -> poll -> campaign recursion as a loop, two rounds at the most. Works on the caller's copies.
// -> RG_ELECT_REQUESTS (the request fields of `a` filled) / PENDING / LOST / WON, or 0: a term of the dropped gap is needed.
RG_D u32 rg_elect_drive(const RgGateCfg &cfg, u64 g, RgSoftView &s, const RgFollowView &v, RgElectView &e, u32 type, u32 res, u32 &events,
                        rg_follow_elect_resp &a) {
    const u32 self_bit = 1u << RG_ELECT_CONF_SELF(e.conf);
    for (;;) {
        u64 req_term = 0;
        if (type == RG_ELECT_C_PRE) { // become_pre_candidate (raft.rs:1124-1143): neither the term nor the vote changes
            rg_elect_set_role(s, 1u);
            e.votes = 0;
            s.lead = 0;
            req_term = s.term + 1; // (:1221)
        } else if (type == RG_ELECT_C_REAL) { // become_candidate (:1101-1117) = reset(term + 1), vote = id
            s.term += 1;
            s.lead = 0;
            rg_elect_reset_clock(cfg, g, s);
            e.votes = 0;
            rg_soft_set_vote(s, e.self_id);
            rg_elect_set_role(s, 2u);
            req_term = s.term;
        }
        if (type != RG_ELECT_C_NONE) { // poll(self, true) (:1227)
            rg_elect_record_vote(e, RG_ELECT_CONF_SELF(e.conf), true);
            res = rg_elect_vote_result(e.conf, e.votes);
        }
        if (res == 2u) {
            if (rg_soft_role(s) == 1u) { // won as PreCandidate: campaign(CAMPAIGN_ELECTION) (:2185-2186)
                type = RG_ELECT_C_REAL;
                continue;
            }
            // won as Candidate: become_leader's reset(term) (:1158-1161) as far as the arena holds it; the group leaves the
            // arena's roles as a Follower of itself
            rg_elect_reset_clock(cfg, g, s);
            e.votes = 0;
            s.lead = e.self_id;
            rg_elect_set_role(s, 0u);
            return RG_ELECT_WON;
        }
        if (res == 1u) { // lost: become_follower(term, 0) (:2192-2197). (Not reachable from a campaign: the others' votes are missing.)
            rg_gate_become_follower(cfg, g, s, s.term, 0, events);
            e.votes = 0;
            return RG_ELECT_LOST;
        }
        if (type == RG_ELECT_C_NONE) return RG_ELECT_PENDING;
        // the vote requests (:1233-1259): last_index, last_term, commit_info()
        const RgFollowSeg lt = rg_follow_seg(v, v.last), ct = rg_follow_seg(v, v.committed);
        if (lt.lo != lt.hi || ct.lo != ct.hi) return 0u;
        a.req_kind = type == RG_ELECT_C_PRE ? RG_FOLLOW_MSG_PREVOTE : RG_FOLLOW_MSG_VOTE;
        a.req_term = req_term;
        a.req_index = v.last;
        a.req_log_term = lt.lo;
        a.req_commit = v.committed;
        a.req_commit_term = ct.lo;
        a.targets = (RG_ELECT_CONF_INCOMING(e.conf) | RG_ELECT_CONF_OUTGOING(e.conf)) & ~self_bit;
        return RG_ELECT_REQUESTS;
    }
}

// One well-formed record on one group. Nothing of `s`, `v` or `e` changes where the status is RG_FOLLOW_HOST.
RG_D rg_follow_elect_resp rg_elect_step(const RgGateCfg &cfg, u64 g, RgSoftView &s, RgFollowView &v, RgElectView &e, const RgElectRec &m) {
    const RgSoftView s0 = s;
    const u64 committed0 = v.committed;
    const u32 votes0 = e.votes;
    const bool response = (m.kind & (RG_FOLLOW_MSG_VOTE | RG_FOLLOW_MSG_PREVOTE)) != 0, reject = (m.flags & RG_ELECT_F_REJECT) != 0;
    u32 events = 0, result = RG_ELECT_IGNORED;
    rg_follow_elect_resp a = rg_elect_answer(0, 0, 0, RG_FOLLOW_NONE);
    bool host = false;
    if (m.kind != RG_ELECT_K_HUP) { // the term gate (raft.rs:1282-1411); a MsgHup is local
        if (m.term > s.term) {
            if (!(m.kind == RG_FOLLOW_MSG_PREVOTE && !reject)) { // (:1319-1321: a granted pre-vote carries OUR future term)
                rg_gate_become_follower(cfg, g, s, m.term, 0, events);
                e.votes = 0;
                result = RG_ELECT_STEPPED_DOWN;
            }
        } else if (m.term < s.term) {
            return rg_elect_answer(s.term, RG_ELECT_IGNORED, 0, RG_FOLLOW_NONE);
        }
    }
    const u32 role = rg_soft_role(s);
    if (response) {
        // step_candidate (:2230-2244): only the responses of our own candidacy; step_follower: `_ => {}`
        if (role != 0 && (role == 1u) == (m.kind == RG_FOLLOW_MSG_PREVOTE)) {
            rg_elect_record_vote(e, (u32)m.from, !reject); // poll(m.from, !m.reject)
            result = rg_elect_drive(cfg, g, s, v, e, RG_ELECT_C_NONE, rg_elect_vote_result(e.conf, e.votes), events, a);
            host = result == 0;
            // maybe_commit_by_vote (:2126-2164) with the role poll left behind; a group that has just won is a Leader (:2131)
            if (!host && result != RG_ELECT_WON && m.commit != 0 && m.commit_term != 0 && m.commit > v.committed) {
                const RgFollowSeg at = rg_follow_seg(v, m.commit);
                if (at.lo != at.hi && m.commit_term >= at.lo && m.commit_term <= at.hi) host = true;
                else if (at.lo == at.hi && at.lo == m.commit_term) {
                    v.committed = m.commit; // (term(m.commit) != 0: m.commit <= last_index)
                    if (rg_soft_role(s) != 0) events |= RG_GATE_EV_CONF_CHECK;
                }
            }
        }
    } else if (m.kind == RG_ELECT_K_TIMEOUT_NOW && (role != 0 || !rg_clock_promotable(s.clock))) {
        // step_candidate ignores it (:2245-2251); so does a Follower that is not promotable (:2311-2317)
    } else if (s.lead == e.self_id) {
        // hup of a group this store leads (:1473-1479): ignored
    } else if (m.flags & RG_ELECT_F_BLOCKED) {
        result = RG_ELECT_BLOCKED; // (:1502-1512)
    } else {
        const bool transfer = m.kind == RG_ELECT_K_TIMEOUT_NOW;
        const u32 type = (!transfer && (cfg.flags & RG_GATE_PRE_VOTE)) ? RG_ELECT_C_PRE : RG_ELECT_C_REAL; // (:1518-1524)
        result = rg_elect_drive(cfg, g, s, v, e, type, 0, events, a);
        host = result == 0;
        if (transfer && result == RG_ELECT_REQUESTS) a.flags = RG_ELECT_REQ_TRANSFER;
    }
    if (host) {
        s = s0;
        v.committed = committed0;
        e.votes = votes0;
        return rg_elect_answer(s.term, RG_ELECT_NONE, 0, RG_FOLLOW_HOST);
    }
    if (s.term != s0.term || v.committed != committed0) events |= RG_GATE_EV_HARD_STATE; // (the vote changes only with the term)
    if (s.lead != s0.lead) events |= RG_GATE_EV_LEADER_CHANGED;
    a.term = s.term;
    a.result = result;
    a.events = events;
    return a;
}

// ---- rg_follow_elect_write / rg_follow_elect_read ----
// 0 = acceptable, else which rule it breaks
RG_FOLLOW_HD int rg_follow_elect_check(const rg_follow_elect &w) {
    if (w.self_id == 0) return 1;
    if (w.yes & w.no) return 2;
    if (w.conf >> 19) return 3;
    return 0;
}
RG_D void rg_follow_store_elect(const RgElectCols &c, const rg_follow_elect &w) {
    c.self_id[w.group] = w.self_id;
    c.conf[w.group] = w.conf;
    c.votes[w.group] = (unsigned short)(w.yes | ((u32)w.no << 8));
}
// (the votes of a Follower read as 0: what reset left in the reference; the gate does not clear the cell)
RG_D rg_follow_elect rg_follow_load_elect(const RgElectCols &c, const u8 *role, u64 g) {
    rg_follow_elect w;
    const u32 votes = role[g] != 0 ? c.votes[g] : 0u;
    w.group = g;
    w.self_id = c.self_id[g];
    w.conf = c.conf[g];
    w.yes = (u8)(votes & 0xffu);
    w.no = (u8)(votes >> 8);
    w.reserved[0] = w.reserved[1] = 0;
    return w;
}
