// rg_term.h -- the leader's term gate and the deposition (include/raftgroups_term.h): the per-group arithmetic of the term check of
// Raft::step (src/raft.rs:1282-1411) for the two response kinds a dense leader tick carries, and of the become_follower(m.term,
// INVALID_ID) that follows a higher term (:1346, reset :942-971, become_follower :1082-1087). Citations are relative to the
// pingcap/raft-rs v0.6.0 tree.
//
// Everything works on values: the flag row is one u64 (byte s = slot s), the terms of its records are eight u64s of which only the
// records' are meaningful. The lead-side stop reuses rg_lead.h (rg_lead_stop, rg_lead_read_stamp), the refusals and the soft cells
// reuse rg_lead_step_down_check and rg_gate_become_follower: tests/host_check/term_gate_twin.cpp checks the compositions against
// tests/term_gate_model.py.
//
// Host/device-clean like rg_lead.h: the kernels (rg_kernels_term.h) include it behind rg_common.h, the twin includes it ALONE.
#pragma once
#include "rg_lead.h"

#include "../../include/raftgroups_term.h"

// A record: a slot whose flag byte names a MsgAppendResponse or a MsgHeartbeatResponse
#define RG_TERM_RECORD_BITS (RG_MF_VALID | RG_MF_HEARTBEAT)
// ... and what a dropped record takes with it; RG_MF_SENT, RG_MF_INS_FULL (and the own slot's RG_MF_APPEND) are the host's facts
#define RG_TERM_RESPONSE_BITS (RG_MF_VALID | RG_MF_REJECT | RG_MF_HAS_RS | RG_MF_HAS_LOGTERM | RG_MF_HEARTBEAT)
RG_D bool rg_term_is_record(u64 row, u32 slot) { return ((row >> (8 * slot)) & RG_TERM_RECORD_BITS) != 0; }

// "Led", as the clock's lazy arming decides it, read only: a tag that differs from RG_COL_CUR_TERM is a leadership the clock has
// not seen yet (become_leader ran since), else the STOPPED bit says.
RG_D bool rg_term_led(u32 cell, u64 tag, u64 cur_term) { return tag != cur_term || !rg_lead_stopped(cell); }

// The gate of one group's row. `t[s]` is read only where slot s < P is a record and the group is led.
struct RgTermGate {
    u64 row, new_term;      // the filtered row; the highest term above cur_term (DEPOSED only)
    u32 events;             // RGT_GATE_EV_* without TRANSFER_ABORTED (the cfg word is the caller's, loaded only on DEPOSED)
    u32 n_stale, n_not_led; // records dropped for a lower term; records of a group that is not led
};
RG_D RgTermGate rg_term_gate_row(u64 row, u32 P, bool led, u64 cur_term, const u64 (&t)[8]) {
    RgTermGate r;
    r.row = row;
    r.new_term = 0;
    r.events = r.n_stale = r.n_not_led = 0;
    u64 stale_mask = 0;
    RG_FOLLOW_UNROLL
    for (u32 s = 0; s < 8; s++) {
        if (s >= P || !rg_term_is_record(row, s)) continue;
        if (!led) {
            r.n_not_led += 1;
            continue;
        }
        const u64 m_term = t[s];
        if (m_term == 0 || m_term == cur_term) continue; // a local message (raft.rs:1282-1283) or the leader's own term
        if (m_term > cur_term) {                         // :1284-1347: become_follower(m.term, INVALID_ID) (:1346)
            if (m_term > r.new_term) r.new_term = m_term;
        } else {                                         // :1349-1410: a response of a lower term is ignored
            stale_mask |= (u64)RG_TERM_RESPONSE_BITS << (8 * s);
            r.n_stale += 1;
        }
    }
    if (!led) {
        r.row = 0;
        r.events = RGT_GATE_EV_NOT_LED;
    } else if (r.new_term) { // the deposing record is the FIRST of the tick: step_follower ignores every other response
        r.row = 0;
        r.events = RGT_GATE_EV_DEPOSED;
        r.n_stale = 0;
    } else if (r.n_stale) {
        r.row = row & ~stale_mask;
        r.events = RGT_GATE_EV_STALE;
    }
    return r;
}

// What a deposition does to the lead group's cfg word: reset aborts the transfer (raft.rs:952). -> RGT_GATE_EV_TRANSFER_ABORTED or 0
RG_D u32 rg_term_abort_transfer(u32 &cfg) {
    if (!RG_CFG_TRANSFEREE(cfg)) return 0;
    cfg &= ~(0xfu << 20);
    return RGT_GATE_EV_TRANSFER_ABORTED;
}

// The way back at the new term (rgt_follow_depose*): rg_lead_step_down_check's refusals, then -- where the soft cells take the term
// (`soft`; the scan form leaves them to the gated step) -- a term that is not above the group's. The log half is rg_handoff_demote's.
RG_D u32 rg_term_depose_check(const RgHandoffWin &w, u64 lead_cur_term, u64 new_term, bool soft) {
    const u32 status = rg_lead_step_down_check(w, lead_cur_term);
    if (status != RG_HANDOFF_DONE) return status;
    if (soft && new_term <= w.term) return RG_HANDOFF_FAULT;
    return RG_HANDOFF_DONE;
}
// ... and become_follower(T, INVALID_ID) (raft.rs:1346) on the soft view of a group that passed: term = T, vote = 0, leader_id 0,
// election_elapsed 0 with a fresh timeout draw chained at T, the role stays Follower (`s` has its role loaded).
RG_D void rg_term_depose_soft(const RgGateCfg &cfg, u64 g, RgSoftView &s, u64 new_term) {
    u32 events = 0;
    rg_gate_become_follower(cfg, g, s, new_term, 0, events);
}
// The scan form's selection on values: a message of a kind the dense gated step takes, the win state at the lead group's term, a
// higher term in the record.
RG_D bool rg_term_scan_selects(u32 msg_flags, const RgHandoffWin &w, u64 lead_cur_term, u64 m_term) {
    const bool kind = msg_flags == RG_FOLLOW_MSG_APPEND || msg_flags == RG_FOLLOW_MSG_HEARTBEAT || msg_flags == RG_FOLLOW_MSG_TOUCH;
    return kind && rg_lead_step_down_check(w, lead_cur_term) == RG_HANDOFF_DONE && m_term > w.term;
}
