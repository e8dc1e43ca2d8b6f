// rg_handoff.h -- the hand-off (include/raftgroups.h: "The hand-off"): the per-group arithmetic that makes a followed group which
// won its election a group of the leader engine (promotion) and refreshes the arena's log summary from a group this store has
// been leading (demotion). Promotion is the log import followed by the arithmetic of RgTick::become_leader (rg_group.h) -- Raft::reset
// (src/raft.rs:942-971) + Raft::become_leader (:1151-1202) -- at new_term = the arena's term; demotion is the inverse import, checked
// with rg_follow_state_check. Citations are relative to the pingcap/raft-rs v0.6.0 tree.
//
// Everything works on values: the kernels (rg_kernels_handoff.h) load a group's cells into these structs, call the functions and
// store what they return, so that a lane issues all its loads before its first store. Every array index below is a compile-time
// constant once the loops are unrolled: the structs live in registers, not in scratch.
//
// Host/device-clean like rg_follow.h / rg_elect.h: the kernels include it behind rg_common.h, tests/host_check/handoff_twin.cpp
// includes it ALONE and is checked against tests/handoff_model.py, sanitizers included -- nothing below needs the HIP headers.
#pragma once
#include "rg_elect.h"

// One group's log summary as the follower arena holds it (RgFollowCols), by value.
struct RgHandoffLog {
    u64 committed, last, tail_first, tail_term, dummy_idx, dummy_term;
    u64 run_first[RG_TERM_RUNS], run_term[RG_TERM_RUNS];
    u32 n_old;
};
// ... and as the leader engine holds it: RG_COL_COMMIT, _TERM_LO, _TERM_HI, _CUR_TERM, _DUMMY_*, _RUN_FIRST / _TERM, _RUN_COUNT.
struct RgHandoffLead {
    u64 commit, lo, hi, cur_term, dummy_idx, dummy_term;
    u64 run_first[RG_TERM_RUNS], run_term[RG_TERM_RUNS];
    u32 n_runs;
};
// What a win leaves in the soft and election cells.
struct RgHandoffWin {
    u64 term, lead, self_id;
    u32 role, conf;
};
// The Progress side of a promotion: the new flag row and cfg word, and which cells are written. Slot i of `present` gets
// matched = 0, next = next_all -- the own slot matched = persisted, next = persisted + 1, committed_index = the log's commit.
struct RgHandoffProgress {
    u64 pf;
    u32 cfg, present, self;
    u32 clear_snap, clear_rs; // slots whose RG_COL_PEND_SNAP / RG_COL_PEND_RS cell becomes 0 (the flag bits are exact)
    u64 next_all;
};

// The refusals of a promotion, in the header's order. `persisted` is F.last_index where the host vouches for it.
RG_D u32 rg_handoff_promote_check(const RgHandoffLog &f, const RgHandoffWin &w, u32 cfg, u32 P, u64 persisted) {
    if (w.role != 0 || w.lead != w.self_id || w.self_id == 0) return RG_HANDOFF_NOT_WON;
    const u32 self = RG_CFG_SELF(cfg);
    if (RG_ELECT_CONF_SELF(w.conf) != self || RG_ELECT_CONF_INCOMING(w.conf) != RG_CFG_INCOMING(cfg) || RG_ELECT_CONF_OUTGOING(w.conf) != RG_CFG_OUTGOING(cfg) ||
        !((RG_CFG_PRESENT(cfg) >> self) & 1u) || self >= P)
        return RG_HANDOFF_CONF;
    if (persisted != f.last) return RG_HANDOFF_NOT_PERSISTED;
    if (f.last >= (1ULL << 63) - 1) return RG_HANDOFF_FAULT; // last_index + 1 reaches 2^63
    const u64 last_term = f.tail_first <= f.last ? f.tail_term : f.dummy_term;
    if (!(w.term > last_term)) return RG_HANDOFF_FAULT; // rg_election_valid: a new leader's term is above every term of its log
    return RG_HANDOFF_DONE;
}

// The log import: the arena's summary in the leader engine's columns. An empty tail (the log ends at the dummy entry) has no
// older runs.
RG_D RgHandoffLead rg_handoff_import(const RgHandoffLog &f) {
    RgHandoffLead l;
    const bool tail = f.tail_first <= f.last;
    const u32 n = tail ? (f.n_old < RG_TERM_RUNS ? f.n_old : (u32)RG_TERM_RUNS) : 0u;
    l.commit = f.committed;
    l.dummy_idx = f.dummy_idx;
    l.dummy_term = f.dummy_term;
    l.lo = tail ? f.tail_first : f.dummy_idx + 1;
    l.hi = tail ? f.last : f.dummy_idx;
    l.cur_term = tail ? f.tail_term : f.dummy_term;
    l.n_runs = n;
    RG_FOLLOW_UNROLL
    for (u32 k = 0; k < RG_TERM_RUNS; k++) {
        l.run_first[k] = k < n ? f.run_first[k] : 0;
        l.run_term[k] = k < n ? f.run_term[k] : 0;
    }
    return l;
}

// RgTick::become_leader on the log summary, at new_term (checked: above l.cur_term): the old range is filed as a run
// (rg_push_run: a full table drops its oldest run), the empty entry is appended.
RG_D void rg_handoff_become_leader(RgHandoffLead &l, u64 new_term) {
    if (l.lo <= l.hi) {
        const bool full = l.n_runs >= RG_TERM_RUNS;
        const u32 k = full ? (u32)RG_TERM_RUNS - 1u : l.n_runs;
        RG_FOLLOW_UNROLL
        for (u32 j = 0; j < RG_TERM_RUNS; j++) {
            const u64 nf = j + 1 < RG_TERM_RUNS ? l.run_first[j + 1 < RG_TERM_RUNS ? j + 1 : j] : 0;
            const u64 nt = j + 1 < RG_TERM_RUNS ? l.run_term[j + 1 < RG_TERM_RUNS ? j + 1 : j] : 0;
            if (full) {
                l.run_first[j] = nf;
                l.run_term[j] = nt;
            }
            if (j == k) {
                l.run_first[j] = l.lo;
                l.run_term[j] = l.cur_term;
            }
        }
        if (!full) l.n_runs += 1;
    }
    l.hi += 1; // append_entry(&mut [Entry::default()]) (raft.rs:1191-1194)
    l.lo = l.hi;
    l.cur_term = new_term;
}

// ... and on the Progress cells: `pf` the group's flag row (RG_COL_PFLAGS), `cfg` its cfg word, `old_hi` last_index before the
// empty entry. Slots at or beyond P are not touched whatever the cfg word says.
RG_D RgHandoffProgress rg_handoff_progress(u64 pf, u32 cfg, u32 P, u64 old_hi) {
    RgHandoffProgress r;
    r.self = RG_CFG_SELF(cfg);
    r.present = RG_CFG_PRESENT(cfg) & ((1u << P) - 1u);
    r.clear_snap = r.clear_rs = 0;
    r.next_all = old_hi + 1;
    RG_FOLLOW_UNROLL
    for (u32 i = 0; i < 8; i++) {
        if (!((r.present >> i) & 1u)) continue;
        const u32 pb = (u32)(pf >> (8 * i)) & 0xffu;
        // Progress::reset (progress.rs:82-92); the own slot: become_replicate (raft.rs:1176-1181), has_pending_conf survives
        const u32 nb = i == r.self ? ((pb & RG_PF_PENDING_CONF) | RG_STATE_REPLICATE) : RG_STATE_PROBE;
        if (pb & RG_PF_PEND_SNAP) r.clear_snap |= 1u << i;
        if (pb & RG_PF_PEND_RS) r.clear_rs |= 1u << i;
        pf = (pf & ~(0xffULL << (8 * i))) | ((u64)nb << (8 * i));
    }
    r.pf = pf;
    r.cfg = RG_CFG_TRANSFEREE(cfg) ? cfg & ~(0xfu << 20) : cfg; // abort_leader_transfer (raft.rs:953)
    return r;
}

RG_D rg_handoff_resp rg_handoff_answer(u32 status, u64 term, u64 last_index, u64 commit, u32 out) {
    rg_handoff_resp a;
    a.term = term;
    a.last_index = last_index;
    a.commit = commit;
    a.status = status;
    a.out = out;
    return a;
}

// Demotion: the leader engine's summary as an rg_follow_state, canonical or refused (rg_follow_state_check). `s.group` is the
// caller's.
RG_D u32 rg_handoff_demote(const RgHandoffLead &l, rg_follow_state &s) {
    const bool tail = l.lo <= l.hi;
    const u32 n = l.n_runs;
    s.committed = l.commit;
    s.last_index = l.hi;
    s.dummy_index = l.dummy_idx;
    s.dummy_term = l.dummy_term;
    s.reserved = 0;
    s.n_runs = 0;
    RG_FOLLOW_UNROLL
    for (u32 k = 0; k < RG_FOLLOW_RUNS; k++) s.run_first[k] = s.run_term[k] = 0;
    if (n > RG_TERM_RUNS) return RG_HANDOFF_FAULT;
    s.n_runs = n + (tail ? 1u : 0u);
    RG_FOLLOW_UNROLL
    for (u32 k = 0; k < RG_FOLLOW_RUNS; k++) {
        const u64 tf = k < RG_TERM_RUNS ? l.run_first[k < RG_TERM_RUNS ? k : 0] : 0, tt = k < RG_TERM_RUNS ? l.run_term[k < RG_TERM_RUNS ? k : 0] : 0;
        s.run_first[k] = k < n ? tf : (k == n && tail) ? l.lo : 0;
        s.run_term[k] = k < n ? tt : (k == n && tail) ? l.cur_term : 0;
    }
    return rg_follow_state_check(s) ? RG_HANDOFF_FAULT : RG_HANDOFF_DONE;
}
// ... and that state in the arena's columns (rg_follow_store_state's layout, by value)
RG_D RgHandoffLog rg_handoff_export(const rg_follow_state &s) {
    RgHandoffLog f;
    const u32 n_old = s.n_runs ? s.n_runs - 1 : 0;
    f.committed = s.committed;
    f.last = s.last_index;
    f.dummy_idx = s.dummy_index;
    f.dummy_term = s.dummy_term;
    f.n_old = n_old;
    f.tail_first = s.last_index + 1;
    f.tail_term = s.dummy_term;
    RG_FOLLOW_UNROLL
    for (u32 k = 0; k < RG_FOLLOW_RUNS; k++) {
        if (s.n_runs && k == n_old) {
            f.tail_first = s.run_first[k];
            f.tail_term = s.run_term[k];
        }
        if (k < RG_TERM_RUNS) {
            f.run_first[k < RG_TERM_RUNS ? k : 0] = k < n_old ? s.run_first[k] : 0;
            f.run_term[k < RG_TERM_RUNS ? k : 0] = k < n_old ? s.run_term[k] : 0;
        }
    }
    return f;
}
