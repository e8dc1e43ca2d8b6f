// rg_follow.h -- the follower half: the per-group arithmetic of a MsgAppend / MsgHeartbeat step (include/raftgroups.h: "The
// follower half") and, in the second part of this file, of what stands in front of it and beside it in a non-leader's
// Raft::step: the term gate, the vote step and the election clock ("The follower's term gate, vote step and election clock").
//
// The engine's restatement of Raft::handle_append_entries (src/raft.rs:2389-2448, from :2394 on) and Raft::handle_heartbeat
// (:2452-2464) over RaftLog::term (src/raft_log.rs:122-140), match_term (:238), find_conflict (:182-198), find_conflict_by_term
// (:209-235), maybe_append (:249-279) and commit_to (:286-300). Citations are relative to the pingcap/raft-rs v0.6.0 tree.
// The reference walks entries; here the log is a bounded table of term runs and a message describes its entries as runs of
// (term, count). A log's terms never decrease with the index, so the indices that hold one term form ONE interval: comparing an
// entry run with the log segment by segment gives what the reference's entry-by-entry loop gives, for any entry terms.
//
// Three departures, all loud (RG_FOLLOW_FAULT, nothing applied):
//   * the reference APPENDS entries whose terms decrease, or whose first term is below the term of the entry they follow; the
//     table below relies on a monotone log, so such a record is refused;
//   * index + n >= 2^63 is refused (the arithmetic below then never wraps);
//   * where the reference panics (src/raft_log.rs:259-265, :291-298, src/log_unstable.rs:169) the record is refused.
// And one hand-back (RG_FOLLOW_HOST): the table keeps RG_TERM_RUNS older runs; once older ones were dropped the terms of
// (dummy, known) are not here. Such an entry's term is SOME value of [dummy_term, known_term]; every comparison is made on that
// interval, and one whose outcome is not the same for all of its values hands the record back, as does needing the value itself.
//
// Host/device-clean: the kernels (rg_kernels_follow.h) include it behind rg_common.h; a host program includes it ALONE and
// compiles it with any C++17 compiler (tests/host_check/follow_twin.cpp is checked that way against tests/follower_model.py,
// tests/host_check/gate_twin.cpp against tests/gate_model.py, sanitizers included) -- nothing below needs the HIP headers.
#pragma once
#include <stdint.h>

#include "../../include/raftgroups.h"

#ifndef RG_D /* stand-alone: a plain host build */
typedef uint64_t u64;
typedef unsigned int u32;
typedef unsigned char u8;
#define RG_D static inline
#define RG_FOLLOW_HD static inline
#else
#define RG_FOLLOW_HD RG_HD /* (the canonical-form check also runs in the library's host code) */
#endif
#if defined(__clang__) /* full unrolling where an array must not be indexed dynamically; g++ (the host twins) needs no hint */
#define RG_FOLLOW_UNROLL _Pragma("unroll")
#else
#define RG_FOLLOW_UNROLL
#endif

// The arena's columns, F = stride groups each. HOT: what the steady append (on the tail, in the tail's term) reads and writes.
// COLD: read only off that path, written only when a term changes or a log is cut.
struct RgFollowCols {
    u64 *committed, *last, *tail_first, *tail_term; // hot [F]; the tail run is [tail_first, last] (empty: tail_first == last + 1)
    u64 *dummy_idx, *dummy_term;                    // cold [F]
    u64 *run_first, *run_term;                      // cold [RG_TERM_RUNS][stride]: older runs 0..n_old-1, ascending
    u8 *n_old;                                      // cold [F]: older runs in use (an empty tail has none)
    u64 stride, n;                                  // n = n_follow
};

// One group's log while a lane works on it: the hot cells by value (the caller loads them and stores what changed), the cold
// ones through pointers at the group's cell of each column -- touched only where the arithmetic needs them.
struct RgFollowView {
    u64 committed, last, tail_first, tail_term;
    u64 *dummy_idx, *dummy_term, *run_first, *run_term;
    u8 *n_old;
    u64 stride;
};
RG_D RgFollowView rg_follow_open(const RgFollowCols &c, u64 g) {
    RgFollowView v;
    v.committed = c.committed[g];
    v.last = c.last[g];
    v.tail_first = c.tail_first[g];
    v.tail_term = c.tail_term[g];
    v.dummy_idx = c.dummy_idx + g;
    v.dummy_term = c.dummy_term + g;
    v.run_first = c.run_first + g;
    v.run_term = c.run_term + g;
    v.n_old = c.n_old + g;
    v.stride = c.stride;
    return v;
}
// store the hot cells a record changed (`o`: as they were loaded)
RG_D void rg_follow_close(const RgFollowCols &c, u64 g, const RgFollowView &v, const RgFollowView &o) {
    if (v.committed != o.committed) c.committed[g] = v.committed;
    if (v.last != o.last) c.last[g] = v.last;
    if (v.tail_first != o.tail_first) c.tail_first[g] = v.tail_first;
    if (v.tail_term != o.tail_term) c.tail_term[g] = v.tail_term;
}

// One record. Entry run 0 is (ent_term, n_entries); runs 1..n_ext are ext[0..n_ext).
struct RgFollowRec {
    u64 index, log_term, commit, ent_term;
    u32 n_entries, flags;
    const rg_follow_ent_run *ext;
    u32 n_ext;
};
RG_D u64 rg_follow_run_term(const RgFollowRec &m, u32 j) { return j == 0 ? m.ent_term : m.ext[j - 1].term; }
RG_D u64 rg_follow_run_count(const RgFollowRec &m, u32 j) { return j == 0 ? m.n_entries : m.ext[j - 1].count; }

// A stretch [start, end] of indices whose terms all lie in [lo, hi]; lo == hi everywhere but in the gap.
struct RgFollowSeg {
    u64 lo, hi, start, end;
};
// The stretch of the log `idx` lies in: RaftLog::term(idx) (raft_log.rs:122-140) for every index of it. Beyond last_index and
// below the dummy entry the term is 0.
RG_D RgFollowSeg rg_follow_seg(const RgFollowView &v, u64 idx) {
    RgFollowSeg s;
    if (idx > v.last) {
        s.lo = s.hi = 0;
        s.start = v.last + 1;
        s.end = ~0ULL;
        return s;
    }
    if (idx >= v.tail_first) { // (the tail is above the dummy entry: nothing cold is needed)
        s.lo = s.hi = v.tail_term;
        s.start = v.tail_first;
        s.end = v.last;
        return s;
    }
    const u64 dummy = *v.dummy_idx;
    if (idx < dummy) {
        s.lo = s.hi = 0;
        s.start = 0;
        s.end = dummy - 1;
        return s;
    }
    if (idx == dummy) {
        s.lo = s.hi = *v.dummy_term;
        s.start = s.end = dummy;
        return s;
    }
    const u32 n = *v.n_old;
    const u64 known = n ? v.run_first[0] : v.tail_first;
    if (idx < known) { // the dropped gap: some term of [dummy_term, known_term]
        s.lo = *v.dummy_term;
        s.hi = n ? v.run_term[0] : v.tail_term;
        s.start = dummy + 1;
        s.end = known - 1;
        return s;
    }
    s.start = known;
    s.lo = 0;
    s.end = v.tail_first - 1;
    for (u32 k = 0; k < n; k++) {
        const u64 first = v.run_first[(u64)k * v.stride];
        if (first > idx) {
            s.end = first - 1;
            break;
        }
        s.start = first;
        s.lo = v.run_term[(u64)k * v.stride];
    }
    s.hi = s.lo;
    return s;
}

// rg_push_run's rule for the follower's table: file [first, ...] of `term` as the newest older run; a full table drops its oldest.
RG_D void rg_follow_push_run(RgFollowView &v, u64 first, u64 term) {
    u32 k = *v.n_old;
    if (k >= RG_TERM_RUNS) {
        for (u32 j = 0; j + 1 < RG_TERM_RUNS; j++) {
            v.run_first[(u64)j * v.stride] = v.run_first[(u64)(j + 1) * v.stride];
            v.run_term[(u64)j * v.stride] = v.run_term[(u64)(j + 1) * v.stride];
        }
        k = RG_TERM_RUNS - 1;
    }
    v.run_first[(u64)k * v.stride] = first;
    v.run_term[(u64)k * v.stride] = term;
    *v.n_old = (u8)(k + 1);
}

// RaftLog::append of ents[conflict - index - 1 ..] (raft_log.rs:267-268 -> log_unstable.rs:156-180) on the run table: cut the
// log to conflict - 1, then the rest of entry run j (`rem` entries) and the runs behind it become the tail.
RG_D void rg_follow_cut_append(RgFollowView &v, const RgFollowRec &m, u64 conflict, u32 j, u64 rem) {
    const u64 cut = conflict - 1;
    if (cut < v.tail_first) { // the whole tail goes (or there was none): the run that holds `cut` becomes the tail
        const u32 n = *v.n_old;
        u32 keep = 0;
        for (u32 k = 0; k < n; k++)
            if (v.run_first[(u64)k * v.stride] <= cut) keep = k + 1;
        if (keep) {
            v.tail_first = v.run_first[(u64)(keep - 1) * v.stride];
            v.tail_term = v.run_term[(u64)(keep - 1) * v.stride];
            keep--;
        } else {
            v.tail_first = conflict; // nothing known is left below: an empty tail on the dummy entry or on the gap
        }
        if (keep != n) *v.n_old = (u8)keep;
    }
    v.last = cut;
    for (u32 r = j; r <= m.n_ext; r++) {
        const u64 cnt = r == j ? rem : rg_follow_run_count(m, r);
        if (cnt == 0) continue;
        const u64 t = rg_follow_run_term(m, r);
        if (v.tail_first > v.last) { // empty tail
            v.tail_first = v.last + 1;
            v.tail_term = t;
        } else if (t != v.tail_term) {
            rg_follow_push_run(v, v.tail_first, v.tail_term);
            v.tail_first = v.last + 1;
            v.tail_term = t;
        }
        v.last += cnt;
    }
}

RG_D rg_follow_resp rg_follow_answer(u32 status, u64 index, u64 commit) {
    rg_follow_resp r;
    r.index = index;
    r.commit = commit;
    r.conflict = r.reject_hint = r.log_term = 0;
    r.status = status;
    r.reserved = 0;
    return r;
}

// Raft::handle_heartbeat (raft.rs:2452-2464): commit_to(m.commit)
RG_D rg_follow_resp rg_follow_heartbeat(RgFollowView &v, const RgFollowRec &m) {
    if (m.commit > v.committed) {
        if (m.commit > v.last) return rg_follow_answer(RG_FOLLOW_FAULT, m.index, v.committed); // raft_log.rs:291-298
        v.committed = m.commit;
    }
    return rg_follow_answer(RG_FOLLOW_HEARTBEAT, 0, v.committed);
}

// Raft::handle_append_entries from raft.rs:2394 on, in the reference's order of evaluation: the first comparison the gap leaves
// open hands the record back, a fault found before it is a fault. Nothing of `v` changes before every check has passed.
RG_D rg_follow_resp rg_follow_append(RgFollowView &v, const RgFollowRec &m) {
    const u64 lim = 1ULL << 63;
    u64 n = 0;
    for (u32 j = 0; j <= m.n_ext; j++) n += rg_follow_run_count(m, j); // (<= 256 runs of < 2^32: no wrap)
    if (m.index >= lim || n >= lim - m.index) return rg_follow_answer(RG_FOLLOW_FAULT, m.index, v.committed);
    if (m.index < v.committed) return rg_follow_answer(RG_FOLLOW_STALE, v.committed, v.committed); // raft.rs:2394-2406
    // match_term(m.index, m.log_term) (raft_log.rs:238); m.index >= committed >= the dummy entry
    const RgFollowSeg at = rg_follow_seg(v, m.index);
    if (m.log_term >= at.lo && m.log_term <= at.hi && at.lo != at.hi) return rg_follow_answer(RG_FOLLOW_HOST, m.index, v.committed);
    if (m.log_term != at.lo || at.lo != at.hi) {
        // reject (raft.rs:2429-2444): find_conflict_by_term(min(index, last_index), log_term), a stretch per round
        u64 ci = m.index < v.last ? m.index : v.last;
        RgFollowSeg s;
        for (;;) {
            s = rg_follow_seg(v, ci);
            if (s.hi <= m.log_term) break;     // term(ci) <= term whatever it is: the walk stops here
            if (s.lo <= m.log_term) return rg_follow_answer(RG_FOLLOW_HOST, m.index, v.committed);
            ci = s.start - 1;                  // every term of the stretch is above: the reference steps below it
        }
        if (s.lo != s.hi) return rg_follow_answer(RG_FOLLOW_HOST, m.index, v.committed); // log_term = term(reject_hint) is needed
        rg_follow_resp r = rg_follow_answer(RG_FOLLOW_REJECT, m.index, v.committed);
        r.reject_hint = ci;
        r.log_term = s.lo;
        return r;
    }
    // find_conflict (raft_log.rs:182-198), run by run
    u64 conflict = 0, rem = 0, i = m.index + 1;
    u32 j = 0;
    for (; j <= m.n_ext && !conflict; j++) {
        const u64 cnt = rg_follow_run_count(m, j);
        if (cnt == 0) continue;
        const u64 t = rg_follow_run_term(m, j), b = i + cnt - 1;
        while (i <= b) {
            const RgFollowSeg s = rg_follow_seg(v, i);
            if (s.lo == s.hi && s.lo == t) {
                i = (s.end < b ? s.end : b) + 1;
            } else if (t < s.lo || t > s.hi) {
                conflict = i;
                rem = b - i + 1;
                break;
            } else {
                return rg_follow_answer(RG_FOLLOW_HOST, m.index, v.committed);
            }
        }
        if (conflict) break;
    }
    u64 new_last = v.last;
    if (conflict) {
        if (conflict <= v.committed) return rg_follow_answer(RG_FOLLOW_FAULT, m.index, v.committed); // raft_log.rs:259-265
        if (conflict > v.last + 1) return rg_follow_answer(RG_FOLLOW_FAULT, m.index, v.committed);   // a hole: log_unstable.rs:169
        u64 prev = rg_follow_run_term(m, j);
        for (u32 r = j + 1; r <= m.n_ext; r++) {
            if (rg_follow_run_count(m, r) == 0) continue;
            const u64 t = rg_follow_run_term(m, r);
            if (t < prev) return rg_follow_answer(RG_FOLLOW_FAULT, m.index, v.committed); // the entries' terms decrease
            prev = t;
        }
        const RgFollowSeg below = rg_follow_seg(v, conflict - 1);
        const u64 t0 = rg_follow_run_term(m, j);
        if (t0 < below.lo) return rg_follow_answer(RG_FOLLOW_FAULT, m.index, v.committed); // ... or start below the log's
        if (t0 < below.hi) return rg_follow_answer(RG_FOLLOW_HOST, m.index, v.committed);
        new_last = m.index + n;
    }
    const u64 to_commit = m.commit < m.index + n ? m.commit : m.index + n;
    if (to_commit > v.committed && to_commit > new_last) return rg_follow_answer(RG_FOLLOW_FAULT, m.index, v.committed); // :291-298
    if (conflict) rg_follow_cut_append(v, m, conflict, j, rem);
    if (to_commit > v.committed) v.committed = to_commit;
    rg_follow_resp r = rg_follow_answer(RG_FOLLOW_ACCEPT, m.index + n, v.committed);
    r.conflict = conflict;
    return r;
}

// One record on one group. flags is exactly one kind (the callers have checked).
RG_D rg_follow_resp rg_follow_apply(RgFollowView &v, const RgFollowRec &m) {
    return (m.flags & RG_FOLLOW_MSG_APPEND) ? rg_follow_append(v, m) : rg_follow_heartbeat(v, m);
}

// ---- whole group states (rg_follow_write / rg_follow_read) ----
// Is `s` canonical (include/raftgroups.h)? 0 = yes, else which rule it breaks (for the message).
RG_FOLLOW_HD int rg_follow_state_check(const rg_follow_state &s) {
    if (s.n_runs > RG_FOLLOW_RUNS) return 1;
    if (s.last_index >= (1ULL << 63)) return 2;
    if (s.committed > s.last_index || s.committed < s.dummy_index || s.last_index < s.dummy_index) return 3;
    if (s.dummy_index == 0 && s.dummy_term != 0) return 4;
    if ((s.n_runs == 0) != (s.last_index == s.dummy_index)) return 5;
    // (a loop of constant length over constant indices: in a kernel -- the hand-off's demotion -- the state stays in registers)
    u64 prev_first = s.dummy_index, prev_term = s.dummy_term;
    int rule = 0; // the first one broken, runs in ascending order
    RG_FOLLOW_UNROLL
    for (u32 k = 0; k < RG_FOLLOW_RUNS; k++) {
        if (k < s.n_runs) {
            if (!rule && s.run_first[k] <= prev_first) rule = 6;
            if (!rule && (k == 0 ? s.run_term[0] < prev_term : s.run_term[k] <= prev_term)) rule = 7;
            prev_first = s.run_first[k];
            prev_term = s.run_term[k];
        }
    }
    if (rule) return rule;
    if (s.n_runs && prev_first > s.last_index) return 8;
    return 0;
}
RG_D void rg_follow_store_state(const RgFollowCols &c, const rg_follow_state &s) {
    const u64 g = s.group;
    c.committed[g] = s.committed;
    c.last[g] = s.last_index;
    c.dummy_idx[g] = s.dummy_index;
    c.dummy_term[g] = s.dummy_term;
    const u32 n_old = s.n_runs ? s.n_runs - 1 : 0;
    c.n_old[g] = (u8)n_old;
    c.tail_first[g] = s.n_runs ? s.run_first[n_old] : s.last_index + 1;
    c.tail_term[g] = s.n_runs ? s.run_term[n_old] : s.dummy_term;
    for (u32 k = 0; k < RG_TERM_RUNS; k++) {
        c.run_first[(u64)k * c.stride + g] = k < n_old ? s.run_first[k] : 0;
        c.run_term[(u64)k * c.stride + g] = k < n_old ? s.run_term[k] : 0;
    }
}
RG_D rg_follow_state rg_follow_load_state(const RgFollowCols &c, u64 g) {
    rg_follow_state s;
    s.group = g;
    s.committed = c.committed[g];
    s.last_index = c.last[g];
    s.dummy_index = c.dummy_idx[g];
    s.dummy_term = c.dummy_term[g];
    s.reserved = 0;
    const u32 n_old = c.n_old[g];
    const bool tail = c.tail_first[g] <= s.last_index;
    s.n_runs = tail ? n_old + 1 : 0;
    for (u32 k = 0; k < RG_FOLLOW_RUNS; k++) {
        const bool old = tail && k < n_old;
        s.run_first[k] = old ? c.run_first[(u64)k * c.stride + g] : (tail && k == n_old) ? c.tail_first[g] : 0;
        s.run_term[k] = old ? c.run_term[(u64)k * c.stride + g] : (tail && k == n_old) ? c.tail_term[g] : 0;
    }
    return s;
}

// ---- the term gate, the vote step and the election clock (include/raftgroups.h: "The follower's term gate ...") ----
// Restated from Raft::step (src/raft.rs:1282-1411 the gate, :1418-1461 the vote step), reset / become_follower (:942-971,
// :1082-1087), step_candidate / step_follower (:2215-2229, :2271-2285), tick_election (:1024-1047), maybe_commit_by_vote
// (:2126-2164), RaftLog::is_up_to_date / maybe_commit / commit_info (src/raft_log.rs:412, :487, :637).
struct RgGateCfg {
    u32 election_tick, min_timeout, max_timeout, flags;
    u64 seed;
};
// The soft columns, F = stride groups each. HOT: term, lead, clock. COLD: vote, priority, role.
struct RgSoftCols {
    u64 *term, *lead;
    u32 *clock; // election_elapsed | promotable << 15 | randomized_election_timeout << 16
    u64 *vote;
    int64_t *priority;
    u8 *role;
    RgGateCfg cfg;
};
#define RG_CLOCK_ELAPSED_MAX 0x7fffu
RG_D u32 rg_clock_elapsed(u32 c) { return c & RG_CLOCK_ELAPSED_MAX; }
RG_D u32 rg_clock_promotable(u32 c) { return (c >> 15) & 1u; }
RG_D u32 rg_clock_timeout(u32 c) { return c >> 16; }
RG_D u32 rg_clock_pack(u32 elapsed, u32 promotable, u32 timeout) { return elapsed | (promotable << 15) | (timeout << 16); }

RG_D u64 rg_follow_mix(u64 z) { // splitmix64's step
    z += 0x9e3779b97f4a7c15ULL;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}
// reset_randomized_election_timeout (raft.rs:2744-2756): a value of [min, max), from the seed, the group, the term after the
// reset and the timeout it replaces
RG_D u32 rg_follow_draw(u64 seed, u64 group, u64 term, u32 prev, u32 min, u32 max) {
    const u64 x = rg_follow_mix(rg_follow_mix(rg_follow_mix(seed ^ group) ^ term) ^ prev);
    return min + (u32)(x >> 32) % (max - min);
}

// One group's soft state while a lane works on it: the hot cells by value, the cold ones loaded on first use and written back
// only where a record changed them (`have`: 1 vote loaded, 2 role loaded, 4 vote to be stored, 8 role to be stored).
struct RgSoftView {
    u64 term, lead, vote;
    u32 clock, role, have;
    const u64 *pvote;
    const int64_t *ppriority;
    const u8 *prole;
};
RG_D RgSoftView rg_soft_open(const RgSoftCols &c, u64 g) {
    RgSoftView s;
    s.term = c.term[g];
    s.lead = c.lead[g];
    s.clock = c.clock[g];
    s.vote = 0;
    s.role = 0;
    s.have = 0;
    s.pvote = c.vote + g;
    s.ppriority = c.priority + g;
    s.prole = c.role + g;
    return s;
}
RG_D void rg_soft_close(const RgSoftCols &c, u64 g, const RgSoftView &s, const RgSoftView &o) {
    if (s.term != o.term) c.term[g] = s.term;
    if (s.lead != o.lead) c.lead[g] = s.lead;
    if (s.clock != o.clock) c.clock[g] = s.clock;
    if (s.have & 4u) c.vote[g] = s.vote;
    if (s.have & 8u) c.role[g] = (u8)s.role;
}
RG_D u64 rg_soft_vote(RgSoftView &s) {
    if (!(s.have & 1u)) {
        s.vote = *s.pvote;
        s.have |= 1u;
    }
    return s.vote;
}
RG_D u32 rg_soft_role(RgSoftView &s) {
    if (!(s.have & 2u)) {
        s.role = *s.prole;
        s.have |= 2u;
    }
    return s.role;
}
RG_D void rg_soft_set_vote(RgSoftView &s, u64 vote) {
    s.vote = vote;
    s.have |= 5u;
}
RG_D void rg_soft_set_elapsed(RgSoftView &s, u32 elapsed) { s.clock = (s.clock & ~RG_CLOCK_ELAPSED_MAX) | elapsed; }

// become_follower(term, lead) (raft.rs:1082-1087) = reset(term) (:942-971) as far as a non-leader has the state
RG_D void rg_gate_become_follower(const RgGateCfg &cfg, u64 g, RgSoftView &s, u64 term, u64 lead, u32 &events) {
    if (s.term != term) {
        s.term = term;
        rg_soft_set_vote(s, 0);
    }
    s.lead = lead;
    const u32 timeout = rg_follow_draw(cfg.seed, g, s.term, rg_clock_timeout(s.clock), cfg.min_timeout, cfg.max_timeout);
    s.clock = rg_clock_pack(0, rg_clock_promotable(s.clock), timeout);
    if (rg_soft_role(s) != 0) {
        events |= RG_GATE_EV_BECAME_FOLLOWER;
        s.role = 0;
        s.have |= 8u;
    }
}

// A well-formed gated record? (what the dense kernel answers FAULT to and the sparse call refuses on the host)
RG_FOLLOW_HD bool rg_gate_well_formed(u32 kind, u64 term, u64 from, u32 n_entries, u32 n_ext, bool votes) {
    const u32 steps = RG_FOLLOW_MSG_APPEND | RG_FOLLOW_MSG_HEARTBEAT | RG_FOLLOW_MSG_TOUCH, vote_kinds = RG_FOLLOW_MSG_VOTE | RG_FOLLOW_MSG_PREVOTE;
    if (kind == 0 || (kind & (kind - 1)) != 0 || term == 0 || from == 0) return false;
    if (kind & steps) return true;
    return votes && (kind & vote_kinds) != 0 && n_entries == 0 && n_ext == 0;
}

RG_D rg_follow_gate_resp rg_gate_answer(u64 term, u32 gate, u32 events) {
    rg_follow_gate_resp a;
    a.term = term;
    a.gate = gate;
    a.events = events;
    return a;
}

// One well-formed record through the gate and its step. `r` is the step's answer (status 0 where no log step ran). Nothing
// of `s` or `v` changes where the answer is IGNORED / STALE_LEADER / PREVOTE_LOW or the status is FAULT / HOST.
RG_D rg_follow_gate_resp rg_gate_step(const RgGateCfg &cfg, u64 g, RgSoftView &s, RgFollowView &v, const RgFollowRec &m, u64 m_term, u64 from,
                                      int64_t m_priority, u32 hdr_flags, rg_follow_resp &r) {
    const u32 kind = m.flags;
    const bool vote_kind = (kind & (RG_FOLLOW_MSG_VOTE | RG_FOLLOW_MSG_PREVOTE)) != 0;
    const RgSoftView s0 = s;
    const u64 committed0 = v.committed;
    u32 events = 0;
    r = rg_follow_answer(RG_FOLLOW_NONE, m.index, v.committed);
    if (m_term > s.term) {
        if (vote_kind) {
            const bool in_lease = (cfg.flags & RG_GATE_CHECK_QUORUM) && s.lead != 0 && rg_clock_elapsed(s.clock) < cfg.election_tick;
            if (!(hdr_flags & RG_GATE_FORCE) && in_lease) return rg_gate_answer(s.term, RG_GATE_IGNORED, 0);
        }
        if (kind != RG_FOLLOW_MSG_PREVOTE) rg_gate_become_follower(cfg, g, s, m_term, kind == RG_FOLLOW_MSG_VOTE ? 0 : from, events);
    } else if (m_term < s.term) {
        if ((cfg.flags & (RG_GATE_CHECK_QUORUM | RG_GATE_PRE_VOTE)) && (kind & (RG_FOLLOW_MSG_APPEND | RG_FOLLOW_MSG_HEARTBEAT)))
            return rg_gate_answer(s.term, RG_GATE_STALE_LEADER, 0);
        return rg_gate_answer(s.term, kind == RG_FOLLOW_MSG_PREVOTE ? RG_GATE_PREVOTE_LOW : RG_GATE_IGNORED, 0);
    }
    u32 gate = RG_GATE_PASS;
    u64 resp_term = s.term;
    bool undone = false;
    if (vote_kind) {
        const bool can_vote = rg_soft_vote(s) == from || (s.vote == 0 && s.lead == 0) || (kind == RG_FOLLOW_MSG_PREVOTE && m_term > s.term);
        bool grant = can_vote;
        if (grant) { // is_up_to_date(m.index, m.log_term) (raft_log.rs:412); the last entry is the tail's or the dummy entry
            const RgFollowSeg lt = rg_follow_seg(v, v.last);
            if (lt.lo != lt.hi) undone = true;
            else grant = m.log_term > lt.lo || (m.log_term == lt.lo && m.index >= v.last);
        }
        if (grant && !undone) grant = m.index > v.last || *s.ppriority <= m_priority;
        if (undone) {
        } else if (grant) {
            gate = RG_GATE_VOTE_GRANT;
            resp_term = m_term;
            if (kind == RG_FOLLOW_MSG_VOTE) { // only real votes are recorded
                rg_soft_set_elapsed(s, 0);
                if (s.vote != from) events |= RG_GATE_EV_HARD_STATE;
                rg_soft_set_vote(s, from);
            }
        } else {
            gate = RG_GATE_VOTE_REJECT;
            const RgFollowSeg ct = rg_follow_seg(v, v.committed); // commit_info (raft_log.rs:637)
            if (ct.lo != ct.hi) undone = true;
            else {
                r.log_term = ct.lo;
                // maybe_commit_by_vote (raft.rs:2126-2164) -> RaftLog::maybe_commit(m.commit, m.commit_term)
                if (m.commit != 0 && m.ent_term != 0 && m.commit > v.committed) {
                    const RgFollowSeg at = rg_follow_seg(v, m.commit);
                    if (at.lo != at.hi && m.ent_term >= at.lo && m.ent_term <= at.hi) undone = true;
                    else if (at.lo == at.hi && at.lo == m.ent_term) {
                        v.committed = m.commit; // (term(m.commit) != 0: m.commit <= last_index)
                        if (rg_soft_role(s) != 0) events |= RG_GATE_EV_CONF_CHECK;
                    }
                }
            }
        }
    } else {
        // step_candidate (raft.rs:2215-2229): role != Follower implies lead == 0, so a group with a leader skips the role cell
        if (s.lead == 0 && rg_soft_role(s) != 0) rg_gate_become_follower(cfg, g, s, m_term, from, events);
        rg_soft_set_elapsed(s, 0); // step_follower (:2271-2285)
        s.lead = from;
        if (kind != RG_FOLLOW_MSG_TOUCH) {
            r = rg_follow_apply(v, m);
            undone = r.status == RG_FOLLOW_FAULT || r.status == RG_FOLLOW_HOST;
        }
    }
    if (undone) {
        s = s0;
        v.committed = committed0;
        if (r.status != RG_FOLLOW_FAULT) r = rg_follow_answer(RG_FOLLOW_HOST, m.index, v.committed);
        return rg_gate_answer(s.term, RG_GATE_PASS, 0);
    }
    if (s.term != s0.term || v.committed != committed0) events |= RG_GATE_EV_HARD_STATE;
    if (s.lead != s0.lead) events |= RG_GATE_EV_LEADER_CHANGED;
    return rg_gate_answer(resp_term, gate, events);
}

// Raft::tick of a non-leader (raft.rs:1024-1047) on the clock cell: the new cell if the group does not fire, and whether it is
// due. A due group's election_elapsed becomes 0 only if its hup is delivered (the caller decides).
RG_D u32 rg_clock_tick(u32 c, bool &due) {
    u32 e = rg_clock_elapsed(c);
    if (e < RG_CLOCK_ELAPSED_MAX) e++;
    due = e >= rg_clock_timeout(c) && rg_clock_promotable(c);
    return (c & ~RG_CLOCK_ELAPSED_MAX) | e;
}

// ---- rg_follow_soft_write / rg_follow_soft_read ----
// 0 = acceptable, else which rule it breaks
RG_FOLLOW_HD int rg_follow_soft_check(const rg_follow_soft &w, u32 min_timeout, u32 max_timeout) {
    if (w.role > 2) return 1;
    if (w.role != 0 && w.leader_id != 0) return 2;
    if (w.randomized_timeout != 0 && (w.randomized_timeout < min_timeout || w.randomized_timeout >= max_timeout)) return 3;
    if (w.election_elapsed > RG_CLOCK_ELAPSED_MAX) return 4;
    if (w.promotable > 1) return 5;
    return 0;
}
RG_D void rg_follow_store_soft(const RgSoftCols &c, const rg_follow_soft &w) {
    const u64 g = w.group;
    u32 timeout = w.randomized_timeout;
    if (timeout == 0) timeout = rg_follow_draw(c.cfg.seed, g, w.term, rg_clock_timeout(c.clock[g]), c.cfg.min_timeout, c.cfg.max_timeout);
    c.term[g] = w.term;
    c.lead[g] = w.leader_id;
    c.clock[g] = rg_clock_pack(w.election_elapsed, w.promotable, timeout);
    c.vote[g] = w.vote;
    c.priority[g] = w.priority;
    c.role[g] = w.role;
}
RG_D rg_follow_soft rg_follow_load_soft(const RgSoftCols &c, u64 g) {
    rg_follow_soft w;
    const u32 k = c.clock[g];
    w.group = g;
    w.term = c.term[g];
    w.vote = c.vote[g];
    w.leader_id = c.lead[g];
    w.priority = c.priority[g];
    w.election_elapsed = rg_clock_elapsed(k);
    w.randomized_timeout = rg_clock_timeout(k);
    w.role = c.role[g];
    w.promotable = (u8)rg_clock_promotable(k);
    for (int i = 0; i < 6; i++) w.reserved[i] = 0;
    return w;
}
