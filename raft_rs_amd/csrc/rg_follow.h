// rg_follow.h -- the follower half: the per-group arithmetic of a MsgAppend / MsgHeartbeat step (include/raftgroups.h: "The
// follower half").
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
// sanitizers included) -- nothing below needs the HIP headers.
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
    for (u32 k = 0; k < s.n_runs; k++) {
        if (k == 0 ? s.run_first[0] <= s.dummy_index : s.run_first[k] <= s.run_first[k - 1]) return 6;
        if (k == 0 ? s.run_term[0] < s.dummy_term : s.run_term[k] <= s.run_term[k - 1]) return 7;
    }
    if (s.n_runs && s.run_first[s.n_runs - 1] > s.last_index) return 8;
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
