// term_gate_twin.cpp -- raft_rs_amd/csrc/rg_term.h on the host, alone: the arithmetic of the leader's term gate and of the
// deposition into the follower arena, driven from stdin and answered on stdout, so that tests/test_term_gate_host.py can compare
// it with tests/term_gate_model.py (and run it under the sanitizers) without a GPU. Every line is a case of its own.
//
//   G <P> <cell> <tag> <cur_term> <cfg> <flag row> {<term>}*8
//       -> "G <events> <flag row> <new_term> <stale> <not_led> <cell> <tag> <cfg>"   (rg_term_led, rg_term_gate_row; on DEPOSED the
//          lead-side stop: rg_lead_stop with the tag taking cur_term, rg_term_abort_transfer)
//   D <soft> <new_term> <role> <leader_id> <self_id> <term> <clock> <seed> <min> <max> <group>
//     <commit> <lo> <hi> <cur_term> <dummy> <dummy_term> <run_count> {<first>}*8 {<term>}*8
//       -> "D <status>", and for DONE " <term> <last_index> <commit> <leader_id> <soft term> <clock> <stored>" (stored: the cells
//          rg_soft_close would write, 1 term | 2 lead | 4 clock | 8 vote | 16 role; vote: 0 where stored)
//   N <msg flags> <role> <leader_id> <self_id> <term> <cur_term> <m_term>        -> "N <selected>"   (rg_term_scan_selects)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../raft_rs_amd/csrc/rg_term.h"

static u64 need() {
    u64 v = 0;
    if (scanf("%" SCNu64, &v) != 1) {
        fprintf(stderr, "short line\n");
        exit(2);
    }
    return v;
}

int main() {
    char kind[8];
    while (scanf("%7s", kind) == 1) {
        if (kind[0] == 'G') {
            const u32 P = (u32)need();
            u32 cell = (u32)need();
            u64 tag = need();
            const u64 cur_term = need();
            u32 cfg = (u32)need();
            const u64 row = need();
            u64 t[8];
            for (int k = 0; k < 8; k++) t[k] = need();
            const bool led = rg_term_led(cell, tag, cur_term);
            for (u32 k = 0; k < 8; k++)
                if (!(k < P && led && rg_term_is_record(row, k))) t[k] = 0xDEADDEADDEADDEADULL; // (the kernel does not load these)
            const RgTermGate r = rg_term_gate_row(row, P, led, cur_term, t);
            u32 ev = r.events;
            if (ev & RGT_GATE_EV_DEPOSED) {
                cell = rg_lead_stop(cell, tag, cur_term);
                tag = cur_term;
                ev |= rg_term_abort_transfer(cfg);
            }
            printf("G %u %" PRIu64 " %" PRIu64 " %u %u %u %" PRIu64 " %u\n", ev, r.row, r.new_term, r.n_stale, r.n_not_led, cell, tag, cfg);
        } else if (kind[0] == 'D') {
            const bool soft = need() != 0;
            const u64 new_term = need();
            RgHandoffWin w;
            w.role = (u32)need();
            w.lead = need();
            w.self_id = need();
            w.term = need();
            w.conf = 0;
            const u32 clock = (u32)need();
            RgGateCfg gc;
            gc.seed = need();
            gc.min_timeout = (u32)need();
            gc.max_timeout = (u32)need();
            gc.election_tick = gc.min_timeout;
            gc.flags = 0;
            const u64 group = need();
            RgHandoffLead l;
            l.commit = need();
            l.lo = need();
            l.hi = need();
            l.cur_term = need();
            l.dummy_idx = need();
            l.dummy_term = need();
            l.n_runs = (u32)need();
            for (u32 k = 0; k < RG_TERM_RUNS; k++) l.run_first[k] = need();
            for (u32 k = 0; k < RG_TERM_RUNS; k++) l.run_term[k] = need();
            u32 status = rg_term_depose_check(w, l.cur_term, new_term, soft);
            rg_follow_state fs;
            fs.group = group;
            if (status == RG_HANDOFF_DONE && rg_handoff_demote(l, fs) != RG_HANDOFF_DONE) status = RG_HANDOFF_FAULT;
            printf("D %u", status);
            if (status == RG_HANDOFF_DONE) {
                u64 vote = 77;
                int64_t priority = 0;
                u8 role = (u8)w.role;
                RgSoftView s;
                s.term = w.term;
                s.lead = w.lead;
                s.clock = clock;
                s.vote = 0;
                s.role = w.role;
                s.have = 2u; // (the check loaded the role)
                s.pvote = &vote;
                s.ppriority = &priority;
                s.prole = &role;
                const RgSoftView o = s;
                if (soft) rg_term_depose_soft(gc, group, s, new_term);
                const u32 stored = (s.term != o.term ? 1u : 0u) | (s.lead != o.lead ? 2u : 0u) | (s.clock != o.clock ? 4u : 0u) | ((s.have & 4u) ? 8u : 0u) |
                                   ((s.have & 8u) ? 16u : 0u);
                if ((stored & 8u) && s.vote != 0) {
                    fprintf(stderr, "a stored vote of %" PRIu64 "\n", s.vote);
                    return 3;
                }
                printf(" %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %u", new_term, l.hi, l.commit, s.lead, s.term, s.clock, stored);
            }
            printf("\n");
        } else if (kind[0] == 'N') {
            const u32 flags = (u32)need();
            RgHandoffWin w;
            w.role = (u32)need();
            w.lead = need();
            w.self_id = need();
            w.term = need();
            w.conf = 0;
            const u64 cur_term = need(), m_term = need();
            printf("N %d\n", rg_term_scan_selects(flags, w, cur_term, m_term) ? 1 : 0);
        } else {
            fprintf(stderr, "unknown line %s\n", kind);
            return 2;
        }
    }
    return 0;
}
