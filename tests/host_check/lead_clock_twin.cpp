// lead_clock_twin.cpp -- raft_rs_amd/csrc/rg_lead.h on the host, alone: the arithmetic of the leader's clock and of the step-down
// into the follower arena, driven from stdin and answered on stdout, so that tests/test_lead_clock_host.py can compare it with
// tests/lead_clock_model.py (and run it under the sanitizers) without a GPU. Every line is a case of its own.
//
//   T <election_tick> <heartbeat_tick> <flags> <cell> <tag> <cur_term> <cfg> <pflags row> <P> <commit> {<matched>}*8
//       -> "T <events> <cell> <tag> <cfg> <pflags row> {<hb_commit>}*8"   (rg_lead_tick; the commits of the cfg word afterwards)
//   C <election_tick> <heartbeat_tick> <flags> <reserved>                 -> "C <rule>"   (rg_lead_config_check)
//   W <election_tick> <heartbeat_tick> <election_elapsed> <heartbeat_elapsed> <led> {<reserved>}*7
//       -> "W <rule>", and for rule 0 " <cell> <election_elapsed> <heartbeat_elapsed> <led>" through rg_lead_cell_of / rg_lead_record
//   X <cell> <tag> <cur_term>                                            -> "X <cell>"   (rg_lead_stop: the lead group's cell after a step-down)
//   R <cur_term>                                                         -> "R <stamp> <stamp != cur_term>"   (rg_lead_read_stamp: the term
//       cell of the group's ReadIndex queue after a step-down)
//   S <role> <leader_id> <self_id> <term> <clock> <seed> <min> <max> <group>
//     <commit> <lo> <hi> <cur_term> <dummy> <dummy_term> <run_count> {<first>}*8 {<term>}*8       soft cells; the lead group's log
//       -> "S <status>", and for DONE " <term> <last_index> <commit> <leader_id> <clock> <stored>" (stored: the cells rg_soft_close
//          would write, 1 term | 2 lead | 4 clock | 8 vote | 16 role)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../raft_rs_amd/csrc/rg_lead.h"

static bool next_u64(u64 &v) { return scanf("%" SCNu64, &v) == 1; }
static u64 need() {
    u64 v = 0;
    if (!next_u64(v)) {
        fprintf(stderr, "short line\n");
        exit(2);
    }
    return v;
}

int main() {
    char kind[8];
    while (scanf("%7s", kind) == 1) {
        if (kind[0] == 'T') {
            RgLeadCfg lc;
            lc.election_tick = (u32)need();
            lc.heartbeat_tick = (u32)need();
            lc.flags = (u32)need();
            u32 cell = (u32)need();
            u64 tag = need();
            const u64 cur_term = need();
            u32 cfg = (u32)need();
            u64 pf = need();
            const u32 P = (u32)need();
            const u64 commit = need();
            u64 m[8];
            for (int k = 0; k < 8; k++) m[k] = need();
            const u32 ev = rg_lead_tick(lc, cell, tag, cur_term, cfg, pf);
            printf("T %u %u %" PRIu64 " %u %" PRIu64, ev, cell, tag, cfg, pf);
            for (u32 k = 0; k < 8; k++) printf(" %" PRIu64, k < P ? rg_lead_hb_commit(cfg, k, m[k], commit) : 0);
            printf("\n");
        } else if (kind[0] == 'C') {
            const u32 et = (u32)need(), ht = (u32)need(), flags = (u32)need(), reserved = (u32)need();
            printf("C %d\n", rg_lead_config_check(et, ht, flags, reserved));
        } else if (kind[0] == 'W') {
            RgLeadCfg lc;
            lc.election_tick = (u32)need();
            lc.heartbeat_tick = (u32)need();
            lc.flags = 0;
            rg_lead_clock_cell w;
            memset(&w, 0, sizeof(w));
            w.election_elapsed = (u32)need();
            w.heartbeat_elapsed = (u32)need();
            w.led = (uint8_t)need();
            for (int k = 0; k < 7; k++) w.reserved[k] = (uint8_t)need();
            const int rule = rg_lead_cell_check(lc, w);
            printf("W %d", rule);
            if (!rule) {
                const u32 cell = rg_lead_cell_of(w);
                const rg_lead_clock_cell r = rg_lead_record(3, 4, cell);
                printf(" %u %u %u %u", cell, r.election_elapsed, r.heartbeat_elapsed, (u32)r.led);
            }
            printf("\n");
        } else if (kind[0] == 'X') {
            const u32 cell = (u32)need();
            const u64 tag = need(), cur_term = need();
            printf("X %u\n", rg_lead_stop(cell, tag, cur_term));
        } else if (kind[0] == 'R') {
            const u64 cur_term = need(), stamp = rg_lead_read_stamp(cur_term);
            printf("R %" PRIu64 " %d\n", stamp, stamp != cur_term ? 1 : 0);
        } else if (kind[0] == 'S') {
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
            u32 status = rg_lead_step_down_check(w, l.cur_term);
            rg_follow_state fs;
            fs.group = group;
            if (status == RG_HANDOFF_DONE && rg_handoff_demote(l, fs) != RG_HANDOFF_DONE) status = RG_HANDOFF_FAULT;
            printf("S %u", status);
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
                rg_lead_step_down_soft(gc, group, s);
                const u32 stored = (s.term != o.term ? 1u : 0u) | (s.lead != o.lead ? 2u : 0u) | (s.clock != o.clock ? 4u : 0u) | ((s.have & 4u) ? 8u : 0u) |
                                   ((s.have & 8u) ? 16u : 0u);
                printf(" %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %u", l.cur_term, l.hi, l.commit, s.lead, s.clock, stored);
            }
            printf("\n");
        } else {
            fprintf(stderr, "unknown line %s\n", kind);
            return 2;
        }
    }
    return 0;
}
