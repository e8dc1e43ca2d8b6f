// vote_twin.cpp -- raft_rs_amd/csrc/rg_vote.h on the host, alone: the per-record arithmetic of the dense vote step, composed as
// rg_kernels_vote.h composes it (the win state, then rg_gate_step on the arena's views or rg_vote_led_group on the leader's values,
// then the stores), driven from stdin and answered on stdout, so that tests/test_vote_step_host.py can compare it with
// tests/vote_step_model.py (and run it under the sanitizers) without a GPU. Every line is a case of its own.
//
//   V <has_lead> <clock_on>  <kind> <m.term> <from> <index> <log_term> <commit> <commit_term> <priority> <hdr flags>
//     <gate flags> <election_tick> <min> <max> <seed> <group>  <term> <leader_id> <vote> <priority> <role> <clock> <self_id>
//     <cell> <tag> <cfg word>  <commit> <lo> <hi> <cur_term> <dummy> <dummy_term> <run_count> {<first>}*8 {<term>}*8
//     <committed> <last> <dummy> <dummy_term> <n_runs> {<first>}*9 {<term>}*9                        (the arena's log)
//       -> "V <status> <gate> <events> <term> <commit> <log_term> <last_index> <deposed>  <term> <leader_id> <vote> <role> <clock>
//           <cell> <tag> <cfg word>  <committed> <last> <dummy> <dummy_term> <n_runs> {<first>}*9 {<term>}*9"
//          (the soft cells, the lead-side cells and the arena's log AFTER the record)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../raft_rs_amd/csrc/rg_vote.h"

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
        if (kind[0] != 'V') {
            fprintf(stderr, "unknown line %s\n", kind);
            return 2;
        }
        const bool has_lead = need() != 0, clock_on = need() != 0;
        RgVoteReq m;
        m.kind = (u32)need();
        m.term = need();
        m.from = need();
        m.index = need();
        m.log_term = need();
        m.commit = need();
        m.commit_term = need();
        m.priority = (int64_t)need();
        m.hdr_flags = (u32)need();
        RgGateCfg gc;
        gc.flags = (u32)need();
        gc.election_tick = (u32)need();
        gc.min_timeout = (u32)need();
        gc.max_timeout = (u32)need();
        gc.seed = need();
        const u64 group = need();
        // ---- the arena: one group's cells, columns of stride 1 ----
        u64 c_term = need(), c_lead = need(), c_vote = need();
        int64_t c_priority = (int64_t)need();
        u8 c_role = (u8)need();
        u32 c_clock = (u32)need();
        const u64 self_id = need();
        u32 cell = (u32)need();
        u64 tag = need();
        u32 cfg = (u32)need();
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
        rg_follow_state st;
        memset(&st, 0, sizeof st);
        st.group = 0;
        st.committed = need();
        st.last_index = need();
        st.dummy_index = need();
        st.dummy_term = need();
        st.n_runs = (u32)need();
        for (u32 k = 0; k < RG_FOLLOW_RUNS; k++) st.run_first[k] = need();
        for (u32 k = 0; k < RG_FOLLOW_RUNS; k++) st.run_term[k] = need();
        u64 a_committed, a_last, a_tail_first, a_tail_term, a_dummy_idx, a_dummy_term, a_run_first[RG_TERM_RUNS], a_run_term[RG_TERM_RUNS];
        u8 a_n_old;
        RgFollowCols fc;
        fc.committed = &a_committed;
        fc.last = &a_last;
        fc.tail_first = &a_tail_first;
        fc.tail_term = &a_tail_term;
        fc.dummy_idx = &a_dummy_idx;
        fc.dummy_term = &a_dummy_term;
        fc.run_first = a_run_first;
        fc.run_term = a_run_term;
        fc.n_old = &a_n_old;
        fc.stride = 1;
        fc.n = 1;
        rg_follow_store_state(fc, st);
        RgSoftView s;
        s.term = c_term;
        s.lead = c_lead;
        s.clock = c_clock;
        s.vote = 0;
        s.role = 0;
        s.have = 0;
        s.pvote = &c_vote;
        s.ppriority = &c_priority;
        s.prole = &c_role;
        const RgSoftView so = s;
        // ---- rg_vote_one ----
        rgv_vote_resp a;
        bool depose = false;
        const bool led = has_lead && s.lead == self_id && self_id != 0 && rg_vote_win_state(s.lead, self_id, rg_soft_role(s));
        if (!led) {
            RgFollowView v = rg_follow_open(fc, 0);
            const RgFollowView o = v;
            RgFollowRec r;
            r.index = m.index;
            r.log_term = m.log_term;
            r.commit = m.commit;
            r.ent_term = m.commit_term;
            r.n_entries = 0;
            r.flags = m.kind;
            r.ext = nullptr;
            r.n_ext = 0;
            rg_follow_resp fr;
            const rg_follow_gate_resp ga = rg_gate_step(gc, group, s, v, r, m.term, m.from, m.priority, m.hdr_flags, fr);
            rg_follow_close(fc, 0, v, o);
            a = rg_vote_answer(fr.status, ga.gate, ga.events, ga.term, fr.commit, fr.log_term, v.last);
        } else {
            RgHandoffLog f;
            a = rg_vote_led_group(gc, group, s, l, clock_on, cell, tag, m, f, depose);
            if (depose) { // rg_handoff_store_log, rg_term_store_stop
                a_committed = f.committed;
                a_last = f.last;
                a_tail_first = f.tail_first;
                a_tail_term = f.tail_term;
                a_dummy_idx = f.dummy_idx;
                a_dummy_term = f.dummy_term;
                a_n_old = (u8)f.n_old;
                for (u32 k = 0; k < RG_TERM_RUNS; k++) {
                    a_run_first[k] = f.run_first[k];
                    a_run_term[k] = f.run_term[k];
                }
                if (clock_on) {
                    cell = rg_lead_stop(cell, tag, l.cur_term);
                    tag = l.cur_term;
                }
                if (rg_term_abort_transfer(cfg)) a.events |= RGV_VOTE_EV_TRANSFER_ABORTED;
            }
        }
        if (!led || depose) { // rg_soft_close
            c_term = s.term;
            c_lead = s.lead;
            c_clock = s.clock;
            if (s.have & 4u) c_vote = s.vote;
            if (s.have & 8u) c_role = (u8)s.role;
        } else if (s.term != so.term || s.lead != so.lead || s.clock != so.clock || (s.have & 12u)) {
            fprintf(stderr, "a led group that is not deposed changed its soft view\n");
            return 3;
        }
        const rg_follow_state after = rg_follow_load_state(fc, 0);
        printf("V %u %u %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %d  %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %u  %u %" PRIu64 " %u  %" PRIu64 " %" PRIu64
               " %" PRIu64 " %" PRIu64 " %u",
               a.status, a.gate, a.events, a.term, a.commit, a.log_term, a.last_index, depose ? 1 : 0, c_term, c_lead, c_vote, (u32)c_role, c_clock, cell, tag, cfg,
               after.committed, after.last_index, after.dummy_index, after.dummy_term, after.n_runs);
        for (u32 k = 0; k < RG_FOLLOW_RUNS; k++) printf(" %" PRIu64, after.run_first[k]);
        for (u32 k = 0; k < RG_FOLLOW_RUNS; k++) printf(" %" PRIu64, after.run_term[k]);
        printf("\n");
    }
    return 0;
}
