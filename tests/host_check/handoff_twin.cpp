// handoff_twin.cpp -- raft_rs_amd/csrc/rg_handoff.h on the host, alone: the arithmetic the hand-off kernels run between the
// follower arena and the leader columns, driven from stdin and answered on stdout, so that tests/test_handoff_host.py can compare
// it with tests/handoff_model.py (and run it under the sanitizers) without a GPU. Every line is a case of its own: the arena is
// one group wide and written through rg_follow_store_state, read back through rg_follow_load_state.
//
//   P <n_slots> <committed> <last> <dummy> <dummy_term> <n_runs> {<first> <term>}*     the arena's log (rg_follow_write's form)
//     <term> <lead> <self_id> <role> <conf>                                             soft and election cells
//     <cfg> <pflags row> <has_persisted> <persisted>                                    the lead group, the record
//       -> "P <status> <term> <last_index> <commit> <out>", and where the status is DONE, on the same line,
//          " L <commit> <lo> <hi> <cur_term> <dummy> <dummy_term> <run_count> {<first>}*8 {<term>}*8
//            <pflags row> <cfg> <present> <self> <clear_snap> <clear_rs> <next_all>"
//   D <commit> <lo> <hi> <cur_term> <dummy> <dummy_term> <run_count> {<first>}*8 {<term>}*8     the lead group's log columns
//       -> "D <status> <term> <last_index> <commit>", and where the status is DONE
//          " S <committed> <last> <dummy> <dummy_term> <n_runs> {<first> <term>}*" as rg_follow_read would report the arena
//   "W <rule>" alone answers a P line whose log is not canonical (rg_follow_state_check's rule).
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../raft_rs_amd/csrc/rg_handoff.h"

static bool next_u64(u64 &v) { return scanf("%" SCNu64, &v) == 1; }

struct Arena { // one group, stride 1
    u64 committed, last, tail_first, tail_term, dummy_idx, dummy_term, run_first[RG_TERM_RUNS], run_term[RG_TERM_RUNS];
    u8 n_old;
    RgFollowCols cols() {
        RgFollowCols c;
        c.committed = &committed;
        c.last = &last;
        c.tail_first = &tail_first;
        c.tail_term = &tail_term;
        c.dummy_idx = &dummy_idx;
        c.dummy_term = &dummy_term;
        c.run_first = run_first;
        c.run_term = run_term;
        c.n_old = &n_old;
        c.stride = 1;
        c.n = 1;
        return c;
    }
};
// (what rg_handoff_load_log of the kernels does)
static RgHandoffLog load_log(const RgFollowCols &c) {
    RgHandoffLog f;
    f.committed = c.committed[0];
    f.last = c.last[0];
    f.tail_first = c.tail_first[0];
    f.tail_term = c.tail_term[0];
    f.dummy_idx = c.dummy_idx[0];
    f.dummy_term = c.dummy_term[0];
    f.n_old = c.n_old[0];
    for (u32 k = 0; k < RG_TERM_RUNS; k++) {
        f.run_first[k] = c.run_first[k];
        f.run_term[k] = c.run_term[k];
    }
    return f;
}

int main() {
    char op[4];
    while (scanf("%3s", op) == 1) {
        Arena a;
        memset(&a, 0xee, sizeof(a)); // (every cell is written before it is read, or the sanitizers and the model notice)
        RgFollowCols c = a.cols();
        if (op[0] == 'P') {
            u64 P = 0, k = 0;
            rg_follow_state s;
            memset(&s, 0, sizeof(s));
            if (!next_u64(P) || P < 1 || P > 8 || !next_u64(s.committed) || !next_u64(s.last_index) || !next_u64(s.dummy_index) || !next_u64(s.dummy_term) ||
                !next_u64(k) || k > RG_FOLLOW_RUNS)
                return 3;
            s.n_runs = (u32)k;
            for (u32 i = 0; i < s.n_runs; i++)
                if (!next_u64(s.run_first[i]) || !next_u64(s.run_term[i])) return 3;
            RgHandoffWin w;
            u64 role = 0, conf = 0, cfg = 0, pf = 0, has = 0, persisted = 0;
            if (!next_u64(w.term) || !next_u64(w.lead) || !next_u64(w.self_id) || !next_u64(role) || !next_u64(conf) || !next_u64(cfg) || !next_u64(pf) ||
                !next_u64(has) || !next_u64(persisted) || role > 255 || conf > 0xffffffffULL || cfg > 0xffffffffULL)
                return 3;
            w.role = (u32)role;
            w.conf = (u32)conf;
            const int rule = rg_follow_state_check(s);
            if (rule) {
                printf("W %d\n", rule);
                continue;
            }
            rg_follow_store_state(c, s);
            const RgHandoffLog f = load_log(c);
            const u32 status = rg_handoff_promote_check(f, w, (u32)cfg, (u32)P, has ? persisted : f.last);
            if (status != RG_HANDOFF_DONE) {
                printf("P %u 0 0 0 0\n", status);
                continue;
            }
            RgHandoffLead l = rg_handoff_import(f);
            const u64 old_hi = l.hi;
            rg_handoff_become_leader(l, w.term);
            const RgHandoffProgress pr = rg_handoff_progress(pf, (u32)cfg, (u32)P, old_hi);
            const rg_handoff_resp r = rg_handoff_answer(RG_HANDOFF_DONE, w.term, l.hi, l.commit, RG_OUT_BECAME_LEADER | RG_OUT_APPENDED);
            printf("P %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %u", r.status, r.term, r.last_index, r.commit, r.out);
            printf(" L %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %u", l.commit, l.lo, l.hi, l.cur_term, l.dummy_idx, l.dummy_term, l.n_runs);
            for (u32 i = 0; i < RG_TERM_RUNS; i++) printf(" %" PRIu64, l.run_first[i]);
            for (u32 i = 0; i < RG_TERM_RUNS; i++) printf(" %" PRIu64, l.run_term[i]);
            printf(" %" PRIu64 " %u %u %u %u %u %" PRIu64 "\n", pr.pf, pr.cfg, pr.present, pr.self, pr.clear_snap, pr.clear_rs, pr.next_all);
        } else if (op[0] == 'D') {
            RgHandoffLead l;
            u64 n = 0;
            if (!next_u64(l.commit) || !next_u64(l.lo) || !next_u64(l.hi) || !next_u64(l.cur_term) || !next_u64(l.dummy_idx) || !next_u64(l.dummy_term) || !next_u64(n) ||
                n > 255)
                return 4;
            l.n_runs = (u32)n;
            for (u32 i = 0; i < RG_TERM_RUNS; i++)
                if (!next_u64(l.run_first[i])) return 4;
            for (u32 i = 0; i < RG_TERM_RUNS; i++)
                if (!next_u64(l.run_term[i])) return 4;
            rg_follow_state s;
            s.group = 0;
            if (rg_handoff_demote(l, s) != RG_HANDOFF_DONE) {
                printf("D %u 0 0 0\n", RG_HANDOFF_FAULT);
                continue;
            }
            const RgHandoffLog f = rg_handoff_export(s);
            a.committed = f.committed;
            a.last = f.last;
            a.tail_first = f.tail_first;
            a.tail_term = f.tail_term;
            a.dummy_idx = f.dummy_idx;
            a.dummy_term = f.dummy_term;
            a.n_old = (u8)f.n_old;
            for (u32 i = 0; i < RG_TERM_RUNS; i++) {
                a.run_first[i] = f.run_first[i];
                a.run_term[i] = f.run_term[i];
            }
            const rg_follow_state t = rg_follow_load_state(c, 0);
            printf("D %u %" PRIu64 " %" PRIu64 " %" PRIu64, RG_HANDOFF_DONE, l.cur_term, l.hi, l.commit);
            printf(" S %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %u", t.committed, t.last_index, t.dummy_index, t.dummy_term, t.n_runs);
            for (u32 i = 0; i < t.n_runs; i++) printf(" %" PRIu64 " %" PRIu64, t.run_first[i], t.run_term[i]);
            printf("\n");
        } else {
            return 6;
        }
    }
    return 0;
}
