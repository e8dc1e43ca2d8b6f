// follow_twin.cpp -- raft_rs_amd/csrc/rg_follow.h on the host, alone: the per-group arithmetic the follower kernels run, driven
// from stdin and answered on stdout, so that tests/test_follower_host.py can compare it with tests/follower_model.py (and run it
// under the sanitizers) without a GPU.
//
//   N <n_follow>                                           first line: the arena (stride = n_follow rounded up to 256)
//   W <g> <committed> <last> <dummy> <dummy_term> <n_runs> {<first> <term>}*     rg_follow_write of one state  -> "W <rule>"
//   A <g> <index> <log_term> <commit> <n_runs> {<term> <count>}*                 a MsgAppend (run 0 is the inline one)
//   H <g> <commit>                                                               a MsgHeartbeat
//         -> "R <status> <index> <commit> <conflict> <reject_hint> <log_term>"
//   S <g>                                                                        rg_follow_read of one group
//         -> "S <committed> <last> <dummy> <dummy_term> <n_runs> {<first> <term>}*"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../raft_rs_amd/csrc/rg_follow.h"

static bool next_u64(u64 &v) { return scanf("%" SCNu64, &v) == 1; }

int main() {
    char op[4];
    u64 n = 0;
    if (scanf("%3s", op) != 1 || op[0] != 'N' || !next_u64(n) || n == 0 || n > (1u << 24)) return 2;
    const u64 stride = (n + 255) & ~255ULL;
    std::vector<u64> committed(stride), last(stride), tail_first(stride, 1), tail_term(stride), dummy_idx(stride), dummy_term(stride);
    std::vector<u64> run_first(RG_TERM_RUNS * stride), run_term(RG_TERM_RUNS * stride);
    std::vector<u8> n_old(stride);
    RgFollowCols c;
    c.committed = committed.data();
    c.last = last.data();
    c.tail_first = tail_first.data();
    c.tail_term = tail_term.data();
    c.dummy_idx = dummy_idx.data();
    c.dummy_term = dummy_term.data();
    c.run_first = run_first.data();
    c.run_term = run_term.data();
    c.n_old = n_old.data();
    c.stride = stride;
    c.n = n;
    std::vector<rg_follow_ent_run> ext;
    while (scanf("%3s", op) == 1) {
        u64 g = 0;
        if (!next_u64(g) || g >= n) return 3;
        if (op[0] == 'W') {
            rg_follow_state s;
            memset(&s, 0, sizeof(s));
            u64 k = 0;
            s.group = g;
            if (!next_u64(s.committed) || !next_u64(s.last_index) || !next_u64(s.dummy_index) || !next_u64(s.dummy_term) || !next_u64(k)) return 4;
            if (k > RG_FOLLOW_RUNS) return 4;
            s.n_runs = (u32)k;
            for (u32 i = 0; i < s.n_runs; i++)
                if (!next_u64(s.run_first[i]) || !next_u64(s.run_term[i])) return 4;
            const int rule = rg_follow_state_check(s);
            if (!rule) rg_follow_store_state(c, s);
            printf("W %d\n", rule);
        } else if (op[0] == 'A' || op[0] == 'H') {
            RgFollowRec m;
            memset(&m, 0, sizeof(m));
            ext.clear();
            if (op[0] == 'A') {
                u64 k = 0, cnt = 0;
                m.flags = RG_FOLLOW_MSG_APPEND;
                if (!next_u64(m.index) || !next_u64(m.log_term) || !next_u64(m.commit) || !next_u64(k) || k < 1 || k > 256) return 5;
                if (!next_u64(m.ent_term) || !next_u64(cnt) || cnt > 0xffffffffULL) return 5;
                m.n_entries = (u32)cnt;
                for (u64 i = 1; i < k; i++) {
                    rg_follow_ent_run r;
                    r.reserved = 0;
                    if (!next_u64(r.term) || !next_u64(cnt) || cnt > 0xffffffffULL) return 5;
                    r.count = (u32)cnt;
                    ext.push_back(r);
                }
                m.ext = ext.data();
                m.n_ext = (u32)ext.size();
            } else {
                m.flags = RG_FOLLOW_MSG_HEARTBEAT;
                if (!next_u64(m.commit)) return 5;
            }
            RgFollowView v = rg_follow_open(c, g);
            const RgFollowView o = v;
            const rg_follow_resp r = rg_follow_apply(v, m);
            rg_follow_close(c, g, v, o);
            printf("R %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", r.status, r.index, r.commit, r.conflict, r.reject_hint,
                   r.log_term);
        } else if (op[0] == 'S') {
            const rg_follow_state s = rg_follow_load_state(c, g);
            printf("S %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %u", s.committed, s.last_index, s.dummy_index, s.dummy_term, s.n_runs);
            for (u32 i = 0; i < s.n_runs; i++) printf(" %" PRIu64 " %" PRIu64, s.run_first[i], s.run_term[i]);
            printf("\n");
        } else {
            return 6;
        }
    }
    return 0;
}
