// promote_send_twin.cpp -- raft_rs_amd/csrc/rg_promote.h (over rg_handoff.h) on the host, alone: the arithmetic the kernels of the
// promotion into an engine with device Inflights run, driven from stdin and answered on stdout, so that
// tests/test_promote_send_host.py can compare it with tests/promote_send_model.py (and run it under the sanitizers) without a GPU.
// Every line is a case of its own: one lead group with its window cells and its row of cumulative entry sizes, stored to as
// rg_promote_send_one / rg_promote_put_items of rg_kernels_promote.h store.
//
//   S <n_slots> <committed> <last> <dummy> <dummy_term> <n_runs> {<first> <term>}*     the arena's log (rg_follow_write's form)
//     <term> <lead> <self_id> <role> <conf>                                             soft and election cells
//     <cfg> <pflags row> <has_persisted> <persisted>                                    the lead group, the record
//     <esz_w> {<cell>}*esz_w                                                            the size row (esz_w 0: no table)
//     {<meta>}*n_slots                                                                  the window cells, start | count << 16
//       -> "S <status> <term> <last_index> <commit> <out>", and where the status is DONE, on the same line,
//          " F <pflags row> <windows> <peers> <n_items> E {<cell>}*esz_w M {<meta>}*n_slots I {<slot> <prev> <last> <n_msgs> <kind>}*n_items"
//   Z <term> <index>  ->  "Z <Entry::compute_size of the empty entry {term, index}>"
//   "W <rule>" alone answers an S line whose log is not canonical.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../raft_rs_amd/csrc/rg_promote.h"

static bool next_u64(u64 &v) { return scanf("%" SCNu64, &v) == 1; }

int main() {
    char op[4];
    while (scanf("%3s", op) == 1) {
        if (op[0] == 'Z') {
            u64 term = 0, index = 0;
            if (!next_u64(term) || !next_u64(index)) return 3;
            printf("Z %u\n", rg_promote_empty_entry_size(term, index));
            continue;
        }
        if (op[0] != 'S') return 6;
        u64 P = 0, k = 0;
        rg_follow_state s;
        memset(&s, 0, sizeof(s));
        if (!next_u64(P) || P < 1 || P > 8 || !next_u64(s.committed) || !next_u64(s.last_index) || !next_u64(s.dummy_index) || !next_u64(s.dummy_term) || !next_u64(k) ||
            k > RG_FOLLOW_RUNS)
            return 3;
        s.n_runs = (u32)k;
        for (u32 i = 0; i < s.n_runs; i++)
            if (!next_u64(s.run_first[i]) || !next_u64(s.run_term[i])) return 3;
        RgHandoffWin w;
        u64 role = 0, conf = 0, cfg = 0, pf = 0, has = 0, persisted = 0, esz_w = 0;
        if (!next_u64(w.term) || !next_u64(w.lead) || !next_u64(w.self_id) || !next_u64(role) || !next_u64(conf) || !next_u64(cfg) || !next_u64(pf) || !next_u64(has) ||
            !next_u64(persisted) || role > 255 || conf > 0xffffffffULL || cfg > 0xffffffffULL || !next_u64(esz_w) || esz_w > 4096 || (esz_w & (esz_w - 1)))
            return 3;
        w.role = (u32)role;
        w.conf = (u32)conf;
        std::vector<u32> esz(esz_w), meta(P); // (exactly as long as the engine's: the sanitizers see an index beyond them)
        for (u64 i = 0; i < esz_w + P; i++) {
            u64 v = 0;
            if (!next_u64(v) || v > 0xffffffffULL) return 3;
            (i < esz_w ? esz[i] : meta[i - esz_w]) = (u32)v;
        }
        const int rule = rg_follow_state_check(s);
        if (rule) {
            printf("W %d\n", rule);
            continue;
        }
        // half 1, as tests/host_check/handoff_twin.cpp runs it: the arena's columns of a canonical state
        RgHandoffLog f;
        const u32 n_old = s.n_runs ? s.n_runs - 1 : 0;
        f.committed = s.committed;
        f.last = s.last_index;
        f.dummy_idx = s.dummy_index;
        f.dummy_term = s.dummy_term;
        f.n_old = n_old;
        f.tail_first = s.n_runs ? s.run_first[n_old] : s.last_index + 1;
        f.tail_term = s.n_runs ? s.run_term[n_old] : s.dummy_term;
        for (u32 i = 0; i < RG_TERM_RUNS; i++) {
            f.run_first[i] = i < n_old ? s.run_first[i] : 0;
            f.run_term[i] = i < n_old ? s.run_term[i] : 0;
        }
        const u32 status = rg_handoff_promote_check(f, w, (u32)cfg, (u32)P, has ? persisted : f.last);
        if (status != RG_HANDOFF_DONE) {
            printf("S %u 0 0 0 0\n", status);
            continue;
        }
        RgHandoffLead l = rg_handoff_import(f);
        const u64 old_hi = l.hi;
        rg_handoff_become_leader(l, w.term);
        const rg_handoff_resp a = rg_handoff_answer(RG_HANDOFF_DONE, w.term, l.hi, l.commit, RG_OUT_BECAME_LEADER | RG_OUT_APPENDED);
        // half 2: the size record
        const u64 hi = a.last_index;
        if (esz_w) {
            const u32 mask = (u32)esz_w - 1u;
            const u32 before = esz[(u32)(hi - 1) & mask];
            esz[(u32)hi & mask] = before + rg_promote_empty_entry_size(a.term, hi);
        }
        // half 3: the windows, the flag row, the items
        const RgHandoffProgress pr = rg_handoff_progress(pf, (u32)cfg, (u32)P, old_hi);
        const RgPromoteSend ps = rg_promote_send(pr.pf, pr.cfg, (u32)P);
        for (u32 i = 0; i < P; i++)
            if ((ps.windows >> i) & 1u) meta[i] = 0;
        printf("S %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %u", a.status, a.term, a.last_index, a.commit, a.out);
        printf(" F %" PRIu64 " %u %u %u E", ps.pf, ps.windows, ps.peers, ps.n_items);
        for (u32 v : esz) printf(" %u", v);
        printf(" M");
        for (u32 v : meta) printf(" %u", v);
        printf(" I");
        for (u32 i = 0; i < P; i++)
            if ((ps.peers >> i) & 1u) printf(" %u %" PRIu64 " %" PRIu64 " 1 %u", i, hi - 1, hi, (unsigned)RG_SEND_APPEND);
        printf("\n");
    }
    return 0;
}
