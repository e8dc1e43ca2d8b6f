// elect_twin.cpp -- raft_rs_amd/csrc/rg_elect.h on the host, alone: the campaign, vote-response and poll arithmetic the
// election kernels run on the three layers of the follower arena, driven from stdin and answered on stdout, so that
// tests/test_follow_elect_host.py can compare it with tests/elect_model.py (and run it under the sanitizers) without a GPU.
//
//   N <n_follow> <election_tick> <min> <max> <flags> <seed>      first line: the arena and rg_follow_gate_config (min, max resolved)
//   W <g> <committed> <last> <dummy> <dummy_term> <n_runs> {<first> <term>}*     rg_follow_write of one state  -> "W <rule>"
//   G <g> <term> <vote> <lead> <priority> <role> <elapsed> <timeout> <promotable>   rg_follow_soft_write        -> "G <rule>"
//   E <g> <self_id> <conf> <yes> <no>                                            rg_follow_elect_write       -> "E <rule>"
//   C <g> <flags> <term> <from>          one rg_follow_campaign_req (RG_CAMPAIGN_*)
//   M <g> <kind> <term> <slot> <reject> <commit> <commit_term>     one rg_follow_vote_rec
//         -> both: "R <result> <events> <term> <req_kind> <targets> <flags> <req_term> <req_index> <req_log_term> <req_commit>
//            <req_commit_term> <status>", or "R malformed"
//   K <cap>                                                  one rg_follow_clock over the arena -> "K <n> {<group>}*"
//   S <g>    rg_follow_read       -> "S <committed> <last> <dummy> <dummy_term> <n_runs> {<first> <term>}*"
//   Q <g>    rg_follow_soft_read  -> "Q <term> <vote> <lead> <priority> <role> <elapsed> <timeout> <promotable>"
//   V <g>    rg_follow_elect_read -> "V <self_id> <conf> <yes> <no>"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../raft_rs_amd/csrc/rg_elect.h"

static bool next_u64(u64 &v) { return scanf("%" SCNu64, &v) == 1; }
static bool next_i64(int64_t &v) { return scanf("%" SCNd64, &v) == 1; }

int main() {
    char op[4];
    u64 n = 0, et = 0, tmin = 0, tmax = 0, flags = 0, seed = 0;
    if (scanf("%3s", op) != 1 || op[0] != 'N' || !next_u64(n) || n == 0 || n > (1u << 24)) return 2;
    if (!next_u64(et) || !next_u64(tmin) || !next_u64(tmax) || !next_u64(flags) || !next_u64(seed)) return 2;
    if (et < 1 || et > 16383 || tmin < et || tmin >= tmax || tmax > 32767) return 2;
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
    std::vector<u64> term(stride), lead(stride), vote(stride);
    std::vector<int64_t> priority(stride);
    std::vector<u32> clock(stride);
    std::vector<u8> role(stride);
    RgSoftCols sc;
    sc.term = term.data();
    sc.lead = lead.data();
    sc.clock = clock.data();
    sc.vote = vote.data();
    sc.priority = priority.data();
    sc.role = role.data();
    sc.cfg.election_tick = (u32)et;
    sc.cfg.min_timeout = (u32)tmin;
    sc.cfg.max_timeout = (u32)tmax;
    sc.cfg.flags = (u32)flags;
    sc.cfg.seed = seed;
    for (u64 g = 0; g < stride; g++) clock[g] = rg_clock_pack(0, 0, rg_follow_draw(seed, g, 0, 0, sc.cfg.min_timeout, sc.cfg.max_timeout)); // k_follow_soft_init
    std::vector<u64> self_id(stride);
    std::vector<u32> conf(stride);
    std::vector<unsigned short> votes(stride);
    RgElectCols ec;
    ec.self_id = self_id.data();
    ec.conf = conf.data();
    ec.votes = votes.data();
    std::vector<u64> hup;
    while (scanf("%3s", op) == 1) {
        u64 g = 0;
        if (!next_u64(g)) return 3;
        if (op[0] == 'K') { // k_follow_clock, lane by lane: a due group beyond the cap is not restarted
            hup.clear();
            for (u64 i = 0; i < n; i++) {
                bool due = false;
                u32 k = rg_clock_tick(clock[i], due);
                if (due && hup.size() < g) {
                    hup.push_back(i);
                    k &= ~RG_CLOCK_ELAPSED_MAX;
                }
                clock[i] = k;
            }
            printf("K %zu", hup.size());
            for (u64 x : hup) printf(" %" PRIu64, x);
            printf("\n");
            continue;
        }
        if (g >= n) return 3;
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
        } else if (op[0] == 'G') {
            rg_follow_soft w;
            memset(&w, 0, sizeof(w));
            u64 r = 0, e = 0, t = 0, p = 0;
            w.group = g;
            if (!next_u64(w.term) || !next_u64(w.vote) || !next_u64(w.leader_id) || !next_i64(w.priority) || !next_u64(r) || !next_u64(e) || !next_u64(t) ||
                !next_u64(p) || r > 255 || p > 255 || e > 0xffffffffULL || t > 0xffffffffULL)
                return 4;
            w.role = (u8)r;
            w.promotable = (u8)p;
            w.election_elapsed = (u32)e;
            w.randomized_timeout = (u32)t;
            const int rule = rg_follow_soft_check(w, sc.cfg.min_timeout, sc.cfg.max_timeout);
            if (!rule) rg_follow_store_soft(sc, w);
            printf("G %d\n", rule);
        } else if (op[0] == 'E') {
            rg_follow_elect w;
            memset(&w, 0, sizeof(w));
            u64 cf = 0, y = 0, no = 0;
            w.group = g;
            if (!next_u64(w.self_id) || !next_u64(cf) || !next_u64(y) || !next_u64(no) || cf > 0xffffffffULL || y > 255 || no > 255) return 4;
            w.conf = (u32)cf;
            w.yes = (u8)y;
            w.no = (u8)no;
            const int rule = rg_follow_elect_check(w);
            if (!rule) rg_follow_store_elect(ec, w);
            printf("E %d\n", rule);
        } else if (op[0] == 'C' || op[0] == 'M') {
            RgElectRec m;
            memset(&m, 0, sizeof(m));
            if (op[0] == 'C') { // as rg_follow_campaign stages a request
                u64 f = 0, t = 0, from = 0;
                if (!next_u64(f) || !next_u64(t) || !next_u64(from) || f > 0xffffffffULL) return 5;
                if (!rg_elect_campaign_well_formed((u32)f, t, from)) {
                    printf("R malformed\n");
                    continue;
                }
                const bool tn = (f & RG_CAMPAIGN_TIMEOUT_NOW) != 0;
                m.term = tn ? t : 0;
                m.from = tn ? from : 0;
                m.kind = tn ? RG_ELECT_K_TIMEOUT_NOW : RG_ELECT_K_HUP;
                m.flags = (f & RG_CAMPAIGN_BLOCKED) ? RG_ELECT_F_BLOCKED : 0u;
            } else { // as rg_follow_vote_resps stages a record
                u64 kind = 0, slot = 0, reject = 0;
                if (!next_u64(kind) || !next_u64(m.term) || !next_u64(slot) || !next_u64(reject) || !next_u64(m.commit) || !next_u64(m.commit_term) || kind > 255 ||
                    slot > 255)
                    return 5;
                if (!rg_elect_resp_well_formed((u32)kind, m.term, (u32)slot)) {
                    printf("R malformed\n");
                    continue;
                }
                m.from = slot;
                m.kind = (u32)kind;
                m.flags = reject ? RG_ELECT_F_REJECT : 0u;
            }
            RgFollowView v = rg_follow_open(c, g);
            RgSoftView s = rg_soft_open(sc, g);
            RgElectView e = rg_elect_open(ec, g);
            const RgFollowView o = v;
            const RgSoftView so = s;
            const RgElectView eo = e;
            const rg_follow_elect_resp a = rg_elect_step(sc.cfg, g, s, v, e, m);
            rg_follow_close(c, g, v, o);
            rg_soft_close(sc, g, s, so);
            rg_elect_close(ec, g, e, eo);
            printf("R %u %u %" PRIu64 " %u %u %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %u\n", a.result, a.events, a.term, a.req_kind, a.targets,
                   a.flags, a.req_term, a.req_index, a.req_log_term, a.req_commit, a.req_commit_term, a.status);
        } else if (op[0] == 'S') {
            const rg_follow_state s = rg_follow_load_state(c, g);
            printf("S %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %u", s.committed, s.last_index, s.dummy_index, s.dummy_term, s.n_runs);
            for (u32 i = 0; i < s.n_runs; i++) printf(" %" PRIu64 " %" PRIu64, s.run_first[i], s.run_term[i]);
            printf("\n");
        } else if (op[0] == 'Q') {
            const rg_follow_soft w = rg_follow_load_soft(sc, g);
            printf("Q %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRId64 " %u %u %u %u\n", w.term, w.vote, w.leader_id, w.priority, (unsigned)w.role, w.election_elapsed,
                   w.randomized_timeout, (unsigned)w.promotable);
        } else if (op[0] == 'V') {
            const rg_follow_elect w = rg_follow_load_elect(ec, role.data(), g);
            printf("V %" PRIu64 " %u %u %u\n", w.self_id, w.conf, (unsigned)w.yes, (unsigned)w.no);
        } else {
            return 6;
        }
    }
    return 0;
}
