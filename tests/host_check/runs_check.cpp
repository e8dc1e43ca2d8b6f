// runs_check.cpp -- csrc/rg_runs.h, a stand-alone program (tests/test_runs_host.py builds it plainly and with
// -fsanitize=address,undefined and runs it directly). The cutter writes into vectors of exactly n and runs + 1 words, so a
// write past either end is the sanitizers' to see; every batch is compared with a plain reference written here.
#include "rg_runs.h"

#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);   \
            return 1;                                                 \
        }                                                             \
    } while (0)

struct Rec { uint64_t group; uint32_t payload; };

// Cuts `g` (one group per record), checks every invariant and compares with the reference: the groups ascending (std::map),
// each with its records' positions in array order.
static int cut(const std::vector<uint64_t> &g, uint64_t want_runs) {
    const uint64_t n = g.size();
    std::vector<Rec> recs(n);
    for (uint64_t i = 0; i < n; i++) recs[i] = Rec{g[i], (uint32_t)i};
    const auto group_of = [&](uint64_t i) { return recs[i].group; };
    std::vector<uint32_t> order(3, 77u); // (stale contents of an earlier, other-sized batch)
    const uint64_t runs = rg_runs_sort(order, n, group_of);
    CHECK(order.size() == n && runs == want_runs);
    std::vector<uint32_t> orig(n), run_start(runs + 1);
    CHECK(rg_runs_cut(order, group_of, orig.data(), run_start.data()) == runs);

    CHECK(run_start[0] == 0 && run_start[runs] == n);
    std::vector<bool> seen(n, false);
    for (uint64_t i = 0; i < n; i++) {
        CHECK(orig[i] < n && !seen[orig[i]] && orig[i] == order[i]); // a permutation of 0..n-1
        seen[orig[i]] = true;
    }
    for (uint64_t r = 0; r < runs; r++) {
        CHECK(run_start[r] < run_start[r + 1]); // strictly ascending: no empty run
        for (uint32_t i = run_start[r]; i < run_start[r + 1]; i++) {
            CHECK(g[orig[i]] == g[orig[run_start[r]]]);               // one group per run
            if (i > run_start[r]) CHECK(orig[i] > orig[i - 1]);       // stable: array order within the run
        }
        if (r) CHECK(g[orig[run_start[r]]] > g[orig[run_start[r - 1]]]); // groups ascend across runs, on 64 bits
    }

    std::map<uint64_t, std::vector<uint32_t>> ref;
    for (uint64_t i = 0; i < n; i++) ref[g[i]].push_back((uint32_t)i);
    CHECK(ref.size() == runs);
    uint64_t r = 0, at = 0;
    for (const auto &kv : ref) {
        CHECK(run_start[r++] == at);
        for (uint32_t pos : kv.second) CHECK(orig[at++] == pos);
    }
    return 0;
}

static int check_cutter() {
    CHECK(cut({9}, 1) == 0);
    CHECK(cut({4, 4, 4, 4, 4, 4, 4}, 1) == 0);
    CHECK(cut({0, 1, 2, 3, 4, 5}, 6) == 0);
    CHECK(cut({5, 4, 3, 2, 1, 0}, 6) == 0);
    CHECK(cut({5, 3, 5, 3, 5}, 2) == 0);
    // the sort is on 64 bits: 2^32 comes after 2^32 - 1, not beside 0
    CHECK(cut({1ULL << 32, ~0ULL, 0, 0xffffffffULL, 1ULL << 32, 0}, 4) == 0);
    uint64_t x = 0x9e3779b97f4a7c15ULL; // seeded sweep: n <= 64 over <= 8 groups
    const auto next = [&] { return x ^= x << 13, x ^= x >> 7, x ^= x << 17, x; };
    for (int t = 0; t < 4000; t++) {
        const uint64_t n = 1 + next() % 64, k = 1 + next() % 8, base = next() % 3 ? next() % 1000 : 0xfffffffcULL;
        std::vector<uint64_t> g(n);
        std::map<uint64_t, int> distinct;
        for (uint64_t i = 0; i < n; i++) distinct[g[i] = base + next() % k]++;
        CHECK(cut(g, distinct.size()) == 0);
    }
    return 0;
}

// The three call shapes of the follower side, as the hand-chained expressions they replace. A: the align of today.
static size_t A(size_t b) { return (b + 255) & ~(size_t)255; }

static int check_layout() {
    {
        RgLayout lay;
        CHECK(lay.total == 0 && lay.add(0) == 0 && lay.total == 0); // an empty region first
        CHECK(lay.add(1) == 0 && lay.total == 1);
        CHECK(lay.add(0) == 256 && lay.total == 256);               // an empty region in the middle takes no room ...
        CHECK(lay.add(0) == 256 && lay.add(300) == 256 && lay.total == 556); // ... and the next one starts where it does
        CHECK(lay.add(256) == 768 && lay.total == 1024 && lay.add(7) == 1024 && lay.total == 1031); // the unpadded end of the last
    }
    // the sizes of rg_follow_msg, rg_follow_hdr, rg_follow_ent_run, rg_follow_resp, rg_follow_gate_resp, RgElectStaged and
    // rg_follow_elect_resp (any sizes would do: the chains are what is compared)
    const size_t MSG = 56, HDR = 32, EXT = 16, RESP = 48, GATE = 16, EREC = 48, ERESP = 72;
    const size_t shapes[][3] = {{1, 1, 0}, {3, 2, 0}, {5, 5, 7}, {16, 1, 1}, {64, 63, 0}, {65, 64, 300}, {1366, 300, 0}, {100000, 99999, 12345}};
    for (const auto &sh : shapes) {
        const size_t n = sh[0], runs = sh[1], n_ext = sh[2];
        { // rg_follow_step
            const size_t off_orig = A(n * MSG), off_runs = off_orig + A(n * 4), off_ext = off_runs + A((runs + 1) * 4), off_resp = off_ext + A(n_ext * EXT);
            RgLayout lay;
            CHECK(lay.add(n * MSG) == 0 && lay.add(n * 4) == off_orig && lay.add((runs + 1) * 4) == off_runs && lay.add(n_ext * EXT) == off_ext);
            CHECK(lay.add(n * RESP) == off_resp && lay.total == off_resp + n * RESP);
            CHECK(off_orig % 256 == 0 && off_runs % 256 == 0 && off_ext % 256 == 0 && off_resp % 256 == 0);
        }
        { // rg_follow_step_gated
            const size_t off_hdr = A(n * MSG), off_orig = off_hdr + A(n * HDR), off_runs = off_orig + A(n * 4), off_ext = off_runs + A((runs + 1) * 4),
                         off_resp = off_ext + A(n_ext * EXT), off_gate = off_resp + A(n * RESP);
            RgLayout lay;
            CHECK(lay.add(n * MSG) == 0 && lay.add(n * HDR) == off_hdr && lay.add(n * 4) == off_orig && lay.add((runs + 1) * 4) == off_runs);
            CHECK(lay.add(n_ext * EXT) == off_ext && lay.add(n * RESP) == off_resp && lay.add(n * GATE) == off_gate && lay.total == off_gate + n * GATE);
            CHECK(off_hdr % 256 == 0 && off_gate % 256 == 0);
        }
        { // rg_elect_run_list
            const size_t off_orig = A(n * EREC), off_runs = off_orig + A(n * 4), off_resp = off_runs + A((runs + 1) * 4);
            RgLayout lay;
            CHECK(lay.add(n * EREC) == 0 && lay.add(n * 4) == off_orig && lay.add((runs + 1) * 4) == off_runs && lay.add(n * ERESP) == off_resp);
            CHECK(lay.total == off_resp + n * ERESP);
        }
    }
    // ... and three of them as plain numbers, worked out by hand from the parent's chains
    {
        RgLayout lay; // rg_follow_step, n = 3, runs = 2, n_ext = 0: 168 -> 256 | 12 -> 256 | 12 -> 256 | 0 | 144
        CHECK(lay.add(3 * MSG) == 0 && lay.add(3 * 4) == 256 && lay.add(3 * 4) == 512 && lay.add(0) == 768 && lay.add(3 * RESP) == 768 && lay.total == 912);
    }
    {
        RgLayout lay; // rg_follow_step_gated, n = 5, runs = 5, n_ext = 7: 280 -> 512 | 160 | 20 | 24 | 112 | 240 | 80
        CHECK(lay.add(5 * MSG) == 0 && lay.add(5 * HDR) == 512 && lay.add(5 * 4) == 768 && lay.add(6 * 4) == 1024 && lay.add(7 * EXT) == 1280);
        CHECK(lay.add(5 * RESP) == 1536 && lay.add(5 * GATE) == 1792 && lay.total == 1872);
    }
    {
        RgLayout lay; // rg_elect_run_list, n = 65, runs = 64: 3120 -> 3328 | 260 -> 512 | 260 -> 512 | 4680
        CHECK(lay.add(65 * EREC) == 0 && lay.add(65 * 4) == 3328 && lay.add(65 * 4) == 3840 && lay.add(65 * ERESP) == 4352 && lay.total == 9032);
    }
    return 0;
}

int main() {
    if (check_cutter() || check_layout()) return 1;
    printf("ok\n");
    return 0;
}
