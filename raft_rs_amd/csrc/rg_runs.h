// rg_runs.h -- what every sparse batch of the follower side does before it is staged: sort the records by group, cut them into
// runs, and lay the batch's regions out in one staging buffer. No HIP in here: tests/host_check/runs_check.cpp runs it under the
// sanitizers.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

static inline size_t rg_align(size_t x) { return (x + 255) & ~(size_t)255; }

// The layout of one staged batch: regions in the order they are added, each on a 256-byte boundary; the total is the unpadded
// end of the last one.
struct RgLayout {
    size_t total = 0;
    size_t add(size_t bytes) {
        const size_t off = rg_align(total);
        total = off + bytes;
        return off;
    }
};

// The run cutter, in two steps because the layout needs the number of runs before there is memory for them. group_of(i) is
// the group of record i; n < 0xffffffff is the caller's check.
// 1. order <- the positions 0..n-1 sorted by group -- stable, so a group's records keep their array order; -> the number of runs
template <typename GroupOf> static inline uint64_t rg_runs_sort(std::vector<uint32_t> &order, uint64_t n, GroupOf group_of) {
    order.resize(n);
    for (uint64_t i = 0; i < n; i++) order[i] = (uint32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return group_of(a) < group_of(b); });
    uint64_t runs = 0;
    for (uint64_t i = 0; i < n; i++) runs += i == 0 || group_of(order[i]) != group_of(order[i - 1]);
    return runs;
}
// 2. orig[i] <- the array position of the i-th sorted record, run_start[r] <- the sorted position run r begins at,
//    run_start[runs] <- n; -> the number of runs
template <typename GroupOf> static inline uint64_t rg_runs_cut(const std::vector<uint32_t> &order, GroupOf group_of, uint32_t *orig, uint32_t *run_start) {
    const uint64_t n = order.size();
    uint64_t r = 0;
    for (uint64_t i = 0; i < n; i++) {
        orig[i] = order[i];
        if (i == 0 || group_of(order[i]) != group_of(order[i - 1])) run_start[r++] = (uint32_t)i;
    }
    run_start[r] = (uint32_t)n;
    return r;
}
