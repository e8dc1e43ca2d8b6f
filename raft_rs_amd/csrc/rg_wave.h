// rg_wave.h -- what a wave (64 lanes) of the clock, gate and vote kernels does together so that it issues ONE atomic where its lanes
// would issue up to 64: a ballot, a sum, a list append. Every lane of the wave must call (no divergent caller); no LDS.
#pragma once
#include "rg_common.h"

// A wave's count of its lanes with `mine` (the same value in every lane)
RG_D u32 rg_wave_count(bool mine) { return (u32)__popcll(__ballot(mine)); }

// The wave's sum of `n` (small: at most 8 per lane) added to *count with one atomic; nothing is issued for a wave of zeros.
RG_D void rg_wave_add(u32 n, unsigned long long *count) {
    if (!__ballot(n != 0)) return;
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) n += __shfl_xor(n, w);
    if ((threadIdx.x & 63u) == 0) atomicAdd(count, (unsigned long long)n);
}

// A wave's lanes with `mine` claim consecutive places of list[cap] with one atomic on *count (which ends as the TRUE total); a lane
// whose place lies within cap writes its group.
RG_D void rg_wave_append(bool mine, u64 g, u64 *list, u64 cap, unsigned long long *count) {
    const unsigned long long ballot = __ballot(mine);
    if (!ballot) return;
    const u32 lane = threadIdx.x & 63u, leader = (u32)__ffsll(ballot) - 1u;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(count, (unsigned long long)__popcll(ballot));
    base = __shfl(base, (int)leader);
    const u64 at = base + (u64)__popcll(ballot & ((1ULL << lane) - 1ULL));
    if (mine && at < cap) list[at] = g;
}
