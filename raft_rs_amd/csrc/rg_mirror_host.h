// rg_mirror_host.h -- the HOST side of the dense tick's read mirror as one pure function: what the engine knows about the plane
// (rg_mirror.h) and the two u64 columns it stands for, which kernel the next dense tick runs, and when the columns are settled
// from the plane. No HIP, no engine: abi_tick.hip applies it to rg_engine's three fields (rg_mirror_apply), and
// tests/host_check/mirror_wb_state.cpp compiles it alone and walks the whole table.
//
//   valid    the plane describes RG_COL_MATCH / RG_COL_PR_COMMIT / RG_COL_COMMIT (the next mirror launch may read it)
//   behind   a write-behind launch has run since the last settle: in every block of 64 groups whose words hold no escape the WORDS are
//            the state and the block's match / committed_index cells may be stale. Only a settle clears it, and only one that was
//            executed -- a settle captured into a graph has not run yet.
//   streak   packed write-through launches since the last build launch or settle point. Write-behind engages once it reaches
//            RG_MIRROR_WB_AFTER, so a host that looks at the columns between ticks never pays a settle.
#pragma once

// Packed launches that stay write-through after a build launch or a settle point; 0 = write-behind never engages.
// ceil(settle time / per-launch gain of write-behind over write-through), measured at 1 M x 5: a settle (kernel + the memset
// behind it) 31.5 us, the gain 10.6 us per launch (medians of three runs each) -> ceil(2.98) = 3 (profiles/mirror_writebehind.txt;
// slowest run against fastest the gain is 9.0 us and the ratio 3.5)
#ifndef RG_MIRROR_WB_AFTER
#define RG_MIRROR_WB_AFTER 3
#endif

struct RgMirrorHost {
    bool valid, behind;
    unsigned streak;
};

enum RgMirrorCall {
    RG_MC_TICK_MIRROR, // a dense tick whose plan is a mirror launch
    RG_MC_TICK_OTHER,  // a dense tick on any other kernel: group commit, tick + send, classes, split, fused and list ticks
    RG_MC_DROP,        // RG_ENTER, the sparse flush: the call may write the columns
    RG_MC_KEEP,        // writes none of the cached columns and reads neither match nor committed_index
    RG_MC_KEEP_LOOK,   // reads match or committed_index (rg_read_column of the two, rg_workload_gen): the plane stays
    RG_MC_OFF          // the mirror goes off: rg_column_ptr, a graph capture, the escape watch
};
enum RgMirrorKernel { RG_MK_NONE = 0, RG_MK_BUILD = 1, RG_MK_PACKED = 2, RG_MK_PACKED_WB = 3 };

struct RgMirrorStep {
    int kernel;  // RgMirrorKernel: what a RG_MC_TICK_MIRROR call launches
    bool settle; // the settle kernel goes first
};

// `executed`: what the call enqueues runs now (false: it is being captured into a graph -- `behind` survives a captured settle)
static inline RgMirrorStep rg_mirror_step(RgMirrorHost &m, RgMirrorCall call, unsigned wb_after, bool executed = true) {
    RgMirrorStep s = {RG_MK_NONE, false};
    if (call == RG_MC_KEEP) return s;
    if (call == RG_MC_TICK_MIRROR) {
        if (m.valid && wb_after && m.streak >= wb_after) { // the streak goes on: the columns fall (or stay) behind
            s.kernel = RG_MK_PACKED_WB;
            m.behind = true;
            return s;
        }
        s.kernel = m.valid ? RG_MK_PACKED : RG_MK_BUILD;
        // (a build launch reads the columns, a write-through launch stores only the cells it changed: both need them current)
        s.settle = m.behind;
        m.streak = m.valid ? m.streak + 1 : 0;
        if (s.settle) m.streak = 0;
        m.valid = true;
    } else {
        s.settle = m.behind;
        m.streak = 0;
        if (call != RG_MC_KEEP_LOOK) m.valid = false;
    }
    if (s.settle && executed) m.behind = false;
    return s;
}
