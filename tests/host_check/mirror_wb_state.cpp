// mirror_wb_state.cpp -- TEST INFRASTRUCTURE. The read mirror's host state machine (raft_rs_amd/csrc/rg_mirror_host.h: a pure
// function, no HIP, no engine) compiled alone: prints one row per (wb_after, executed, call class, valid, behind, streak) with
// what rg_mirror_step answers and leaves, for tests/test_mirror_writebehind_host.py to compare with its own table.
// Build: c++ -std=c++17 -O1 mirror_wb_state.cpp -o mirror_wb_state
#include <cstdio>

#include "../../raft_rs_amd/csrc/rg_mirror_host.h"

int main() {
    std::printf("default_wb_after %u\n", (unsigned)RG_MIRROR_WB_AFTER);
    const unsigned afters[] = {0, 1, 3};
    for (unsigned wb_after : afters)
        for (int executed = 0; executed < 2; executed++)
            for (int call = RG_MC_TICK_MIRROR; call <= RG_MC_OFF; call++)
                for (int valid = 0; valid < 2; valid++)
                    for (int behind = 0; behind < 2; behind++)
                        for (unsigned streak = 0; streak <= wb_after + 1; streak++) {
                            RgMirrorHost m = {valid != 0, behind != 0, streak};
                            const RgMirrorStep s = rg_mirror_step(m, (RgMirrorCall)call, wb_after, executed != 0);
                            std::printf("%u %d %d %d %d %u -> %d %d %d %d %u\n", wb_after, executed, call, valid, behind, streak, s.kernel,
                                        (int)s.settle, (int)m.valid, (int)m.behind, m.streak);
                        }
    return 0;
}
