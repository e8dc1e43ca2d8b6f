// tick_inst.hip -- the tick kernels and their launchers for ONE slot count (compile with -DRG_P=1..8).
#ifndef RG_P
#error "compile with -DRG_P=<slots>"
#endif
#define RG_TICK_INSTANTIATE
#include "rg_tick_kernels.h"

// this slot count's launcher table (taking the launchers' addresses instantiates them, and the kernels with them)
template <> const RgTickLaunch &rg_tick_launch_p<RG_P>() {
    static const RgTickLaunch t = {rg_launch_tick_t<RG_P>,        rg_launch_tick_classes_t<RG_P>, rg_launch_tick_split_t<RG_P>,
                                   rg_launch_tick_list_t<RG_P>,   rg_launch_tick_fused_t<RG_P>,   rg_launch_tick_send_t<RG_P>,
                                   rg_launch_flush_small_t<RG_P>, rg_launch_flush_small_send_t<RG_P>, rg_launch_mailbox_t<RG_P>,
                                   rg_launch_tick_mirror_t<RG_P>};
    return t;
}
