// ext_mirror.hip -- what the dense tick's read mirror (rg_mirror.h, k_tick_mirror; decided in abi_tick.hip: rg_plan_tick) tells the
// host about itself (include/raftgroups_mirror.h, the seventh extension header: its one entry point, rgr_mirror_stats, is exported as an
// object holding the function's address -- the set of exported functions is what the older headers declare). Counters kept on the
// host: nothing here touches the device or the mirror.
#include "rg_engine.h"
#pragma GCC visibility push(default) // (the build hides everything else: the exports are the header's declarations, as in rg_engine.h)
#include "../../include/raftgroups_mirror.h"
#pragma GCC visibility pop

static int rg_mirror_stats_impl(const rg_engine *h, rgr_mirror_info *info) try {
    if (!h || !info) return rg_fail(RG_ERR_INVALID_ARG, "rgr_mirror_stats: bad argument");
    memset(info, 0, sizeof(*info));
    info->packed_launches = h->mirror_packed;
    info->build_launches = h->mirror_build;
    info->plane_bytes = h->mirror ? (uint64_t)h->P * h->stride * 4 : 0;
    info->present = h->mirror ? 1u : 0u;
    info->valid = h->mirror && h->mirror_valid && !h->mirror_off && !h->mirror_escaping ? 1u : 0u;
    info->off = (h->mirror_off ? 1u : 0u) | (h->mirror_escaping ? 2u : 0u);
    info->version = RGR_MIRROR_VERSION;
    return RG_OK;
} RG_ABI_GUARD

#if !defined(__HIP_DEVICE_COMPILE__) /* (a host object: the device pass must not emit it) */
extern "C" {
__attribute__((visibility("default"))) const rgr_mirror_stats_fn rgr_mirror_stats = rg_mirror_stats_impl;
}
#endif
