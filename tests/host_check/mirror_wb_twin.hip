// mirror_wb_twin.hip -- TEST INFRASTRUCTURE. The write-behind road of the dense tick's read mirror (raft_rs_amd/csrc/rg_mirror.h:
// rg_load_group_pk, rg_store_mirror_wb, rg_mirror_settle_group -- the exact code k_tick_mirror_wb and k_mirror_settle inline)
// compiled for the HOST beside the plain road and the write-through road, so a CPU-only test can run a streak, settle, and compare
// every column with the plain road's. Never part of libraftgroups.so.
// Build: hipcc -O3 -shared -fPIC --offload-arch=gfx950 mirror_wb_twin.hip -o libmirror_wb_twin.so
//
// WAVES: on the device three decisions belong to the whole wave (rg_mirror_any is a ballot): the loader's escape branch (over the
// words the wave loads), the write-behind store of the cells (over the words the wave is about to store) and the settle's skip
// (over the words of the block). The twin plays a wave of `lanes` consecutive groups (64: the device; 1: every group alone): it
// works out each answer for the block before the lanes ask, and rg_mirror_any returns it.
static bool twin_wave_any = false;
#define RG_MIRROR_TWIN_ANY(mine) ((void)(mine), twin_wave_any)
#include "../../raft_rs_amd/csrc/rg_tick_kernels.h"

// state[]: match next pr_commit pend_snap pend_rs gid pflags commit term_lo term_hi cfg out
//          run_first run_term dummy_index dummy_term cur_term host_hint run_count   (19 pointers, as tests/host_check/host_tick.hip)
// msg[]:   m_index m_commit m_hint m_rs m_flags m_logterm       (6 pointers; no log terms here: no pre-pass)
static RgState twin_state(void *const *p, u64 G, u64 stride) {
    RgState st = RgState();
    st.match = (u64 *)p[0]; st.next = (u64 *)p[1]; st.prc = (u64 *)p[2]; st.psnap = (u64 *)p[3];
    st.prs = (u64 *)p[4]; st.gid = (u64 *)p[5]; st.pflags = (u64 *)p[6]; st.commit = (u64 *)p[7];
    st.lo = (u64 *)p[8]; st.hi = (u64 *)p[9]; st.cfg = (u32 *)p[10]; st.out = (u32 *)p[11];
    st.run_first = (u64 *)p[12]; st.run_term = (u64 *)p[13]; st.dummy_idx = (u64 *)p[14]; st.dummy_term = (u64 *)p[15];
    st.cur_term = (u64 *)p[16];
    st.hhint = (u8 *)p[17];
    if ((u8 *)p[18] != (u8 *)p[17] + stride) __builtin_trap(); // (RG_COL_RUN_COUNT sits `stride` bytes behind RG_COL_HOST_HINT: rg_run_n)
    st.G = G; st.stride = stride;
    return st;
}
static RgMsgs twin_msgs(const void *const *p) {
    RgMsgs ms;
    ms.mi = (const u64 *)p[0]; ms.mc = (const u64 *)p[1]; ms.mh = (const u64 *)p[2]; ms.mrs = (const u64 *)p[3];
    ms.mflags = (const u64 *)p[4]; ms.mlt = (const u64 *)p[5];
    ms.mhr = ms.mh;
    return ms;
}
// the engine-owned bits and cells the library derives when columns are loaded (k_fix_pending, k_fix_run_count)
static void twin_derive(const RgState &st, unsigned P) {
    for (u64 g = 0; g < st.G; g++) {
        u64 row = st.pflags[g];
        for (unsigned p = 0; p < P; p++) {
            const u64 o = (u64)p * st.stride + g;
            row &= ~((u64)RG_PF_PENDING << (8 * p));
            row |= (u64)((st.psnap[o] ? RG_PF_PEND_SNAP : 0u) | (st.prs[o] ? RG_PF_PEND_RS : 0u)) << (8 * p);
        }
        st.pflags[g] = row;
        rg_run_n(st)[g] = (u8)rg_count_runs(st, g);
    }
}

static bool twin_word_esc(u32 w) { return (w & 0xffffu) == RG_MIRROR_MT_ESC || (w >> 16) == RG_MIRROR_PC_ESC; }
// does any word of the plane hold an escape in groups [g0, g1)?
static bool twin_plane_any(const u32 *pk, u64 stride, unsigned P, u64 g0, u64 g1) {
    for (u64 g = g0; g < g1; g++)
        for (unsigned p = 0; p < P; p++)
            if (twin_word_esc(pk[(u64)p * stride + g])) return true;
    return false;
}
// ... and would any word the lane is about to store (rg_store_mirror_wb's encode, from the registers)?
template <int P> static bool twin_regs_esc(const RgGroup<P> &r) {
    const u32 present = RG_CFG_PRESENT(r.cfg);
    for (int p = 0; p < P; p++)
        if (((present >> p) & 1u) && twin_word_esc(rg_mirror_encode(r.mt[p], r.pc[p], r.commit))) return true;
    return false;
}

// mode 0: the plain road; 1: build (plain loader, every store, then the words); 2: packed write-through (k_tick_mirror<PACKED>);
// 3: packed write-behind (k_tick_mirror_wb). A block's lanes load and tick first and store afterwards, as a wave does.
template <int P, typename IX> static void twin_load_tick(RgGroup<P> &r, const RgState &st, const RgMsgs &ms, const u32 *pk, int mode, IX g) {
    typedef typename RgLaneStores<P, false, false>::type ES;
    static_assert(!ES::on && !ES::late_pc, "the lane kernel neither stores early nor loads late");
    if (mode >= 2) rg_load_group_pk<P, IX, false>(r, st, ms, pk, g);
    else rg_load_group<P, RG_LANE_NX, IX, false, false, ES>(r, st, ms, g);
    rg_group_tick<P, false, RG_LANE_NX, false, IX, ES>(r, st, ms, g);
}
template <int P, typename IX> static void twin_store(const RgGroup<P> &r, const RgState &st, u32 *pk, int mode, IX g) {
    if (mode == 3) {
        rg_store_group<P, IX, 3, false, false, false, false>(r, st, g);
        rg_store_mirror_wb<P, IX>(r, st, pk, g);
    } else {
        rg_store_group<P, IX, 3, false, false, false>(r, st, g);
        if (mode) rg_store_mirror<P, IX>(r, pk, st.stride, g);
    }
}
template <int P> static void twin_tick(const RgState &st, const RgMsgs &ms, u32 *pk, int mode, u64 lanes) {
    const bool fits32 = rg_fits_u32_offsets(P, st.stride);
    static RgGroup<P> regs[64];
    for (u64 g0 = 0; g0 < st.G; g0 += lanes) {
        const u64 g1 = g0 + lanes < st.G ? g0 + lanes : st.G;
        twin_wave_any = mode >= 2 && twin_plane_any(pk, st.stride, P, g0, g1); // the loader's branch
        for (u64 g = g0; g < g1; g++) { // (odd groups with 64-bit indices: both index types are compared)
            if (fits32 && !(g & 1)) twin_load_tick<P, u32>(regs[g - g0], st, ms, pk, mode, (u32)g);
            else twin_load_tick<P, u64>(regs[g - g0], st, ms, pk, mode, g);
        }
        twin_wave_any = false; // the store's branch
        for (u64 g = g0; g < g1 && mode == 3; g++) twin_wave_any = twin_wave_any || twin_regs_esc<P>(regs[g - g0]);
        for (u64 g = g0; g < g1; g++) {
            if (fits32 && !(g & 1)) twin_store<P, u32>(regs[g - g0], st, pk, mode, (u32)g);
            else twin_store<P, u64>(regs[g - g0], st, pk, mode, g);
        }
    }
}

extern "C" int rg_mirror_wb_twin_tick(unsigned P, unsigned long G, unsigned long stride, void *const *state, const void *const *msg,
                                      unsigned *pk, int mode, unsigned lanes) {
    if (lanes != 1 && lanes != 64) return -1;
    const RgState st = twin_state(state, G, stride);
    const RgMsgs ms = twin_msgs(msg);
    twin_derive(st, P);
    switch (P) {
    case 1: twin_tick<1>(st, ms, pk, mode, lanes); break;
    case 2: twin_tick<2>(st, ms, pk, mode, lanes); break;
    case 3: twin_tick<3>(st, ms, pk, mode, lanes); break;
    case 4: twin_tick<4>(st, ms, pk, mode, lanes); break;
    case 5: twin_tick<5>(st, ms, pk, mode, lanes); break;
    case 6: twin_tick<6>(st, ms, pk, mode, lanes); break;
    case 7: twin_tick<7>(st, ms, pk, mode, lanes); break;
    case 8: twin_tick<8>(st, ms, pk, mode, lanes); break;
    default: return -1;
    }
    return 0;
}

// k_mirror_settle over the whole shard: rg_mirror_settle_group per group, the block's skip decided by the block
extern "C" int rg_mirror_wb_twin_settle(unsigned P, unsigned long G, unsigned long stride, void *const *state, const unsigned *pk,
                                        unsigned lanes) {
    if (lanes != 1 && lanes != 64) return -1;
    const RgState st = twin_state(state, G, stride);
    for (u64 g0 = 0; g0 < G; g0 += lanes) {
        const u64 g1 = g0 + lanes < G ? g0 + lanes : G;
        twin_wave_any = twin_plane_any(pk, stride, P, g0, g1);
        for (u64 g = g0; g < g1; g++) rg_mirror_settle_group(st, pk, P, g);
    }
    return 0;
}
