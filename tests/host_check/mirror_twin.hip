// mirror_twin.hip -- TEST INFRASTRUCTURE. The loader and the store of the dense tick's read mirror (raft_rs_amd/csrc/rg_mirror.h:
// rg_load_group_pk, rg_store_mirror -- the exact code k_tick_mirror inlines) compiled for the HOST, beside the plain road
// (rg_load_group / rg_group_tick / rg_store_group), so a CPU-only test can run both over the same stream and compare every column
// after every tick. Never part of libraftgroups.so. Build: hipcc -O3 -shared -fPIC --offload-arch=gfx950 mirror_twin.hip -o libmirror_twin.so
//
// WAVE mode (mode 3): on the device the escape branch of rg_load_group_pk is decided by the whole 64-lane wave (rg_mirror_any is a
// ballot), so a lane WITHOUT an escape re-reads its cells too when a neighbour has one. The twin plays that: before it runs the
// lanes of a block of 64 consecutive groups it works out the block's answer from the plane, and rg_mirror_any returns that.
static bool twin_wave_mode = false, twin_wave_any = false;
#define RG_MIRROR_TWIN_ANY(mine) (twin_wave_mode ? twin_wave_any : (mine))
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

// mode 0: the plain road; 1: build (plain loader, then the words); 2: packed (the words in the place of the two columns), every
// lane deciding the escape branch for itself; 3: packed, the block of 64 groups deciding it together (the device's semantics).
// Exactly k_tick_mirror's sequence in modes 1 and 2 (NTM only picks the load instruction on the device).
template <int P, typename IX> static void twin_one(const RgState &st, const RgMsgs &ms, u32 *pk, int mode, IX g) {
    RgGroup<P> r;
    typedef typename RgLaneStores<P, false, false>::type ES;
    static_assert(!ES::on && !ES::late_pc, "the lane kernel neither stores early nor loads late");
    if (mode == 2) rg_load_group_pk<P, IX, false>(r, st, ms, pk, g);
    else rg_load_group<P, RG_LANE_NX, IX, false, false, ES>(r, st, ms, g);
    rg_group_tick<P, false, RG_LANE_NX, false, IX, ES>(r, st, ms, g);
    rg_store_group<P, IX, 3, false, false, false>(r, st, g);
    if (mode) rg_store_mirror<P, IX>(r, pk, st.stride, g);
}
template <int P> static void twin_tick(const RgState &st, const RgMsgs &ms, u32 *pk, int mode) {
    const bool fits32 = rg_fits_u32_offsets(P, st.stride);
    twin_wave_mode = mode == 3;
    if (mode == 3) mode = 2;
    for (u64 g = 0; g < st.G; g++) { // (odd groups with 64-bit indices: both index types of the loader are compared)
        if (twin_wave_mode && !(g & 63u)) { // the block's answer, from the plane as the last tick left it
            twin_wave_any = false;
            for (u64 k = g; k < g + 64 && k < st.G; k++)
                for (int p = 0; p < P; p++) {
                    const u32 w = pk[(u64)p * st.stride + k];
                    twin_wave_any = twin_wave_any || (w & 0xffffu) == RG_MIRROR_MT_ESC || (w >> 16) == RG_MIRROR_PC_ESC;
                }
        }
        if (fits32 && !(g & 1)) twin_one<P, u32>(st, ms, pk, mode, (u32)g);
        else twin_one<P, u64>(st, ms, pk, mode, g);
    }
    twin_wave_mode = false;
}

extern "C" int rg_mirror_twin_tick(unsigned P, unsigned long G, unsigned long stride, void *const *state, const void *const *msg,
                                   unsigned *pk, int mode) {
    const RgState st = twin_state(state, G, stride);
    const RgMsgs ms = twin_msgs(msg);
    twin_derive(st, P);
    switch (P) {
    case 1: twin_tick<1>(st, ms, pk, mode); break;
    case 2: twin_tick<2>(st, ms, pk, mode); break;
    case 3: twin_tick<3>(st, ms, pk, mode); break;
    case 4: twin_tick<4>(st, ms, pk, mode); break;
    case 5: twin_tick<5>(st, ms, pk, mode); break;
    case 6: twin_tick<6>(st, ms, pk, mode); break;
    case 7: twin_tick<7>(st, ms, pk, mode); break;
    case 8: twin_tick<8>(st, ms, pk, mode); break;
    default: return -1;
    }
    return 0;
}

// the word of one cell, for the edge table of the test
extern "C" unsigned rg_mirror_twin_encode(unsigned long mt, unsigned long pc, unsigned long c) { return rg_mirror_encode(mt, pc, c); }
extern "C" unsigned long rg_mirror_twin_match(unsigned w, unsigned long c) { return rg_mirror_match(w, c); }
extern "C" unsigned long rg_mirror_twin_prc(unsigned w, unsigned long c) { return rg_mirror_prc(w, c); }
