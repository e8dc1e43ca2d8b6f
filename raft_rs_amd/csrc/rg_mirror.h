// rg_mirror.h -- the dense lane tick's READ MIRROR: one packed 32-bit word per (slot, group) from which the next dense tick
// rebuilds Progress.matched and Progress.committed_index instead of loading their two 8-byte cells (80 B -> 20 B per group at
// five slots). Included by rg_tick_kernels.h behind rg_load_group / rg_store_group; the host twin of the tests
// (tests/host_check/mirror_twin.hip) compiles the same functions for the CPU.
//
// The mirror starts as a CACHE of the two u64 columns: k_tick_mirror stores them exactly as before and they are correct after
// every such launch; only the mirror kernels write the plane and only they read it. The first protocol is invalidation, on the
// host (rg_engine::mirror_valid, cleared by RG_ENTER): a tick that finds the plane invalid loads the columns as rg_load_group
// does ("build"), a tick that finds it valid loads the words ("packed"); both leave a valid plane.
// Once packed launches follow one another (RG_MIRROR_WB_AFTER of them, rg_mirror_host.h) the plane becomes the STATE of those
// two columns: k_tick_mirror_wb stores the words and no longer the cells ("write-behind", below), the host remembers that the
// columns are behind (rg_engine::cols_behind), and every entry that reads or writes them, or ends the streak, first writes them
// back from the plane (rg_mirror_settle). The columns are then what a write-through engine would hold, bit for bit.
//
// The word of slot p, with c = the group's commit index as the tick leaves it (RgGroup::commit at store time, which is what
// the next tick loads from RG_COL_COMMIT):
//   bits  0-15  matched - c          as a signed 16-bit value in [-32767, 32767];  0x8000 = not representable
//   bits 16-31  c - committed_index  as an unsigned 16-bit value in [0, 65534];    0xFFFF = not representable
// Both differences are taken in 64-bit wrap-around arithmetic and range-checked afterwards, so ANY pair of u64 values encodes
// to a value or to the escape. A field that holds the escape is fetched from its column cell by the packed loader (a dependent
// load of the wave's cells; on the benchmark's stream fewer than one field in a thousand, tests/test_mirror_host.py).
//
// Every slot with a Progress is encoded from the REGISTERS, every tick, event or not (the others get the word 0): the base moves with the commit index, so
// no word survives a tick anyway, and a wave's stores of one slot are 256 contiguous bytes. The decode therefore reproduces the
// register image the tick left -- which, for a slot with a Progress, is the column cell (the tick stores what it changes), and
// a slot WITHOUT one gets the word 0 (rg_store_mirror), which decodes to values no tick looks at. So rg_group_tick sees the
// operands rg_load_group would have produced wherever it reads them, and rg_store_group stores what it would have stored.
#pragma once
#include "rg_mirror_host.h" // RG_MIRROR_WB_AFTER, RgMirrorKernel: the host's side

#define RG_MIRROR_MT_ESC 0x8000u
#define RG_MIRROR_PC_ESC 0xffffu

RG_HD u32 rg_mirror_encode(u64 mt, u64 pc, u64 c) {
    const u64 dm = mt - c + 32767u; // matched - c in [-32767, 32767]  <=>  dm in [0, 65534]
    const u64 dp = c - pc;
    const u32 lo = dm <= 65534u ? ((u32)dm - 32767u) & 0xffffu : RG_MIRROR_MT_ESC;
    const u32 hi = dp <= 65534u ? (u32)dp : RG_MIRROR_PC_ESC;
    return lo | (hi << 16);
}
RG_HD u64 rg_mirror_match(u32 w, u64 c) { return c + (u64)(int64_t)(int16_t)(w & 0xffffu); }
RG_HD u64 rg_mirror_prc(u32 w, u64 c) { return c - (u64)(w >> 16); }

// Does any lane of the wave say so? (the host twin: the lane's own answer, or -- RG_MIRROR_TWIN_ANY, which only
// tests/host_check/mirror_twin.hip defines -- the answer the twin worked out for the lane's block of 64 groups beforehand)
RG_HD bool rg_mirror_any(bool mine) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_ballot_w64(mine) != 0;
#elif defined(RG_MIRROR_TWIN_ANY)
    return RG_MIRROR_TWIN_ANY(mine);
#else
    return mine;
#endif
}

// rg_load_group for the cached lane kernel (RG_NX_PREFETCH, no late loads, state columns through the cache) with the P words of
// the plane in the place of the 2 P cells of RG_COL_MATCH / RG_COL_PR_COMMIT: same batch, same order otherwise. The decode runs
// once `commit` and the words have arrived; the rare-path batch behind them stays in flight (memory returns a wave's loads in
// order). The escapes are looked for by the whole wave at once: the steady wave pays one ballot, not 2 P branches.
template <int P, typename IX, bool NTM> RG_HD void rg_load_group_pk(RgGroup<P> &r, const RgState &st, const RgMsgs &ms, const u32 *pk, IX g) {
    r.mf = rg_ld_stream<NTM>(&rg_at(ms.mflags, g));
    r.pf = rg_at(st.pflags, g);
    r.cfg = rg_at(st.cfg, g);
    r.commit = rg_at(st.commit, g);
    r.lo = rg_at(st.lo, g);
    r.hi = rg_at(st.hi, g);
    r.adv = rg_pub_load(st, g);
    u32 w[P];
#pragma unroll
    for (int p = 0; p < P; p++) {
        const IX o = (IX)p * (IX)st.stride + g;
        w[p] = rg_at(pk, o);
        r.mi[p] = rg_ld_stream<NTM>(&rg_at(ms.mi, o));
        r.mc[p] = rg_ld_stream<NTM>(&rg_at(ms.mc, o));
    }
    rg_prefetch_rare<P, IX>(r, st, ms, g);
    u32 esc = 0; // bit p: matched of slot p is not in its word, bit 8 + p: committed_index
#pragma unroll
    for (int p = 0; p < P; p++) {
        r.mt[p] = rg_mirror_match(w[p], r.commit);
        r.pc[p] = rg_mirror_prc(w[p], r.commit);
        esc |= ((w[p] & 0xffffu) == RG_MIRROR_MT_ESC ? 1u << p : 0u) | ((w[p] >> 16) == RG_MIRROR_PC_ESC ? 1u << (8 + p) : 0u);
    }
    // An escape (rare: a lagging or probing peer, a freshly elected leader, an index 16 bits away from the commit index) is served
    // from the columns by the WHOLE wave: every lane re-reads its 2 P cells -- in the lanes and slots that needed no escape the
    // decoded value and the cell are the same thing -- so the loads are unconditional inside ONE wave-uniform branch, and the
    // steady wave pays one ballot. Loaded under the lanes' own condition (or per slot under a ballot of its own), each cell keeps
    // its decoded and its loaded value alive side by side until they are merged: 136 VGPRs at five slots instead of 127, a wave
    // per SIMD less, 180 at seven. (32-bit offsets opaque next to the access, rg_u32o, so that no cell address of this branch is
    // hoisted out of it as a 64-bit register pair.)
    if (__builtin_expect(rg_mirror_any(esc != 0), 0)) {
        typedef typename std::conditional<std::is_same<IX, u32>::value, rg_u32o, IX>::type IXO;
#pragma unroll
        for (int p = 0; p < P; p++) {
            const IXO o = (IXO)(u64)((IX)p * (IX)st.stride + g);
            r.mt[p] = rg_at(st.match, o);
            r.pc[p] = rg_at(st.prc, o);
        }
    }
}

// The P words of one group, from the registers the tick leaves (behind rg_store_group: r.commit is what RG_COL_COMMIT holds now).
// A slot WITHOUT a Progress gets the word 0 and never an escape: its `matched` register is zeroed by the next tick whatever the
// loader delivers and its `committed_index` is neither read nor stored by any tick, so what it decodes to (the commit index, twice)
// is never looked at -- encoded like the others it would be an escape for good as soon as the group's commit index passes 32 767,
// and every wave of a shard with absent peers would re-read its columns in every tick.
// -> does any field of this group hold an escape (the next packed tick of its wave goes to the columns)?
template <int P, typename IX> RG_HD bool rg_store_mirror(const RgGroup<P> &r, u32 *pk, u64 stride, IX g) {
    const u32 present = RG_CFG_PRESENT(r.cfg);
    bool esc = false;
#pragma unroll
    for (int p = 0; p < P; p++) {
        const u32 w = ((present >> p) & 1u) ? rg_mirror_encode(r.mt[p], r.pc[p], r.commit) : 0u;
        esc = esc || (w & 0xffffu) == RG_MIRROR_MT_ESC || (w >> 16) == RG_MIRROR_PC_ESC;
        rg_at(pk, (IX)p * (IX)stride + g) = w;
    }
    return esc;
}

// ---- write-behind (k_tick_mirror_wb) -------------------------------------------------------------------------------------------
// While packed launches follow one another nothing reads the two u64 columns: the next tick reads the words. The write-behind
// store therefore leaves the match / committed_index cells alone and stores the words only -- per WAVE (a block of 64 consecutive
// groups), under one invariant:
//   no word of the block holds an escape  ->  the words are the state; the block's cells may be stale
//   some word of the block holds one      ->  the block's cells are current
// The wave ballots the escapes of the words it is about to store. A wave with one stores EVERY match / committed_index cell of
// its slots that have a Progress, from the registers (so the loader's wave-uniform escape branch, which re-reads all 2 P cells of
// every lane, finds what the columns of a write-through engine would hold); a wave without one stores none. The cells of a slot
// WITHOUT a Progress are never stored -- as rg_store_group leaves them (no event is applied to such a slot, so it has no dirty
// bit; RG_OPT_WAVE_ST, which would widen a neighbour's store over them, switches write-behind off: rg_tick_kernels.h).
// -> does any field of this group hold an escape
template <int P, typename IX> RG_HD bool rg_store_mirror_wb(const RgGroup<P> &r, const RgState &st, u32 *pk, IX g) {
    const u32 present = RG_CFG_PRESENT(r.cfg);
    u32 w[P];
    bool esc = false;
#pragma unroll
    for (int p = 0; p < P; p++) {
        w[p] = ((present >> p) & 1u) ? rg_mirror_encode(r.mt[p], r.pc[p], r.commit) : 0u;
        esc = esc || (w[p] & 0xffffu) == RG_MIRROR_MT_ESC || (w[p] >> 16) == RG_MIRROR_PC_ESC;
    }
    if (__builtin_expect(rg_mirror_any(esc), 0)) {
        typedef typename std::conditional<std::is_same<IX, u32>::value, rg_u32o, IX>::type IXO;
#pragma unroll
        for (int p = 0; p < P; p++) {
            if (!((present >> p) & 1u)) continue;
            const IXO o = (IXO)(u64)((IX)p * (IX)st.stride + g);
            rg_at(st.match, o) = r.mt[p];
            rg_at(st.prc, o) = r.pc[p];
        }
    }
#pragma unroll
    for (int p = 0; p < P; p++) rg_at(pk, (IX)p * (IX)st.stride + g) = w[p];
    return esc;
}

// The settle (k_mirror_settle, rg_mirror_settle): the two columns written from the plane, once, when something is about to look
// at them or to write them. One lane per group, one wave per block of 64 groups: a block whose words hold an escape is left
// alone (its cells are current, and an escaped field cannot be decoded); in every other block each slot the cfg word names as
// present gets match = decode(word, commit) and committed_index = decode(word, commit). Nothing else is touched.
RG_HD void rg_mirror_settle_group(const RgState &st, const u32 *pk, u32 P, u64 g) {
    bool esc = false;
    for (u32 p = 0; p < P; p++) {
        const u32 w = pk[(u64)p * st.stride + g];
        esc = esc || (w & 0xffffu) == RG_MIRROR_MT_ESC || (w >> 16) == RG_MIRROR_PC_ESC;
    }
    if (rg_mirror_any(esc)) return;
    const u64 c = st.commit[g];
    const u32 present = RG_CFG_PRESENT(st.cfg[g]);
    for (u32 p = 0; p < P; p++) {
        if (!((present >> p) & 1u)) continue;
        const u64 o = (u64)p * st.stride + g;
        const u32 w = pk[o];
        st.match[o] = rg_mirror_match(w, c);
        st.prc[o] = rg_mirror_prc(w, c);
    }
}

// What the host learns about escapes without a synchronisation. A wave that stored an escape adds 1 to a count in device memory
// (ONE atomic per such wave: none at all on a steady stream), and every 16th of them copies the running count into a word of
// pinned host memory. rg_plan_tick compares that word over windows of RG_MIRROR_WINDOW mirror launches: where more than one wave in
// RG_MIRROR_WAVE_SHARE stores an escape -- a shard under leader-term rollover: a fresh leader's followers have matched = 0, a
// probing peer lags far behind -- the packed launches would read the words AND the columns, so the engine goes back to
// k_tick_lane for good (rgr_mirror_info.off = 2).
#define RG_MIRROR_WINDOW 32u
#define RG_MIRROR_WAVE_SHARE 8u
struct RgMirrorEsc {
    u32 *count; // device
    u32 *host;  // pinned host memory, device-visible
};
RG_D void rg_mirror_note_escape(bool esc, const RgMirrorEsc &e) {
#if defined(__HIP_DEVICE_COMPILE__)
    const u64 b = __builtin_amdgcn_ballot_w64(esc);
    if (b != 0 && (threadIdx.x & 63u) == (u32)__builtin_ctzll(b)) {
        const u32 n = atomicAdd(e.count, 1u) + 1u;
        if ((n & 15u) == 0) *(volatile u32 *)e.host = n;
    }
#endif
}
