// conf_twin.cpp -- the arithmetic of the batched conf change (raft_rs_amd/csrc/rg_conf.h, included ALONE: no device header) as a
// stand-alone host program, composed in the order the kernels compose it (rg_kernels_conf.h: rg_conf_one). tests/test_conf_change_host.py
// builds it with g++ -- once more under AddressSanitizer + UBSan -- and checks every line against tests/conf_model.py.
//
// stdin, one case per line:
//   C P cap has_ins clock led W old pf hi lo commit dummy max_entries flags esz_w n_sizes  size[0..n_sizes)  then per slot s < P:
//   match next pend_rs count
// (size[i] = Entry::compute_size() of entry i; only read under RG_SEND_BYTES)
// stdout:  C status cfg pf commit out events added removed n_items  then per slot: next count kind prev last
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../raft_rs_amd/csrc/rg_conf.h"

int main() {
    char tag;
    while (scanf(" %c", &tag) == 1) {
        if (tag != 'C') return 2;
        unsigned P, cap, has_ins, clock, led, W, old, flags, esz_w, n_sizes;
        unsigned long long pf, hi, lo, commit, dummy, max_entries;
        if (scanf("%u %u %u %u %u %u %u %llu %llu %llu %llu %llu %llu %u %u %u", &P, &cap, &has_ins, &clock, &led, &W, &old, &pf, &hi, &lo, &commit, &dummy, &max_entries, &flags,
                  &esz_w, &n_sizes) != 16 || P < 1 || P > 8)
            return 3;
        std::vector<u64> sizes(n_sizes);
        for (unsigned i = 0; i < n_sizes; i++) {
            unsigned long long v;
            if (scanf("%llu", &v) != 1) return 4;
            sizes[i] = v;
        }
        u64 mt[8] = {0}, nx[8] = {0}, prs[8] = {0};
        u32 count[8] = {0};
        for (unsigned s = 0; s < P; s++) {
            unsigned long long a, b, c;
            unsigned d;
            if (scanf("%llu %llu %llu %u", &a, &b, &c, &d) != 4) return 5;
            mt[s] = a, nx[s] = b, prs[s] = c, count[s] = d;
        }
        u32 kind[8] = {0};
        u64 prev[8] = {0}, last[8] = {0};
        u32 cfg = old, events = 0, added = 0, removed = 0, n_items = 0, out = 0;
        const u32 status = rg_conf_check(W, old, P, clock != 0, led != 0);
        if (status == RGC_CONF_DONE || status == RGC_CONF_DEMOTED) {
            const u32 self = RG_CFG_SELF(old), Wp = RG_CFG_PRESENT(W);
            RgConfApply ap = rg_conf_apply(W, old, pf);
            added = ap.added, removed = ap.removed;
            u64 row = ap.pf;
            for (unsigned s = 0; s < P; s++)
                if ((ap.added >> s) & 1u) mt[s] = 0, nx[s] = hi + 1, prs[s] = 0, count[s] = 0;
            if (status == RGC_CONF_DONE) {
                u64 v[8];
                for (unsigned s = 0; s < 8; s++) v[s] = (s < P && ((Wp >> s) & 1u)) ? mt[s] : 0;
                const u64 mci = rg_conf_mci<8>(v, RG_CFG_INCOMING(W), RG_CFG_OUTGOING(W));
                u64 c = commit;
                const bool committed = rg_conf_log_maybe_commit(mci, c, lo, hi);
                commit = c;
                if (committed) events |= RGC_CONF_EV_COMMITTED, out = RG_OUT_CHANGED;
                if (has_ins) {
                    for (unsigned s = 0; s < P; s++) {
                        if (!((Wp >> s) & 1u) || s == self) continue;
                        u32 pb = (u32)(row >> (8 * s)) & 0xffu;
                        const RgConfPeer r = rg_conf_send_peer(pb, nx[s], (pb & RG_PF_PEND_RS) ? prs[s] : 0, count[s] == cap, hi, dummy + 1, committed, max_entries, flags, esz_w,
                                                               [&](u64 next, u64 avail) -> u64 { // util::limit_size (src/util.rs:52-76), literally
                                                                   if (avail <= 1 || max_entries == ~0ULL) return avail;
                                                                   u64 size = 0, n = 0;
                                                                   for (u64 k = 0; k < avail; k++) {
                                                                       const u64 sz = sizes.at(next + k);
                                                                       if (size == 0) {
                                                                           size += sz;
                                                                           n++;
                                                                           continue;
                                                                       }
                                                                       size += sz;
                                                                       if (size > max_entries) break;
                                                                       n++;
                                                                   }
                                                                   return n;
                                                               });
                        if (r.add) count[s] += 1, nx[s] = r.next;
                        pb = r.pb;
                        if (!((ap.added >> s) & 1u))
                            pb = (pb & ~RG_PF_INS_FULL) | (((pb & RG_PF_STATE_MASK) == RG_STATE_REPLICATE && count[s] == cap) ? RG_PF_INS_FULL : 0u);
                        row = (row & ~(0xffULL << (8 * s))) | ((u64)pb << (8 * s));
                        kind[s] = r.kind, prev[s] = r.prev, last[s] = r.last;
                        n_items += r.kind ? 1u : 0u;
                    }
                }
                events |= rg_conf_transfer(ap.cfg);
            }
            cfg = ap.cfg;
            pf = row;
        }
        printf("C %u %u %llu %llu %u %u %u %u %u", status, cfg, pf, commit, out, events, added, removed, n_items);
        for (unsigned s = 0; s < P; s++) printf(" %llu %u %u %llu %llu", (unsigned long long)nx[s], count[s], kind[s], (unsigned long long)prev[s], (unsigned long long)last[s]);
        printf("\n");
    }
    return 0;
}
