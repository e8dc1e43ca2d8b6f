// transfer_twin.cpp -- the arithmetic of the batched leader transfer (raft_rs_amd/csrc/rg_transfer.h, included ALONE: no device
// header) as a stand-alone host program, composed in the order the kernels compose it (rg_kernels_transfer.h: rg_transfer_one).
// tests/test_transfer_host.py builds it with g++ -- once more under AddressSanitizer + UBSan -- and checks every line against
// tests/transfer_model.py.
//
// stdin, one case per line:
//   T P cap has_ins clock led t old pf hi dummy cur_term tag cell max_entries flags esz_w n_sizes  size[0..n_sizes)  then the cells of
//   the transferee's slot (of slot 0 where t >= P): match next pend_rs count
// (size[i] = Entry::compute_size() of entry i; only read under RG_SEND_BYTES)
// stdout:  T status cfg pf events previous matched cell next count kind prev last
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../raft_rs_amd/csrc/rg_transfer.h"

int main() {
    char tag_c;
    while (scanf(" %c", &tag_c) == 1) {
        if (tag_c != 'T') return 2;
        unsigned P, cap, has_ins, clock, led_in, t, old, cell, flags, esz_w, n_sizes;
        unsigned long long pf, hi, dummy, cur_term, tag, max_entries;
        if (scanf("%u %u %u %u %u %u %u %llu %llu %llu %llu %llu %u %llu %u %u %u", &P, &cap, &has_ins, &clock, &led_in, &t, &old, &pf, &hi, &dummy, &cur_term, &tag, &cell,
                  &max_entries, &flags, &esz_w, &n_sizes) != 17 || P < 1 || P > 8)
            return 3;
        std::vector<u64> sizes(n_sizes);
        for (unsigned i = 0; i < n_sizes; i++) {
            unsigned long long v;
            if (scanf("%llu", &v) != 1) return 4;
            sizes[i] = v;
        }
        unsigned long long mt, nx, prs;
        unsigned count;
        if (scanf("%llu %llu %llu %u", &mt, &nx, &prs, &count) != 4) return 5;
        const u32 ts = t < P ? t : 0u;
        // with the clock layer the kernel derives `led` from the cell; the line's flag says what the cell must give
        const bool led = clock ? rg_term_led(cell, tag, cur_term) : true;
        if (clock && led != (led_in != 0)) return 6;
        u32 pb = (u32)(pf >> (8 * ts)) & 0xffu;
        u32 kind = 0, cfg = old, events = 0, previous = 0;
        u64 prev = 0, last = 0, next = nx;
        const u64 matched = (t < P && ((RG_CFG_PRESENT(old) >> ts) & 1u)) ? mt : 0;
        const u32 status = rg_transfer_check(t, old, P, clock != 0, led);
        if (status == RGM_XFER_STARTED || status == RGM_XFER_SELF) {
            const RgTransferWord w = rg_transfer_word(status, t, old);
            cfg = w.cfg, events = w.events, previous = w.previous;
            if (status == RGM_XFER_STARTED) {
                if (clock) (void)rg_transfer_clock(cell, tag, cur_term);
                events |= rg_transfer_first(mt, hi);
                if ((events & RGM_XFER_EV_APPEND) && has_ins) {
                    const RgConfPeer r = rg_conf_send_peer(pb, nx, (pb & RG_PF_PEND_RS) ? prs : 0, count == cap, hi, dummy + 1, true, max_entries, flags, esz_w,
                                                           [&](u64 nxt, u64 avail) -> u64 { // util::limit_size (src/util.rs:52-76), literally
                                                               if (avail <= 1 || max_entries == ~0ULL) return avail;
                                                               u64 size = 0, n = 0;
                                                               for (u64 k = 0; k < avail; k++) {
                                                                   const u64 sz = sizes.at(nxt + k);
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
                    if (r.add) count += 1, next = r.next;
                    pb = (r.pb & ~RG_PF_INS_FULL) | (((r.pb & RG_PF_STATE_MASK) == RG_STATE_REPLICATE && count == cap) ? RG_PF_INS_FULL : 0u);
                    pf = (pf & ~(0xffULL << (8 * ts))) | ((u64)pb << (8 * ts));
                    kind = r.kind, prev = r.prev, last = r.last;
                }
            }
        }
        printf("T %u %u %llu %u %u %llu %u %llu %u %u %llu %llu\n", status, cfg, pf, events, previous, (unsigned long long)matched, cell, (unsigned long long)next, count, kind,
               (unsigned long long)prev, (unsigned long long)last);
    }
    return 0;
}
