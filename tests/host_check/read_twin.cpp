// read_twin.cpp -- the ReadIndex arithmetic of csrc/rg_read.h on the host, driven by a script (tests/test_read_index_host.py).
// A plain C++17 program: no HIP, no library -- the header is host/device-clean, and this is the build that shows it (twice: the
// second one with -fsanitize=address,undefined). It keeps the queue columns the way the engine lays them out (ring slots
// depth-major, one count | head word per group) and applies every batch the way k_read_list does: lazy term reset, one walk
// over a private copy that only counts the emitted states, one walk over the columns.
//
//   script:  "P depth G"                          header
//            "c g cfg commit term_lo term"        the group's RG_COL_CFG / COMMIT / TERM_LO / CUR_TERM as of now
//            "b g n" + n x "r ctx lease" | "a slot ctx flags"   one batch of records of group g, in arrival order
//   output:  per batch "s <status>..." (its requests), "e g ctx index" per read state; at the end "q g n ctx:index:acks ..."
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rg_read.h"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    unsigned P, depth;
    unsigned long long G;
    if (fscanf(f, "%u %u %llu", &P, &depth, &G) != 3 || depth < 1 || depth > RG_READ_MAX_DEPTH) return 2;
    const u64 stride = (G + 255) / 256 * 256;
    std::vector<u32> qw(stride, 0), cfg(G, 0);
    std::vector<u64> qterm(stride, 0), ctx((size_t)depth * stride, 0), idx((size_t)depth * stride, 0), commit(G, 0), lo(G, 0), term(G, 0);
    std::vector<u8> acks((size_t)depth * stride, 0);
    RgReadCols rc;
    rc.qw = qw.data();
    rc.qterm = qterm.data();
    rc.ctx = ctx.data();
    rc.idx = idx.data();
    rc.acks = acks.data();
    rc.stride = stride;
    rc.depth = depth;
    auto open = [&](u64 g) {
        RgReadPos p = {RG_READ_QW_N(qw[g]), RG_READ_QW_HEAD(qw[g]), depth};
        if (rg_read_sync_term(qterm[g], term[g], p)) qw[g] = 0;
        return p;
    };
    char op[8];
    std::vector<RgReadRec> recs;
    std::vector<u8> status;
    while (fscanf(f, "%7s", op) == 1) {
        unsigned long long g;
        if (op[0] == 'c') {
            unsigned c;
            unsigned long long cm, l, t;
            if (fscanf(f, "%llu %u %llu %llu %llu", &g, &c, &cm, &l, &t) != 5 || g >= G) return 2;
            cfg[g] = c;
            commit[g] = cm;
            lo[g] = l;
            term[g] = t;
        } else if (op[0] == 'b') {
            unsigned n;
            if (fscanf(f, "%llu %u", &g, &n) != 2 || g >= G) return 2;
            recs.assign(n, RgReadRec());
            status.assign(n, 0xff);
            for (unsigned k = 0; k < n; k++) {
                char kind[8];
                unsigned long long a, b, c;
                if (fscanf(f, "%7s %llu %llu %llu", kind, &a, &b, &c) != 4) return 2;
                RgReadRec &r = recs[k];
                r.group = g;
                r.orig = k;
                r.pad = 0;
                if (kind[0] == 'r') {
                    r.ctx = a;
                    r.slot = 0;
                    r.flags = RG_READ_REC_REQUEST | (b ? RG_READ_REC_LEASE : 0u);
                } else {
                    r.slot = (u32)a;
                    r.ctx = b;
                    r.flags = (u32)c;
                }
            }
            const RgReadPos p0 = open(g);
            RgReadRing ring = rg_read_ring(rc, g);
            RgReadCopy cp;
            memset(&cp, 0, sizeof(cp));
            for (u32 j = 0; j < p0.n; j++) {
                const u32 s = rg_read_slot_of(p0, j);
                cp.set(s, ring.ctx(s), ring.idx(s), ring.acks(s));
            }
            RgReadPos p = p0;
            unsigned counted = 0, emitted = 0;
            rg_read_walk(cp, p, cfg[g], commit[g], lo[g], recs.data(), 0, n, (u8 *)nullptr, [&](u64, u64) { counted++; });
            const RgReadPos dry = p;
            p = p0;
            std::vector<u64> out;
            rg_read_walk(ring, p, cfg[g], commit[g], lo[g], recs.data(), 0, n, status.data(), [&](u64 c, u64 i) {
                emitted++;
                out.push_back(c);
                out.push_back(i);
            });
            if (counted != emitted || dry.n != p.n || dry.head != p.head) {
                fprintf(stderr, "the counting walk and the real walk disagree: %u / %u states\n", counted, emitted);
                return 3;
            }
            qw[g] = RG_READ_QW(p.n, p.head);
            printf("s");
            for (unsigned k = 0; k < n; k++)
                if (recs[k].flags & RG_READ_REC_REQUEST) printf(" %u", (unsigned)status[k]);
            printf("\n");
            for (size_t k = 0; k < out.size(); k += 2) printf("e %llu %llu %llu\n", g, (unsigned long long)out[k], (unsigned long long)out[k + 1]);
        } else {
            return 2;
        }
    }
    fclose(f);
    for (u64 g = 0; g < G; g++) {
        const RgReadPos p = open(g);
        const RgReadRing ring = rg_read_ring(rc, g);
        printf("q %llu %u", (unsigned long long)g, p.n);
        for (u32 j = 0; j < p.n; j++) {
            const u32 s = rg_read_slot_of(p, j);
            printf(" %llu:%llu:%u", (unsigned long long)ring.ctx(s), (unsigned long long)ring.idx(s), ring.acks(s));
        }
        printf("\n");
    }
    return 0;
}
