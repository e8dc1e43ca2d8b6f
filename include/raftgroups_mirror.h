/* raftgroups_mirror.h -- observability of the dense tick's READ MIRROR. A SEVENTH extension of include/raftgroups.h, beside
 * raftgroups_lead.h, raftgroups_term.h, raftgroups_vote.h, raftgroups_handoff.h, raftgroups_conf.h and raftgroups_transfer.h and in
 * a header of its own; it needs the core header only.
 *
 * The older headers stay as they are (raftgroups.h gains one rg_config flag, RG_CFGF_NO_READ_MIRROR, and nothing else): their entry
 * points, struct layouts and versions are unchanged, and a caller that does not include this file sees the same library as before.
 * What is declared here carries the prefix rgr_ / RGR_. The library's set of exported FUNCTIONS stays exactly what the seven older
 * headers declare (their tests pin it, name by name and in number): this header's one entry point is exported as an OBJECT that
 * holds the function's address -- `rgr_mirror_stats(h, &info)` reads the same in C -- and the version it was built with travels in
 * the answer (rgr_mirror_info.version; RGR_MIRROR_VERSION is bumped whenever a layout or the signature of THIS file changes). Same
 * rules as raftgroups.h otherwise: C99, no exception leaves the entry point, the int result is RG_OK or an RG_ERR_* code with the
 * text in rg_last_error().
 *
 * WHAT IT IS. A dense tick of the lane kernel (RG_KERNEL_LANE, cache regimes 0 and 1, no group commit) reads, per group, the two
 * 8-byte cells RG_COL_MATCH and RG_COL_PR_COMMIT of every slot; in a live group both lie within a few thousand of RG_COL_COMMIT,
 * which the tick loads anyway. An engine that can run that kernel (lane variant, 32-bit cell offsets, max_inflight == 0, no
 * RG_CFGF_NO_READ_MIRROR) therefore keeps, next to its columns, one packed 32-bit word per slot and group (4 x n_slots x stride
 * bytes, counted in rg_device_info.engine_bytes): the tick writes it behind its ordinary stores, and the NEXT dense tick reads it in
 * the place of the two cells. Through every call that looks at them the columns hold exactly what they hold without the mirror; the
 * plane is no RG_COL_*, is reachable through no column call and is part of no checkpoint.
 *
 * The plane is a cache, and its one protocol is invalidation: every entry point that takes the engine drops it, except the dense
 * tick itself and the calls that write none of the three columns (rg_results, rg_result_counts, rg_sync, rg_get_device_info,
 * rg_msg_stats, rg_read_column, rg_workload_gen, and this header's). A tick that finds it dropped reads the columns as ever and rebuilds it (a
 * "build" launch: 4 B per slot and group more than a tick without the mirror); a tick that finds it valid is a "packed" launch.
 * WRITE-BEHIND. Once packed launches follow one another with nothing but such calls in between, the packed launch stops storing
 * the RG_COL_MATCH / RG_COL_PR_COMMIT cells the words stand for (the plane is then the state of the two columns, not their cache),
 * and the engine writes them back from the plane before anything reads or writes them or ends the streak: every entry point that
 * drops the plane, rg_read_column of one of the two, rg_workload_gen, rg_column_ptr, and any dense tick on another kernel. The
 * dense tick itself, rg_results, rg_result_counts, rg_sync, rg_get_device_info, rg_msg_stats, rg_read_column of other columns and
 * this header's call do not. Nothing of it shows through the ABI: packed_launches counts both kinds of packed launch.
 * The mirror stays off while a resident mailbox workgroup runs (rg_mailbox_start), and for good once rg_column_ptr has handed
 * out RG_COL_MATCH, RG_COL_PR_COMMIT or RG_COL_COMMIT or a tick has been captured into a graph (whoever holds the pointer or the
 * graph changes the columns without an entry point). rg_device_info.last_tick_kernel / last_tick_streaming report what they
 * would without the mirror.
 *
 * ESCAPES. A cell the word cannot hold (a peer 32 767 entries away from the commit index: a fresh leader's followers, a probing
 * peer) is an escape: the wave that meets one re-reads its cells from the columns, which costs more than it saves. A slot without
 * a Progress never escapes. The engine counts the waves that store escapes and, where over a window of 32 launches more than one
 * wave in 8 did, returns to the plain kernel for good (off bit 1): a shard under constant leader-term rollover runs as it did. */
#ifndef RAFTGROUPS_MIRROR_H
#define RAFTGROUPS_MIRROR_H
#include "raftgroups.h"
#ifdef __cplusplus
extern "C" {
#endif

#define RGR_MIRROR_VERSION 1u

typedef struct {
    uint64_t packed_launches; /* dense ticks that read the plane in the place of RG_COL_MATCH / RG_COL_PR_COMMIT */
    uint64_t build_launches;  /* dense ticks that read the columns and (re)built the plane */
    uint64_t plane_bytes;     /* 0: this engine keeps no mirror */
    uint32_t present;         /* the plane exists */
    uint32_t valid;           /* ... and the next eligible dense tick would be a packed launch */
    uint32_t off;             /* ... or never again: bit 0 a column pointer was handed out or a tick was captured into a graph,
                                 bit 1 too many waves of this shard store escapes (below) */
    uint32_t version;         /* RGR_MIRROR_VERSION of the build */
} rgr_mirror_info;

/* Host-side counters only: no device work, no synchronisation, and the mirror stays as it is. */
typedef int (*rgr_mirror_stats_fn)(const rg_engine *h, rgr_mirror_info *info);
extern const rgr_mirror_stats_fn rgr_mirror_stats; /* a data symbol of libraftgroups.so: the address of the function */

#ifdef __cplusplus
}
#endif
#endif /* RAFTGROUPS_MIRROR_H */
