// rg_promote.h -- the promotion into an engine with device Inflights (include/raftgroups_handoff.h): what comes BEHIND the
// arithmetic of rg_handoff.h when the leader engine keeps the windows and the send decision itself -- the window resets of
// Raft::reset, the bcast_append that follows become_leader, the size record of the empty entry. Citations are relative to the
// pingcap/raft-rs v0.6.0 tree.
//
// The first appends are a CLOSED FORM, derived here from the stage rg_group_send (rg_send.h) runs for the out word
// RG_OUT_BECAME_LEADER | RG_OUT_APPENDED over the cells rg_handoff_promote_one has just written -- there is no decision left:
//   work set     present & ~self, below the engine's slot count (rg_send_request: `elected` and `bcast` both add `present`);
//   the window   Raft::reset -> Progress::reset -> ins.reset() (progress.rs:82-92; rg_send_serve: `elected` -> start = count = 0).
//                The reference resets the own Progress's window too; the stage never looks at that slot, this call empties it;
//   the state    every peer is Probe with no flag set (rg_handoff_progress), so is_paused() is false (progress.rs:210-216);
//   the entries  next = last_index (the index of the empty entry: Progress::new(last_index + 1) BEFORE the append, raft.rs:959-966,
//                1191-1194), so exactly ONE entry is left to send; pending_request_snapshot is 0 (reset); first_index =
//                dummy_index + 1 <= next, so nothing is compacted away (raft_log.rs:382-389);
//   the limits   one entry: max_entries_per_msg cannot split it, and util::limit_size keeps the first entry whatever its size
//                (util.rs:52-76; rg_limit_size: avail <= 1) -- neither limit nor RG_SEND_SKIP_BCAST_COMMIT (an append always
//                broadcasts, raft.rs:2049-2053) changes anything. With RG_SEND_BYTES the peer is never the host's (RG_SEND_HOST needs
//                avail > 1);
//   the message  send_append (raft.rs:773-819): prev_index = next - 1, one entry, last_index = next; Progress::update_state(last) of a
//                Probe peer pauses it (progress.rs:231-243) and leaves next alone; the loop's second pass finds it paused.
// So: every peer slot's flag byte becomes RG_STATE_PROBE | RG_PF_PAUSED, its window empty, its `next` cell stays, and it gets one
// work item {prev_index = hi - 1, last_index = hi, n_msgs = 1, RG_SEND_APPEND}. tests/test_promote_send_host.py holds this form
// against the reference's own stage and against rg_group_send itself, tests/test_promote_send_gpu.py the kernels.
//
// Host/device-clean like rg_handoff.h: the kernels (rg_kernels_promote.h) include it behind rg_common.h,
// tests/host_check/promote_send_twin.cpp includes it ALONE and is checked against tests/promote_send_model.py, sanitizers included.
#pragma once
#include "rg_handoff.h"

// prost's encoded_len_varint
RG_D u32 rg_promote_varint_len(u64 v) {
    u32 n = 1;
    while (v >= 0x80u) {
        v >>= 7;
        n++;
    }
    return n;
}
// Entry::compute_size() of the empty entry become_leader appends: {entry_type Normal, term, index, no data, no context} -- a
// default field is not encoded, the two others cost their tag byte and their varint (eraftpb: term = 2, index = 3).
RG_D u32 rg_promote_empty_entry_size(u64 term, u64 index) {
    return (term ? 1u + rg_promote_varint_len(term) : 0u) + (index ? 1u + rg_promote_varint_len(index) : 0u);
}

// What the promotion of one group leaves to the send side, from the cfg word and the flag row the promotion wrote (pr.cfg, pr.pf)
struct RgPromoteSend {
    u64 pf;      // the flag row behind the first appends
    u32 windows; // slots whose Inflights window becomes empty: every slot with a Progress, the own one included
    u32 peers;   // slots that get a message: those of `windows` but the own
    u32 n_items; // ... how many
};
RG_D RgPromoteSend rg_promote_send(u64 pf, u32 cfg, u32 P) {
    RgPromoteSend r;
    r.windows = RG_CFG_PRESENT(cfg) & ((1u << P) - 1u);
    r.peers = r.windows & ~(1u << RG_CFG_SELF(cfg));
    r.n_items = 0;
    RG_FOLLOW_UNROLL
    for (u32 s = 0; s < 8; s++) {
        if (!((r.peers >> s) & 1u)) continue;
        pf |= (u64)RG_PF_PAUSED << (8 * s); // (the byte is RG_STATE_PROBE: rg_handoff_progress)
        r.n_items++;
    }
    r.pf = pf;
    return r;
}
