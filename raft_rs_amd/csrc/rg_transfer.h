// rg_transfer.h -- the batched leader transfer (include/raftgroups_transfer.h): the per-group arithmetic of
// Raft::handle_transfer_leader (src/raft.rs:1821-1889) for a group this store leads. Citations are relative to the pingcap/raft-rs
// v0.6.0 tree.
//
// Everything works on values: the kernels (rg_kernels_transfer.h) load a group's cells, call the functions and store what they
// return, so that a lane issues its loads before its first store. The order of a group is
//   rg_transfer_check   the checks in the reference's order: FAULT, NOT_LED, NO_PROGRESS, LEARNER, IN_PROGRESS, SELF, else STARTED
//   rg_transfer_word    the new cfg word: a previous transfer aborted (:1852), TRANSFEREE = t + 1 on STARTED (:1877)
//   rg_transfer_clock   election_elapsed = 0 (:1876) on the leader's clock cell
//   rg_transfer_first   MsgTimeoutNow (:1879-1885) or send_append (:1887)
// and, on an engine with device Inflights, one pass of rg_conf_send_peer (rg_conf.h) with allow_empty = true for the transferee.
//
// Host/device-clean like rg_conf.h: the kernels include it behind rg_common.h, tests/host_check/transfer_twin.cpp includes it ALONE
// and is checked against tests/transfer_model.py, sanitizers included -- nothing below needs a device header.
#pragma once
#include "rg_conf.h"

#include "../../include/raftgroups_transfer.h"

// The checks (the header's order). `t`: the record's slot, any value; `clock`: the leader's clock layer is on, `led`: rg_term_led of
// the group's cell (read only under `clock`). -> RGM_XFER_* but NONE
RG_D u32 rg_transfer_check(u32 t, u32 old, u32 P, bool clock, bool led) {
    const u32 self = RG_CFG_SELF(old), present = RG_CFG_PRESENT(old);
    if (t >= P || self >= P || !((present >> self) & 1u)) return RGM_XFER_FAULT;
    if (clock && !led) return RGM_XFER_NOT_LED;
    if (!((present >> t) & 1u)) return RGM_XFER_NO_PROGRESS;                                          // raft.rs:1822-1829
    if (!(((RG_CFG_INCOMING(old) | RG_CFG_OUTGOING(old)) >> t) & 1u)) return RGM_XFER_LEARNER;        // :1832-1839
    if (RG_CFG_TRANSFEREE(old) == t + 1u) return RGM_XFER_IN_PROGRESS;                                // :1841-1851
    if (t == self) return RGM_XFER_SELF;                                                              // :1860-1866
    return RGM_XFER_STARTED;
}

// The cfg word of a group whose status is SELF or STARTED: abort_leader_transfer of a transfer to another slot (:1852), then -- STARTED
// only -- lead_transferee = Some(t) (:1877). Every other bit is kept.
struct RgTransferWord {
    u32 cfg, events, previous; // events: RGM_XFER_EV_ABORTED_PREVIOUS or 0; previous: slot + 1 of the aborted transfer, else 0
};
RG_D RgTransferWord rg_transfer_word(u32 status, u32 t, u32 old) {
    RgTransferWord r;
    r.cfg = old;
    r.previous = RG_CFG_TRANSFEREE(old);
    r.events = r.previous ? RGM_XFER_EV_ABORTED_PREVIOUS : 0u;
    (void)rg_term_abort_transfer(r.cfg);
    if (status == RGM_XFER_STARTED) r.cfg |= (t + 1u) << 20;
    return r;
}

// election_elapsed = 0 (:1876) on the clock cell of a group whose status is STARTED. A tag that differs from RG_COL_CUR_TERM is a
// leadership the clock has not armed yet: the cell is left alone (the next rgx_lead_clock zeroes both counters before its
// increment). -> true = store `cell`
RG_D bool rg_transfer_clock(u32 &cell, u64 tag, u64 cur_term) {
    if (tag != cur_term) return false;
    const u32 c = rg_lead_pack(rg_lead_hb(cell), 0, false); // (STARTED: the group is led, the STOPPED bit is clear)
    const bool changed = c != cell;
    cell = c;
    return changed;
}

// The first message (:1878-1888)
RG_D u32 rg_transfer_first(u64 matched, u64 hi) { return matched == hi ? RGM_XFER_EV_TIMEOUT_NOW : RGM_XFER_EV_APPEND; }
