// GENERATED from include/raftgroups_term.h by tools/gen_rust_bindings.py -- do not edit.
// The leader's term gate and the deposition, an extension of raftgroups.rs and raftgroups_lead.rs (same library).
// tests/test_term_gate_host.py checks that it names every rgt_* export of libraftgroups.so with the header's arity.
#![allow(non_camel_case_types, dead_code)]
use super::raftgroups::*;
use super::raftgroups_lead::*;

pub const RGT_TERM_VERSION: u32 = 1;
pub const RGT_GATE_EV_TRANSFER_ABORTED: u32 = 0x08;
pub const RGT_GATE_EV_STALE: u32 = 0x20;
pub const RGT_GATE_EV_NOT_LED: u32 = 0x40;
pub const RGT_GATE_EV_DEPOSED: u32 = 0x80;

#[repr(C)]
pub struct RgtLeadGateOut {
    pub flags: *mut u8,
    pub events: *mut u8,
    pub new_term: *mut u64,
    pub down: *mut u64,
    pub down_cap: u64,
}

#[repr(C)]
pub struct RgtDeposeRec {
    pub follow_group: u64,
    pub lead_group: u64,
    pub term: u64,
    pub reserved: u64,
}

extern "C" {
    pub fn rgt_term_version() -> u32;
    pub fn rgt_lead_gate_device(h: *mut RgEngine, dev_msgs: *const RgMsgs, dev_m_term: *const u64, dev_out: *const RgtLeadGateOut, host_counts: *mut u64) -> i32;
    pub fn rgt_lead_gate_counts(h: *const RgEngine) -> *const u64;
    pub fn rgt_follow_depose(h: *mut RgEngine, host_recs: *const RgtDeposeRec, n: u64, host_resp: *mut RgHandoffResp) -> i32;
    pub fn rgt_follow_depose_device(h: *mut RgEngine, dev_events: *const u8, dev_new_term: *const u64, dev_lead: *const u64, dev_out: *const RgHandoffOut) -> i32;
    pub fn rgt_follow_depose_scan_device(h: *mut RgEngine, dev_msg_flags: *const u8, dev_term: *const u64, dev_lead: *const u64, dev_out: *const RgHandoffOut) -> i32;
}
