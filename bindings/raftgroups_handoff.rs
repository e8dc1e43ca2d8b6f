// GENERATED from include/raftgroups_handoff.h by tools/gen_rust_bindings.py -- do not edit.
// The promotion into an engine with device Inflights, an extension of raftgroups.rs (same library).
// tests/test_promote_send_host.py checks that it names every rgh_* export of libraftgroups.so with the header's arity.
#![allow(non_camel_case_types, dead_code)]
use super::raftgroups::*;

pub const RGH_HANDOFF_VERSION: u32 = 1;

#[repr(C)]
pub struct RghPromoteOut {
    pub out: RgHandoffOut,
    pub items: *mut RgSendItem,
    pub item_cap: u64,
    pub count: *mut u32,
}

extern "C" {
    pub fn rgh_handoff_version() -> u32;
    pub fn rgh_follow_promote(h: *mut RgEngine, host_recs: *const RgHandoffRec, n: u64, host_resp: *mut RgHandoffResp, max_entries_per_msg: u64, flags: u32, host_items: *mut RgSendItem, item_cap: u64, n_items: *mut u64) -> i32;
    pub fn rgh_follow_promote_device(h: *mut RgEngine, dev_result: *const u8, dev_lead: *const u64, dev_persisted: *const u64, max_entries_per_msg: u64, flags: u32, dev_out: *const RghPromoteOut) -> i32;
}
