// GENERATED from include/raftgroups_conf.h by tools/gen_rust_bindings.py -- do not edit.
// The batched conf change (apply_conf and post_conf_change on the device), an extension of raftgroups.rs (same library).
// tests/test_conf_change_host.py checks that it names every rgc_* export of libraftgroups.so with the header's arity.
#![allow(non_camel_case_types, dead_code)]
use super::raftgroups::*;

pub const RGC_CONF_VERSION: u32 = 1;
pub const RGC_CONF_NONE: u32 = 0;
pub const RGC_CONF_DONE: u32 = 1;
pub const RGC_CONF_DEMOTED: u32 = 2;
pub const RGC_CONF_NOT_LED: u32 = 3;
pub const RGC_CONF_HOST: u32 = 4;
pub const RGC_CONF_FAULT: u32 = 5;
pub const RGC_CONF_EV_COMMITTED: u32 = 0x1;
pub const RGC_CONF_EV_TRANSFER_ABORTED: u32 = 0x2;

#[repr(C)]
pub struct RgcConfRec {
    pub group: u64,
    pub cfg: u32,
    pub reserved: u32,
}

#[repr(C)]
pub struct RgcConfResp {
    pub commit: u64,
    pub last_index: u64,
    pub cfg: u32,
    pub out: u32,
    pub n_items: u32,
    pub status: u8,
    pub events: u8,
    pub added: u8,
    pub removed: u8,
}

#[repr(C)]
pub struct RgcConfOut {
    pub status: *mut u8,
    pub events: *mut u8,
    pub commit: *mut u64,
    pub items: *mut RgSendItem,
    pub item_cap: u64,
    pub count: *mut u32,
}

extern "C" {
    pub fn rgc_conf_version() -> u32;
    pub fn rgc_apply_conf(h: *mut RgEngine, host_recs: *const RgcConfRec, n: u64, host_resp: *mut RgcConfResp, max_entries_per_msg: u64, flags: u32, host_items: *mut RgSendItem, item_cap: u64, n_items: *mut u64) -> i32;
    pub fn rgc_apply_conf_device(h: *mut RgEngine, dev_sel: *const u8, dev_cfg: *const u32, max_entries_per_msg: u64, flags: u32, dev_out: *const RgcConfOut) -> i32;
}
