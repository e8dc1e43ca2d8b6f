// GENERATED from include/raftgroups_transfer.h by tools/gen_rust_bindings.py -- do not edit.
// The batched leader transfer (handle_transfer_leader on the device), an extension of raftgroups.rs (same library).
// tests/test_transfer_host.py checks that it names every rgm_* export of libraftgroups.so with the header's arity.
#![allow(non_camel_case_types, dead_code)]
use super::raftgroups::*;

pub const RGM_TRANSFER_VERSION: u32 = 1;
pub const RGM_XFER_NONE: u32 = 0;
pub const RGM_XFER_STARTED: u32 = 1;
pub const RGM_XFER_SELF: u32 = 2;
pub const RGM_XFER_IN_PROGRESS: u32 = 3;
pub const RGM_XFER_LEARNER: u32 = 4;
pub const RGM_XFER_NO_PROGRESS: u32 = 5;
pub const RGM_XFER_NOT_LED: u32 = 6;
pub const RGM_XFER_FAULT: u32 = 7;
pub const RGM_XFER_EV_TIMEOUT_NOW: u32 = 0x1;
pub const RGM_XFER_EV_APPEND: u32 = 0x2;
pub const RGM_XFER_EV_ABORTED_PREVIOUS: u32 = 0x4;

#[repr(C)]
pub struct RgmTransferRec {
    pub group: u64,
    pub slot: u32,
    pub reserved: u32,
}

#[repr(C)]
pub struct RgmTransferResp {
    pub last_index: u64,
    pub matched: u64,
    pub cfg: u32,
    pub n_items: u32,
    pub status: u8,
    pub events: u8,
    pub previous: u8,
    pub reserved: u8,
    pub reserved2: u32,
}

#[repr(C)]
pub struct RgmTransferOut {
    pub status: *mut u8,
    pub events: *mut u8,
    pub items: *mut RgSendItem,
    pub item_cap: u64,
    pub count: *mut u32,
}

extern "C" {
    pub fn rgm_transfer_version() -> u32;
    pub fn rgm_transfer_leader(h: *mut RgEngine, host_recs: *const RgmTransferRec, n: u64, host_resp: *mut RgmTransferResp, max_entries_per_msg: u64, flags: u32, host_items: *mut RgSendItem, item_cap: u64, n_items: *mut u64) -> i32;
    pub fn rgm_transfer_leader_device(h: *mut RgEngine, dev_to: *const u8, max_entries_per_msg: u64, flags: u32, dev_out: *const RgmTransferOut) -> i32;
}
