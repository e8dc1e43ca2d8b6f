// GENERATED from include/raftgroups_lead.h by tools/gen_rust_bindings.py -- do not edit.
// The leader's clock, an extension of raftgroups.rs (same library). tests/test_lead_clock_host.py checks that it names every
// rgx_* export of libraftgroups.so with the header's arity.
#![allow(non_camel_case_types, dead_code)]
use super::raftgroups::*;

pub const RGX_LEAD_VERSION: u32 = 1;
pub const RG_LEAD_CLOCK_START_LED: u32 = 0x100;
pub const RG_LEAD_EV_BEAT: u32 = 0x1;
pub const RG_LEAD_EV_CHECK_QUORUM: u32 = 0x2;
pub const RG_LEAD_EV_STEPPED_DOWN: u32 = 0x4;
pub const RG_LEAD_EV_TRANSFER_ABORTED: u32 = 0x8;
pub const RG_LEAD_EV_NEW_TERM: u32 = 0x10;
pub const RG_HANDOFF_NO_LEAD: u64 = u64::MAX;

#[repr(C)]
pub struct RgLeadClockConfig {
    pub election_tick: u32,
    pub heartbeat_tick: u32,
    pub flags: u32,
    pub reserved: u32,
}

#[repr(C)]
pub struct RgLeadClockCell {
    pub group: u64,
    pub term: u64,
    pub election_elapsed: u32,
    pub heartbeat_elapsed: u32,
    pub led: u8,
    pub reserved: [u8; 7],
}

#[repr(C)]
pub struct RgLeadClockOut {
    pub events: *mut u8,
    pub beat: *mut u64,
    pub beat_cap: u64,
    pub down: *mut u64,
    pub down_cap: u64,
    pub hb_commit: *mut u64,
}

extern "C" {
    pub fn rgx_lead_version() -> u32;
    pub fn rgx_lead_clock_enable(h: *mut RgEngine, cfg: *const RgLeadClockConfig) -> i32;
    pub fn rgx_lead_clock_write(h: *mut RgEngine, host: *const RgLeadClockCell, n: u64) -> i32;
    pub fn rgx_lead_clock_read(h: *mut RgEngine, host_groups: *const u64, n: u64, host_out: *mut RgLeadClockCell) -> i32;
    pub fn rgx_lead_clock(h: *mut RgEngine, dev_out: *const RgLeadClockOut, host_counts: *mut u64) -> i32;
    pub fn rgx_lead_clock_counts(h: *const RgEngine) -> *const u64;
    pub fn rgx_follow_step_down(h: *mut RgEngine, host_recs: *const RgHandoffRec, n: u64, host_resp: *mut RgHandoffResp) -> i32;
    pub fn rgx_follow_step_down_device(h: *mut RgEngine, dev_events: *const u8, dev_lead: *const u64, dev_out: *const RgHandoffOut) -> i32;
}
