// GENERATED from include/raftgroups_vote.h by tools/gen_rust_bindings.py -- do not edit.
// The dense vote step, an extension of raftgroups.rs, raftgroups_lead.rs and raftgroups_term.rs (same library).
// tests/test_vote_step_host.py checks that it names every rgv_* export of libraftgroups.so with the header's arity.
#![allow(non_camel_case_types, dead_code)]
use super::raftgroups::*;
use super::raftgroups_lead::*;
use super::raftgroups_term::*;

pub const RGV_VOTE_VERSION: u32 = 1;
pub const RGV_VOTE_EV_LED: u32 = 0x20;
pub const RGV_VOTE_EV_TRANSFER_ABORTED: u32 = 0x40;
pub const RGV_VOTE_EV_DEPOSED: u32 = 0x80;

#[repr(C)]
pub struct RgvVoteOut {
    pub status: *mut u8,
    pub gate: *mut u8,
    pub events: *mut u8,
    pub term: *mut u64,
    pub commit: *mut u64,
    pub log_term: *mut u64,
    pub answered: *mut u64,
    pub answered_cap: u64,
}

#[repr(C)]
pub struct RgvVoteRec {
    pub follow_group: u64,
    pub lead_group: u64,
    pub term: u64,
    pub from: u64,
    pub index: u64,
    pub log_term: u64,
    pub commit: u64,
    pub commit_term: u64,
    pub priority: i64,
    pub kind: u32,
    pub flags: u32,
}

#[repr(C)]
pub struct RgvVoteResp {
    pub term: u64,
    pub commit: u64,
    pub log_term: u64,
    pub last_index: u64,
    pub gate: u32,
    pub events: u32,
    pub status: u32,
    pub reserved: u32,
}

extern "C" {
    pub fn rgv_vote_version() -> u32;
    pub fn rgv_follow_vote_device(h: *mut RgEngine, dev_msgs: *const RgFollowMsgs, dev_term: *const u64, dev_from: *const u64, dev_priority: *const i64, dev_hdr_flags: *const u8, dev_lead: *const u64, dev_out: *const RgvVoteOut, host_counts: *mut u64) -> i32;
    pub fn rgv_follow_vote_counts(h: *const RgEngine) -> *const u64;
    pub fn rgv_follow_vote(h: *mut RgEngine, host_recs: *const RgvVoteRec, n: u64, host_resp: *mut RgvVoteResp) -> i32;
}
