// GENERATED from include/raftgroups_mirror.h by tools/gen_rust_bindings.py -- do not edit.
// The dense tick's read mirror (its counters), an extension of raftgroups.rs (same library).
// tests/test_mirror_host.py checks that it names the rgr_* export of libraftgroups.so -- an OBJECT holding the function's address.
#![allow(non_camel_case_types, dead_code)]
use super::raftgroups::*;

pub const RGR_MIRROR_VERSION: u32 = 1;

extern "C" {
    pub static rgr_mirror_stats: unsafe extern "C" fn(h: *const RgEngine, info: *mut RgrMirrorInfo) -> i32;
}

#[repr(C)]
pub struct RgrMirrorInfo {
    pub packed_launches: u64,
    pub build_launches: u64,
    pub plane_bytes: u64,
    pub present: u32,
    pub valid: u32,
    pub off: u32,
    pub version: u32,
}
