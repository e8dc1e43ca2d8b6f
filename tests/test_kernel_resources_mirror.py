"""CPU-only guard, beside test_kernel_resources.py and with its tool: k_tick_mirror (the lane kernel with the read mirror,
raft_rs_amd/csrc/rg_mirror.h) keeps the lane kernel's register budget in BOTH modes -- the packed loader once cost it a wave
(136 VGPRs at five slots, while the escapes were loaded under the lanes' own condition)."""
import re

from test_kernel_resources import resource_usage


def mirror_rows(p):
    rows = {}
    for k, v in resource_usage(p).items():
        m = re.search(r"k_tick_mirrorILi%dEjLi([01])ELb([01])EE" % p, k)
        if m:
            rows[(int(m.group(1)), bool(int(m.group(2))))] = v  # (streamed messages, packed)
    assert sorted(rows) == [(0, False), (0, True), (1, False), (1, True)], sorted(rows)
    return rows


def test_mirror_kernel_keeps_the_lane_budget_at_five_slots():
    for key, r in mirror_rows(5).items():
        assert int(r["VGPRs"]) <= 128 and int(r["Occupancy [waves/SIMD]"]) >= 4 and int(r["ScratchSize [bytes/lane]"]) == 0, (key, r)


def test_mirror_kernel_at_seven_slots():
    for key, r in mirror_rows(7).items():
        assert int(r["Occupancy [waves/SIMD]"]) >= 3 and int(r["ScratchSize [bytes/lane]"]) == 0, (key, r)


def test_mirror_kernel_streams_what_the_lane_kernel_streams():
    """NTM = 1: the read-once message columns as non-temporal loads, as in k_tick_lane<.., 1>; the plane and the state never."""
    rows = mirror_rows(5)
    for packed in (False, True):
        assert rows[(0, packed)].get("nt loads", 0) == 0 and rows[(0, packed)].get("nt stores", 0) == 0, rows[(0, packed)]
        assert rows[(1, packed)].get("nt loads", 0) >= 11 and rows[(1, packed)].get("nt stores", 0) == 0, rows[(1, packed)]
