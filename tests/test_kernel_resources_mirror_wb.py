"""CPU-only guard, beside test_kernel_resources_mirror.py and with its tool: k_tick_mirror_wb (the packed launch of a streak, which
no longer stores the match / committed_index cells: raft_rs_amd/csrc/rg_mirror.h, "write-behind") keeps the lane kernel's register
budget, streams nothing it stores, and leaves the four k_tick_mirror instantiations what they were."""
import re

from test_kernel_resources import resource_usage
from test_kernel_resources_mirror import mirror_rows


def wb_rows(p):
    rows = {}
    for k, v in resource_usage(p).items():
        m = re.search(r"k_tick_mirror_wbILi%dEjLi([01])EE" % p, k)
        if m:
            rows[int(m.group(1))] = v  # (streamed messages)
    assert sorted(rows) == [0, 1], sorted(rows)
    return rows


def test_write_behind_kernel_keeps_the_lane_budget_at_five_slots():
    for key, r in wb_rows(5).items():
        assert int(r["VGPRs"]) <= 128 and int(r["Occupancy [waves/SIMD]"]) >= 4 and int(r["ScratchSize [bytes/lane]"]) == 0, (key, r)


def test_write_behind_kernel_at_seven_slots():
    for key, r in wb_rows(7).items():
        assert int(r["Occupancy [waves/SIMD]"]) >= 3 and int(r["ScratchSize [bytes/lane]"]) == 0, (key, r)


def test_write_behind_kernel_has_no_streamed_stores():
    for p in (5, 7):
        rows = wb_rows(p)
        assert rows[0].get("nt stores", 0) == 0 and rows[0].get("nt loads", 0) == 0, rows[0]
        assert rows[1].get("nt stores", 0) == 0 and rows[1].get("nt loads", 0) >= 11, rows[1]


def test_the_four_write_through_instantiations_are_what_they_were():
    """Exactly four kernels under the old name (mirror_rows asserts it), inside the budget test_kernel_resources_mirror.py pins."""
    for p, waves in ((5, 4), (7, 3)):
        for key, r in mirror_rows(p).items():
            assert int(r["Occupancy [waves/SIMD]"]) >= waves and int(r["ScratchSize [bytes/lane]"]) == 0, (p, key, r)
            assert r.get("nt stores", 0) == 0, (p, key, r)
