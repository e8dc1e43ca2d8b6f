"""Time rgx_lead_clock at 1 M groups x 5 slots next to the two whole-shard calls it replaces.

    python tools/bench_lead_clock.py [--groups N] [--out profiles/lead_clock.txt]

Cases: (a) every group led and between timeouts; (b) heartbeat_tick = 4 with the counters staggered, so that a quarter of the
groups beats in every call, with hb_commit; (c) rg_quorum_recently_active + rg_heartbeat_commits (device destination) over the whole
shard, the only alternative before the clock layer. (a) and (b) are asynchronous calls, timed in batches between two
synchronisations; (c) synchronises by itself (its result goes to the host). Medians of the per-call times: WHOLE calls issued from Python
(a 32-byte memset and a launch each), an upper bound on the kernels' own times. Byte model (DESIGN.md
section 3): 21 B per stopped group, 25 B per led group between timeouts, 117 B per beating group at 5 slots."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8e12  # B/s, the MI355X's HBM


def median_call(fn, sync, calls=50, repeats=15):
    fn()
    sync()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        sync()
        ts.append((time.perf_counter() - t0) / calls)
    return statistics.median(ts)


def main():
    import torch
    import raft_rs_amd as rg
    E = rg.engine
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    G, P, HB = a.groups, 5, 4
    lines = []

    def engine(heartbeat_tick, stagger):
        eng = rg.Engine(G, P, device=0)
        eng.workload_init(rg.WL_MAJORITY)
        eng.lead_clock_enable(16383, heartbeat_tick,  # RG_GATE_CHECK_QUORUM | START_LED
                              0x1 | E.LEAD_CLOCK_START_LED)
        if stagger:
            cells = np.zeros(G, dtype=E.LEAD_CLOCK_CELL_DTYPE)
            cells["group"] = np.arange(G)
            cells["term"] = eng.read_column(E.COL.CUR_TERM)
            cells["heartbeat_elapsed"] = np.arange(G) % heartbeat_tick
            cells["led"] = 1
            eng.lead_clock_write(cells)
        return eng

    events = torch.zeros(G, dtype=torch.uint8, device="cuda")
    # (a) between timeouts: 16382 calls fit before the first timeout of either kind
    eng = engine(16382, False)
    t = median_call(lambda: eng.lead_clock(events, sync=False), eng.sync)
    lines.append("between_timeouts  %9.2f us   25 B/group  %.3f of 8 TB/s" % (t * 1e6, 25 * G / t / PEAK))
    eng.close()
    # (b) a quarter of the groups beats in every call, with hb_commit and the beat list
    eng = engine(HB, True)
    hb = torch.zeros((P, eng.stride), dtype=torch.int64, device="cuda")
    beat = torch.zeros(G, dtype=torch.int64, device="cuda")
    t = median_call(lambda: eng.lead_clock(events, beat, G, None, 0, hb, sync=False), eng.sync, calls=40)
    model = (25 * 3 + 117) / 4.0
    lines.append("quarter_beats     %9.2f us   %.0f B/group  %.3f of 8 TB/s" % (t * 1e6, model, model * G / t / PEAK))
    # (c) the whole-shard pair the parent offers
    def pair():
        eng.quorum_recently_active()
        eng.heartbeat_commits(dev_out=hb.data_ptr())
    t = median_call(pair, eng.sync, calls=10)
    lines.append("whole_shard_pair  %9.2f us   (rg_quorum_recently_active + rg_heartbeat_commits, every tick)" % (t * 1e6))
    eng.close()
    text = "rgx_lead_clock, %d groups x %d slots, medians\n" % (G, P) + "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
