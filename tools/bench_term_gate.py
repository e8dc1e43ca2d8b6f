"""Time rgt_lead_gate_device at 1 M groups x 5 slots, with rgx_lead_clock's figure from the same run beside it as the scale.

    python tools/bench_term_gate.py [--groups N] [--out profiles/term_gate.txt]

Cases: (a) a steady stream -- every group led, a record of the group's own term in every slot, nothing dropped; (b) the same stream
with 1/32 of the groups deposed by one record of a higher term. (a) is an asynchronous call, timed in batches between two
synchronisations, like bench_lead_clock.py's cases; a deposition changes the state the next call meets (the group is stopped), so (b)
is timed ONE call at a time, between a re-arming rgx_lead_clock_write and a synchronisation, and (a) is repeated that way so that the
two compare: the single-call figures carry the launch and the synchronisation (an upper bound of the kernel's time). Medians of WHOLE
calls issued from Python (a 24-byte memset and a launch each). The output rows go to a column of their own, so the input stream is the
same in every call. Byte model: a steady group reads 8 B of flags, 8 + 8 + 4 B of term, tag and clock cell and
8 B per record, and writes 8 + 1 B -- 77 B at 5 records; a deposed group 4 B of cfg, 4 B of clock cell and 8 B of new_term more."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8e12  # B/s, the MI355X's HBM
STEADY_B, DEPOSED_B = 8 + 20 + 8 * 5 + 9, 8 + 20 + 8 * 5 + 9 + 4 + 4 + 8


def median_batched(fn, sync, calls=50, repeats=15):
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


def median_single(prepare, fn, sync, repeats=25):
    ts = []
    for _ in range(repeats):
        prepare()
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    import torch
    import raft_rs_amd as rg
    E = rg.engine
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    G, P = a.groups, 5
    eng = rg.Engine(G, P, device=0)
    eng.workload_init(rg.WL_MAJORITY)
    eng.lead_clock_enable(16383, 16382, 0x1 | E.LEAD_CLOCK_START_LED)  # between timeouts for every call of this run
    cur = eng.read_column(E.COL.CUR_TERM).astype(np.uint64)
    flags = np.zeros((G, 8), np.uint8)
    flags[:, :P] = 0x01  # RG_MF_VALID
    terms = np.zeros((P, eng.stride), np.uint64)
    terms[:, :G] = cur[:G]
    deposing = terms.copy()
    deposing[1, 0:G:32] += 1
    n_deposed = len(range(0, G, 32))
    led = np.zeros(G, dtype=E.LEAD_CLOCK_CELL_DTYPE)
    led["group"], led["term"], led["led"] = np.arange(G), cur[:G], 1

    def dev(x):
        return torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).cuda()
    d_flags, d_out, d_terms, d_deposing = dev(flags.reshape(-1)), torch.zeros(G * 8, dtype=torch.uint8, device="cuda"), dev(terms), dev(deposing)
    events = torch.zeros(eng.stride, dtype=torch.uint8, device="cuda")
    new_term = torch.zeros(eng.stride, dtype=torch.int64, device="cuda")
    clock_events = torch.zeros(eng.stride, dtype=torch.uint8, device="cuda")

    def gate(t):
        return eng.lead_gate_device(d_flags, t, events, new_term, d_out, sync=False)
    assert eng.lead_gate_device(d_flags, d_terms, events, new_term, d_out) == (0, 0, 0)
    lines = []
    t = median_batched(lambda: gate(d_terms), eng.sync)
    lines.append("gate_steady_batched     %9.2f us   %d B/group  %.3f of 8 TB/s" % (t * 1e6, STEADY_B, STEADY_B * G / t / PEAK))
    t = median_batched(lambda: eng.lead_clock(clock_events, sync=False), eng.sync)
    lines.append("lead_clock_batched      %9.2f us   25 B/group  %.3f of 8 TB/s   (k_lead_clock between timeouts: the scale)" % (t * 1e6, 25 * G / t / PEAK))
    t = median_single(lambda: eng.lead_clock_write(led), lambda: gate(d_terms), eng.sync)
    lines.append("gate_steady_single      %9.2f us   %d B/group  %.3f of 8 TB/s   (one call, launch and synchronisation included)" % (t * 1e6, STEADY_B, STEADY_B * G / t / PEAK))
    model = ((32 - 1) * STEADY_B + DEPOSED_B) / 32.0
    t = median_single(lambda: eng.lead_clock_write(led), lambda: gate(d_deposing), eng.sync)
    lines.append("gate_1_in_32_deposed    %9.2f us   %.1f B/group  %.3f of 8 TB/s   (one call, launch and synchronisation included)" % (t * 1e6, model, model * G / t / PEAK))
    eng.lead_clock_write(led)
    assert eng.lead_gate_device(d_flags, d_deposing, events, new_term, d_out) == (n_deposed, 0, 0)
    eng.close()
    text = "rgt_lead_gate_device, %d groups x %d slots, medians\n" % (G, P) + "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
