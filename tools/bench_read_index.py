#!/usr/bin/env python3
"""Time the dense ReadIndex ack pass (rg_read_acks_device, k_read_acks_dense) on one MI355X: 1 M groups x 5 slots with 0 %, 10 %
and 100 % of the groups holding one pending read, next to k_quorum_active (rg_quorum_recently_active) at the same size in the
same process -- the engine's other per-group quorum bitmask sweep, the yardstick for the pass over empty queues.

    python tools/bench_read_index.py [--out profiles/read_index.txt]
    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/bench_read_index.py --out ...   # (kernel times)
    python tools/bench_read_index.py --trace DIR --out profiles/read_index.txt                              # append them

Device events around each launch give the call time (launch overhead included: what a host loop sees); the kernel trace of a
separate profiled run gives the kernel time. Every timed pass starts from the same queues (rg_restore between passes, outside
the timed window) and the list of read states is drained after each.

Bytes a pass moves per group (the model next to the timings):
    empty queue          4 (the queue word) -- nothing else is read
    one pending read     4 queue word + 5 x 8 ctx cells + 8 queue term + 8 RG_COL_CUR_TERM + 4 RG_COL_CFG + 8 queued ctx + 1 + 1 acks
                         byte (read, written) per ack until the quorum (2 acks at 3 of 5) + 4 queue word written
                         + 16 (ctx, index read back) + 24 (the read state written)  ~= 120
    k_quorum_active      4 RG_COL_CFG + 8 flag row read, 8 flag row + 1 result written = 21 (the flag row is written back whole)
"""
import argparse
import csv
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

G, P, WARM, K = 1_000_000, 5, 5, 40
FRACTIONS = (0.0, 0.1, 1.0)
BYTES_EMPTY, BYTES_ONE, BYTES_QA = 4, 120, 21


def run(out_path):
    import torch
    import raft_rs_amd as rg
    eng = rg.Engine(G, P)
    eng.workload_init(rg.WL_MAJORITY)
    eng.load_column(rg.COL.TERM_LO, np.zeros(G, dtype=np.uint64))  # every leader has committed in its term: no request is dropped
    eng.read_index_enable(2)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(3)
    lines = [f"dense ReadIndex ack pass, {G} groups x {P} slots, depth 2; device events around each of {K} launches (after {WARM} warm-up)",
             "fraction of groups with one pending read | call us: median  min  max | states per pass | model bytes/group | model GB/s at the median"]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    pending = np.zeros(G, dtype=bool)
    for frac in FRACTIONS:
        want = int(G * frac)
        add = rng.permutation(np.flatnonzero(~pending))[:want - int(pending.sum())]
        if len(add):
            reqs = np.zeros(len(add), dtype=rg.engine.READ_REQ_DTYPE)
            reqs["group"] = add
            reqs["ctx"] = add.astype(np.uint64) + np.uint64(1)
            st = eng.read_index(reqs)
            assert (st == rg.engine.READ_QUEUED).all(), np.bincount(st)
            pending[add] = True
        # every peer answers the heartbeat with the group's last pending ctx (0 where nothing is pending)
        last = eng.read_last_pending()
        assert int((last != 0).sum()) == want
        cols = np.zeros((P, eng.stride), dtype=np.uint64)
        cols[:, :G] = last
        d = torch.from_numpy(cols.view(np.int64)).cuda()
        eng.checkpoint()
        ts, n_states = [], 0
        for it in range(WARM + K):
            eng.restore()
            eng.quorum_recently_active()  # (the yardstick kernel, alternating with the pass: its time comes from the kernel trace)
            torch.cuda.synchronize()
            e0.record()
            eng.read_acks_device(d.data_ptr())
            e1.record()
            torch.cuda.synchronize()
            _, n_states = eng.read_states(cap=1)  # drains everything
            assert n_states == want, (n_states, want)
            if it >= WARM:
                ts.append(e0.elapsed_time(e1) * 1e3)
        eng.restore()  # (the next fraction builds on these queues)
        med = float(np.median(ts))
        model = BYTES_EMPTY * (1 - frac) + BYTES_ONE * frac
        lines.append(f"{frac*100:5.0f} % | {med:8.1f} {min(ts):8.1f} {max(ts):8.1f} | {n_states:8d} | {model:6.1f} | {model*G/med/1e3:8.1f}")
    eng.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


def trace(trace_dir, out_path):
    """Kernel times of the profiled run: the launches of k_read_acks_dense come in the order the fractions were timed."""
    path = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    dense = [dur(r) for r in rows if "k_read_acks_dense" in r["Kernel_Name"]]
    qa = [dur(r) for r in rows if "k_quorum_active" in r["Kernel_Name"]]
    per = WARM + K
    assert len(dense) == per * len(FRACTIONS) and len(qa) == len(dense), (len(dense), len(qa))
    lines = ["", f"kernel time, rocprofv3 --kernel-trace of a separate run of this tool (the {K} timed launches of each fraction; us: median  min  max)"]
    med = {}
    for k, frac in enumerate(FRACTIONS):
        a, b = dense[k * per + WARM:(k + 1) * per], qa[k * per + WARM:(k + 1) * per]
        med[frac] = (float(np.median(a)), float(np.median(b)))
        lines.append(f"{frac*100:5.0f} % | k_read_acks_dense<{P}> {np.median(a):7.2f} {min(a):7.2f} {max(a):7.2f} | k_quorum_active (same process, alternating) "
                     f"{np.median(b):7.2f} {min(b):7.2f} {max(b):7.2f}")
    d0, q0 = med[0.0]
    lines.append(f"empty queues against the yardstick: k_read_acks_dense {d0:.2f} us ({BYTES_EMPTY} B/group) vs k_quorum_active {q0:.2f} us ({BYTES_QA} B/group): "
                 + ("not slower" if d0 <= q0 else "SLOWER"))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(out_path, "a") as f:
        f.write(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "read_index.txt"))
    ap.add_argument("--trace", help="directory of a rocprofv3 --kernel-trace run of this tool: append the kernel times to --out")
    a = ap.parse_args()
    if a.trace:
        trace(a.trace, a.out)
    else:
        run(a.out)
