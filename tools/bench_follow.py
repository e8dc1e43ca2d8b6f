#!/usr/bin/env python3
"""Time the dense follower step (rg_follow_step_device, k_follow_dense) on one MI355X at n_follow = 1 M and 8 M.

    python tools/bench_follow.py [--out profiles/follow_step.txt] [--sizes 1000000 8000000]

The stream is seeded and generated on the device, a region of steps ahead of the timed window: in every step EVERY group gets
a MsgAppend of 1..8 single-term entries on its tail with commit = its last index; 1 % of the groups send a log_term that does
not match (a reject, nothing changes); a rotating 1/32 of the groups open a new term with their entries (the old tail is filed
as an older run; after 8 of those a group's table is full and every further one drops its oldest run). The generator keeps the
mirror (last index, tail term) the next step's records are built from, and the tool checks the engine against that mirror: the
status column of every step (ACCEPT / REJECT where expected) and, after the last step, last_index of every group.

Timing: device events around a region of STEPS launches on the engine's stream, after one warm-up region; the figure is the
median over REGIONS regions, per step. The time is a call time (launch overhead included), not a kernel time.

Bytes of the steady step per group with a message, counted from k_follow_dense / rg_follow_append (no ext column is passed):
    record columns read   flags 1 + index 8 + log_term 8 + commit 8 + ent_term 8 + n_entries 4              = 37
    hot state read        committed 8 + last 8 + tail_first 8 + tail_term 8                                 = 32
    hot state written     last 8 + committed 8                                                              = 16
    response written      status 1 + index 8 + commit 8 + conflict 8                                        = 25
                                                                                                       total 110
A term change adds the cold cells (run count read and written, one run filed: 18 B; 7 runs moved down once the table is full:
+ 224 B) and a reject writes reject_hint and log_term instead of the state (+ 16 - 16).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS, REGIONS, WARM_REGIONS = 20, 5, 1
BYTES_STEADY = 110


class Stream:
    """The seeded stream and its mirror, on the device."""

    def __init__(self, torch, n, stride, seed):
        self.torch, self.n, self.F = torch, n, stride
        self.gen = torch.Generator(device="cuda")
        self.gen.manual_seed(seed)
        self.g = torch.arange(stride, device="cuda", dtype=torch.int64)
        self.last = torch.zeros(stride, device="cuda", dtype=torch.int64)
        self.term = torch.zeros(stride, device="cuda", dtype=torch.int64)
        self.step_no = 0

    def next(self):
        """The columns of one step (rg_follow_msgs) and the statuses it must produce; advances the mirror."""
        torch, F = self.torch, self.F
        n_entries = torch.randint(1, 9, (F,), generator=self.gen, device="cuda", dtype=torch.int32)
        reject = torch.rand(F, generator=self.gen, device="cuda") < 0.01
        change = (((self.g + self.step_no) % 32) == 0) | (self.term == 0)  # (an empty log's first entries open term 1)
        cols = {"flags": torch.ones(F, device="cuda", dtype=torch.uint8), "index": self.last.clone(), "log_term": self.term + reject.to(torch.int64),
                "commit": self.last.clone(), "ent_term": self.term + change.to(torch.int64), "n_entries": n_entries}
        ok = ~reject
        self.last = self.last + n_entries.to(torch.int64) * ok
        self.term = self.term + (change & ok).to(torch.int64)
        self.step_no += 1
        return cols, torch.where(reject, 2, 1).to(torch.uint8)  # RG_FOLLOW_REJECT / RG_FOLLOW_ACCEPT


def run_size(torch, rg, n, seed):
    eng = rg.Engine(1024, 3)
    eng.follow_enable(n)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    F = eng.follow_stride()
    st = Stream(torch, n, F, seed)
    out = {k: torch.zeros(F, device="cuda", dtype=torch.int64) for k in ("index", "commit", "conflict", "reject_hint", "log_term")}
    out["status"] = torch.zeros(F, device="cuda", dtype=torch.uint8)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for region in range(WARM_REGIONS + REGIONS):
        steps = [st.next() for _ in range(STEPS)]
        torch.cuda.synchronize()
        if region < WARM_REGIONS:  # (the warm-up region also checks every step's statuses, which a timed region cannot)
            for cols, want in steps:
                eng.follow_step_device(cols, out)
                torch.cuda.synchronize()
                assert bool((out["status"][:n] == want[:n]).all()), "the engine and the stream's mirror disagree"
            continue
        e0.record()
        for cols, _ in steps:
            eng.follow_step_device(cols, out)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / STEPS)
        assert bool((out["status"][:n] == steps[-1][1][:n]).all()), "the engine and the stream's mirror disagree"
    state = eng.follow_read(np.arange(0, n, max(1, n // 4096), dtype=np.uint64))
    mirror = st.last.cpu().numpy()[::max(1, n // 4096)][:len(state)]
    assert (state["last_index"].astype(np.int64) == mirror).all() and (state["committed"] <= state["last_index"]).all()
    runs = np.bincount(state["n_runs"], minlength=10)
    eng.close()
    med = float(np.median(times))
    return {"n_follow": n, "stride": int(F), "us_per_step_median": round(med, 2), "us_per_step_min": round(min(times), 2),
            "us_per_step_max": round(max(times), 2), "regions": REGIONS, "steps_per_region": STEPS,
            "model_bytes_per_group": BYTES_STEADY, "model_gb_per_s_at_median": round(BYTES_STEADY * n / med / 1e3, 1),
            "groups_per_s_at_median": round(n / med * 1e6), "runs_per_group_sampled_max": int(np.flatnonzero(runs)[-1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "follow_step.txt"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 8_000_000])
    ap.add_argument("--seed", type=int, default=5)
    a = ap.parse_args()
    import torch
    import raft_rs_amd as rg
    if not torch.cuda.is_available():
        raise SystemExit("bench_follow: no GPU (there is no CPU fallback and no CPU timing)")
    rows = [run_size(torch, rg, n, a.seed) for n in a.sizes]
    lines = [f"dense follower step (rg_follow_step_device), every group a 1..8-entry append on its tail, 1 % rejects, 1/32 term changes per step; "
             f"device events around {STEPS} launches, median of {REGIONS} regions after {WARM_REGIONS} warm-up region(s)",
             "n_follow | us/step: median  min  max | model bytes/group | model GB/s at the median | groups/s"]
    for r in rows:
        lines.append(f"{r['n_follow']:9d} | {r['us_per_step_median']:9.2f} {r['us_per_step_min']:9.2f} {r['us_per_step_max']:9.2f} | "
                     f"{r['model_bytes_per_group']:4d} | {r['model_gb_per_s_at_median']:8.1f} | {r['groups_per_s_at_median']:.3e}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(json.dumps({"bench": "follow_step_device", "results": rows}))


if __name__ == "__main__":
    main()
