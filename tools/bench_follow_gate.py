#!/usr/bin/env python3
"""Time the gated dense follower step and the election clock next to the ungated step, in ONE run on one MI355X.

    python tools/bench_follow_gate.py [--out profiles/follow_gate.txt] [--sizes 1000000 8000000]

Two engines get the SAME seeded steady stream (tools/bench_follow.py's: every group a 1..8-entry append on its tail, 1 % rejects,
1/32 term changes per step): one through rg_follow_step_device (k_follow_dense), one through rg_follow_step_gated_device
(k_follow_gate_dense) with Message.term = 1 and Message.from = 2 for every group -- after the first step the steady case of the
gate: an equal term and the leader the group already has. Per size and region the tool times, with device events around STEPS
launches each, in this order:
    1. the ungated step
    2. the gated step (election_elapsed is 0 after the first step of the region: the clock cell is read, not written)
    3. rg_follow_clock with nothing due (no group promotable)                       [after the step regions]
    4. rg_follow_clock with a fixed 1/32 of the groups due on every call (election_tick 1: a promotable group fires every tick)
    5. rg_follow_clock + the gated step, alternating (every step now writes the clock cell the tick before it moved)
The figure is the median over REGIONS regions, per launch (5: per pair). Every ratio is formed from times of this one run.
Both engines are checked against the stream's mirror (statuses of every warm-up step, last_index at the end), the gated one also
for gate == PASS and the term / leader cells.

Bytes per group with a message, counted from the kernels:
    ungated step   110 (tools/bench_follow.py)
    gated step     110 + term 8 + from 8 (columns) + term 8 + lead 8 + clock 4 (cells read) + gate 1 + events 1 + resp_term 8
                   (written) = 156; + 4 where the clock cell is written (case 5)
    clock          clock cell 4 read + 4 written = 8; a due group adds 8 (its place in the list) and one atomic per wave
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_follow import Stream  # noqa: E402

STEPS, REGIONS, WARM_REGIONS = 20, 5, 1
BYTES = {"ungated": 110, "gated": 156, "clock": 8}


def timed(torch, fn, count):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for k in range(count):
        fn(k)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / count


def run_size(torch, rg, n, seed):
    E = rg.engine
    stream = torch.cuda.current_stream().cuda_stream
    plain, gated = rg.Engine(1024, 3), rg.Engine(1024, 3)
    for eng in (plain, gated):
        eng.follow_enable(n)
        eng.set_stream(stream)
    gated.follow_gate_enable(1, seed=seed)
    F = plain.follow_stride()
    st = Stream(torch, n, F, seed)

    def outs():
        o = {k: torch.zeros(F, device="cuda", dtype=torch.int64) for k in ("index", "commit", "conflict", "reject_hint", "log_term")}
        o["status"] = torch.zeros(F, device="cuda", dtype=torch.uint8)
        return o
    out_p, out_g = outs(), outs()
    gate, events = torch.zeros(F, device="cuda", dtype=torch.uint8), torch.zeros(F, device="cuda", dtype=torch.uint8)
    resp_term = torch.zeros(F, device="cuda", dtype=torch.int64)
    m_term, m_from = torch.ones(F, device="cuda", dtype=torch.int64), torch.full((F,), 2, device="cuda", dtype=torch.int64)
    hup = torch.zeros(n // 32 + 64, device="cuda", dtype=torch.int64)

    def step_p(cols):
        plain.follow_step_device(cols, out_p)

    def step_g(cols):
        gated.follow_step_gated_device(cols, m_term, m_from, out_g, gate, events, resp_term)

    t = {"ungated": [], "gated": [], "clock_idle": [], "clock_due": [], "pair": []}
    last_steps = None
    for region in range(WARM_REGIONS + REGIONS):
        steps = [st.next() for _ in range(STEPS)]
        torch.cuda.synchronize()
        if region < WARM_REGIONS:  # (the warm-up region also checks every step, which a timed region cannot)
            for cols, want in steps:
                step_p(cols)
                step_g(cols)
                torch.cuda.synchronize()
                assert bool((out_p["status"][:n] == want[:n]).all()) and bool((out_g["status"][:n] == want[:n]).all()), "engine and mirror disagree"
                assert bool((gate[:n] == E.GATE_PASS).all()) and bool((resp_term[:n] == 1).all())
            continue
        t["ungated"].append(timed(torch, lambda k: step_p(steps[k][0]), STEPS))
        t["gated"].append(timed(torch, lambda k: step_g(steps[k][0]), STEPS))
        assert bool((out_g["status"][:n] == steps[-1][1][:n]).all()) and bool((out_p["status"][:n] == steps[-1][1][:n]).all())
        assert bool((gate[:n] == E.GATE_PASS).all())
        last_steps = steps
    sample = np.arange(0, n, max(1, n // 4096), dtype=np.uint64)
    mirror = st.last.cpu().numpy()[::max(1, n // 4096)][:len(sample)]
    for eng in (plain, gated):
        state = eng.follow_read(sample)
        assert (state["last_index"].astype(np.int64) == mirror).all()
    soft = gated.follow_soft_read(sample)
    assert (soft["term"] == 1).all() and (soft["leader_id"] == 2).all() and (soft["election_elapsed"] == 0).all()

    for _ in range(REGIONS):  # nothing due: no group is promotable
        t["clock_idle"].append(timed(torch, lambda k: gated.follow_clock(hup, len(hup), sync=False), STEPS))
    assert gated.follow_clock(hup, len(hup)) == 0
    due = np.arange(0, n, 32, dtype=np.uint64)
    w = gated.follow_soft_read(due)
    w["promotable"] = 1
    gated.follow_soft_write(w)
    for _ in range(REGIONS):  # timeouts are 1: every promotable group fires on every call
        t["clock_due"].append(timed(torch, lambda k: gated.follow_clock(hup, len(hup), sync=False), STEPS))
    assert gated.follow_clock(hup, len(hup)) == len(due)
    # the pair: the tick moves every clock cell, the step that follows writes it back to 0 (the same records again: STALE or a
    # repeat ACCEPT, the same bytes but for last_index / committed, which a repeat does not move)
    for _ in range(REGIONS):
        def pair(k):
            gated.follow_clock(hup, len(hup), sync=False)
            step_g(last_steps[k][0])
        t["pair"].append(timed(torch, pair, STEPS))
    plain.close()
    gated.close()
    med = {k: float(np.median(v)) for k, v in t.items()}
    row = {"n_follow": n, "stride": int(F), "regions": REGIONS, "launches_per_region": STEPS}
    for k, v in t.items():
        row["us_" + k] = [round(med[k], 2), round(min(v), 2), round(max(v), 2)]
    row["gated_over_ungated"] = round(med["gated"] / med["ungated"], 3)
    row["byte_ratio"] = round(BYTES["gated"] / BYTES["ungated"], 3)
    row["pair_minus_clock_over_ungated"] = round((med["pair"] - med["clock_idle"]) / med["ungated"], 3)
    row["gb_per_s"] = {"ungated": round(BYTES["ungated"] * n / med["ungated"] / 1e3, 1), "gated": round(BYTES["gated"] * n / med["gated"] / 1e3, 1),
                       "clock_idle": round(BYTES["clock"] * n / med["clock_idle"] / 1e3, 1)}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "follow_gate.txt"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 8_000_000])
    ap.add_argument("--seed", type=int, default=5)
    a = ap.parse_args()
    import torch
    import raft_rs_amd as rg
    if not torch.cuda.is_available():
        raise SystemExit("bench_follow_gate: no GPU (there is no CPU fallback and no CPU timing)")
    rows = [run_size(torch, rg, n, a.seed) for n in a.sizes]
    lines = [f"gated dense follower step (rg_follow_step_gated_device) and election clock (rg_follow_clock) next to the ungated step "
             f"(rg_follow_step_device), one run, the same steady stream; device events around {STEPS} launches, median (min max) of {REGIONS} regions",
             f"model bytes/group: ungated {BYTES['ungated']}, gated {BYTES['gated']} (+4 where the clock cell is written), clock {BYTES['clock']}; "
             f"byte ratio gated/ungated {BYTES['gated'] / BYTES['ungated']:.3f}",
             "n_follow | us/launch ungated | gated | clock, nothing due | clock, 1/32 due | clock + gated step (pair) | gated/ungated | "
             "(pair - idle clock)/ungated | model GB/s ungated, gated, clock"]
    for r in rows:
        f3 = lambda v: f"{v[0]:8.2f} ({v[1]:.2f} {v[2]:.2f})"  # noqa: E731
        lines.append(f"{r['n_follow']:9d} | {f3(r['us_ungated'])} | {f3(r['us_gated'])} | {f3(r['us_clock_idle'])} | {f3(r['us_clock_due'])} | "
                     f"{f3(r['us_pair'])} | {r['gated_over_ungated']:.3f} | {r['pair_minus_clock_over_ungated']:.3f} | "
                     f"{r['gb_per_s']['ungated']:.1f} {r['gb_per_s']['gated']:.1f} {r['gb_per_s']['clock_idle']:.1f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(json.dumps({"bench": "follow_gate", "results": rows}))


if __name__ == "__main__":
    main()
