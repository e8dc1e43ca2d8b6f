#!/usr/bin/env python3
"""Time the election storm and a dense vote-response round on the follower arena, in ONE run on one MI355X.

    python tools/bench_follow_elect.py [--out profiles/follow_elect.txt] [--n 1000000]

One engine, n followed groups, every group a five-voter configuration (own slot 0), a ten-entry log of one term with commit 8
(last_term and commit_info are answered from the tail: the hot cells), election_tick 1 -- every timeout is 1, so a promotable
group is due on every rg_follow_clock; no pre-vote, so every MsgHup is a whole become_candidate with its vote requests. Timed
with device events around STEPS repetitions each, in this order, the figure the median over REGIONS regions:
    0. rg_follow_clock with nothing due
    1. a fixed 1/32 of the groups promotable (due every time): rg_follow_clock alone; rg_follow_campaign_device alone, on the list
       and the count word the last clock left (the same groups campaign again: a candidate's MsgHup); the two chained on the
       stream -- the storm path
    2. the same three with every group promotable
    3. rg_follow_vote_resps_device: one MsgRequestVoteResponse per group at the group's term, a denial from slot 1 -- the election
       stays open (the first round records it, every later one finds the slot's vote there)
Checked in the run: the number due, every campaign's result (REQUESTS), request term (= the group's new term) and targets; every
response's result (PENDING), and on a sample the role, term and vote cells.

Bytes per group with a record, counted from the kernels ("The candidate half"):
    campaign   list entry 8 + log cells 32 + term, lead, clock 20 + role 1 + self_id, conf, votes 14 read = 75;
               term, clock, vote, role, votes 23 written; result, events, status, term 11 + the request columns 43 written = 152;
               (+ 8 where the group had a leader, + 1 with a dev_block column); the clock beside it: 8 per group of the ARENA + 8 per due group
    response   kind, slot, reject, term, commit, commit_term 27 + log cells 32 + term, lead, clock 20 + role 1 + election cells 14
               read = 94; votes 2 (the first round only) + result, events, status, term 11 written = 105 (107)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_follow_gate import timed  # noqa: E402

STEPS, REGIONS = 20, 5
BYTES = {"clock": 8, "due": 8, "campaign": 152, "response": 105}
HBM_PEAK = 8e12  # bytes/s: the fraction below is model bytes / time / this
CHUNK = 1 << 17


def run(torch, rg, n, seed):
    E = rg.engine
    eng = rg.Engine(1024, 3)
    eng.follow_enable(n)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    eng.follow_gate_enable(1, seed=seed)
    eng.follow_elect_enable()
    F = eng.follow_stride()
    for a in range(0, n, CHUNK):
        g = np.arange(a, min(n, a + CHUNK), dtype=np.uint64)
        st = np.zeros(len(g), dtype=E.FOLLOW_STATE_DTYPE)
        st["group"], st["committed"], st["last_index"], st["n_runs"] = g, 8, 10, 1
        st["run_first"][:, 0] = 1
        st["run_term"][:, 0] = 1
        eng.follow_write(st)
        ce = np.zeros(len(g), dtype=E.FOLLOW_ELECT_DTYPE)
        ce["group"], ce["self_id"], ce["conf"] = g, g + 1, E.elect_conf_make(0x1f, 0, 0)
        eng.follow_elect_write(ce)

    def promote(groups):
        for a in range(0, len(groups), CHUNK):
            w = eng.follow_soft_read(groups[a:a + CHUNK])
            w["promotable"], w["term"] = 1, 1
            eng.follow_soft_write(w)
    hup = torch.zeros(n + 64, device="cuda", dtype=torch.int64)
    out = {k: torch.zeros(n + 64, device="cuda", dtype=torch.uint8) for k in E.ELECT_OUT_COLUMNS[:6]}
    out.update({k: torch.zeros(n + 64, device="cuda", dtype=torch.int64) for k in E.ELECT_OUT_COLUMNS[6:]})
    counts = eng.follow_clock_counts()

    def storm(k):
        eng.follow_clock(hup, n + 64, sync=False)
        eng.follow_campaign_device(hup, counts, n + 64, out)

    def check_storm(due):
        assert eng.follow_clock(hup, n + 64) == due  # (one more tick, synchronous: the count)
        eng.follow_campaign_device(hup, counts, n + 64, out)
        torch.cuda.synchronize()
        assert bool((out["result"][:due] == E.ELECT_REQUESTS).all()) and bool((out["req_kind"][:due] == E.FOLLOW_MSG_VOTE).all())
        assert bool((out["targets"][:due] == 0x1e).all()) and bool((out["status"][:due] == 0).all())
        assert bool((out["req_term"][:due] == out["term"][:due]).all()) and bool((out["req_index"][:due] == 10).all())
        assert bool((out["req_commit"][:due] == 8).all()) and bool((out["req_commit_term"][:due] == 1).all())
    def clock_only(k):
        eng.follow_clock(hup, n + 64, sync=False)

    def campaign_only(k):  # the list and the count word the last clock left: the same groups campaign again (a candidate's MsgHup)
        eng.follow_campaign_device(hup, counts, n + 64, out)
    t = {k: [] for k in ("clock_idle", "clock_32", "campaign_32", "storm_32", "clock_all", "campaign_all", "storm_all", "responses")}
    for _ in range(REGIONS):  # nothing due: what the clock alone costs in this run
        t["clock_idle"].append(timed(torch, clock_only, STEPS))
    some = np.arange(0, n, 32, dtype=np.uint64)
    promote(some)
    for tag, due in (("32", len(some)), ("all", n)):
        if tag == "all":
            promote(np.setdiff1d(np.arange(n, dtype=np.uint64), some))
        storm(0)  # (warm-up)
        for _ in range(REGIONS):  # the pair's two halves on their own, then the pair
            t["clock_" + tag].append(timed(torch, clock_only, STEPS))
            t["campaign_" + tag].append(timed(torch, campaign_only, STEPS))
            t["storm_" + tag].append(timed(torch, storm, STEPS))
        check_storm(due)
    # the response round: every group is a Candidate now; its term from the cells
    term = np.zeros(F, dtype=np.uint64)
    for a in range(0, n, CHUNK):
        w = eng.follow_soft_read(np.arange(a, min(n, a + CHUNK), dtype=np.uint64))
        assert (w["role"] == E.ROLE_CANDIDATE).all() and (w["vote"] == w["group"] + 1).all() and (w["leader_id"] == 0).all()
        term[a:a + len(w)] = w["term"]
    msgs = {"kind": torch.full((F,), E.FOLLOW_MSG_VOTE, device="cuda", dtype=torch.uint8), "slot": torch.ones(F, device="cuda", dtype=torch.uint8),
            "reject": torch.ones(F, device="cuda", dtype=torch.uint8), "term": torch.from_numpy(term.view(np.int64)).cuda(),
            "commit": torch.zeros(F, device="cuda", dtype=torch.int64), "commit_term": torch.zeros(F, device="cuda", dtype=torch.int64)}
    dout = {k: torch.zeros(F, device="cuda", dtype=v.dtype) for k, v in out.items()}
    eng.follow_vote_resps_device(msgs, dout)  # (the round that records the votes)
    for _ in range(REGIONS):
        t["responses"].append(timed(torch, lambda k: eng.follow_vote_resps_device(msgs, dout), STEPS))
    assert bool((dout["result"][:n] == E.ELECT_PENDING).all()) and bool((dout["status"][:n] == 0).all()) and bool((dout["events"][:n] == 0).all())
    cells = eng.follow_elect_read(np.arange(0, n, max(1, n // 4096), dtype=np.uint64))
    assert (cells["yes"] == 1).all() and (cells["no"] == 2).all()
    eng.close()
    med = {k: float(np.median(v)) for k, v in t.items()}
    row = {"n_follow": n, "stride": int(F), "regions": REGIONS, "repetitions_per_region": STEPS}
    for k, v in t.items():
        row["us_" + k] = [round(med[k], 2), round(min(v), 2), round(max(v), 2)]
    model = {"clock_idle": BYTES["clock"] * n, "responses": BYTES["response"] * n}
    for tag, due in (("32", len(some)), ("all", n)):
        model["clock_" + tag] = BYTES["clock"] * n + BYTES["due"] * due
        model["campaign_" + tag] = BYTES["campaign"] * due
        model["storm_" + tag] = model["clock_" + tag] + model["campaign_" + tag]
    row["model_bytes"] = model
    row["gb_per_s"] = {k: round(model[k] / med[k] / 1e3, 1) for k in model}
    row["frac_of_hbm_peak"] = {k: round(model[k] / (med[k] * 1e-6) / HBM_PEAK, 3) for k in model}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "follow_elect.txt"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=5)
    a = ap.parse_args()
    import torch
    import raft_rs_amd as rg
    if not torch.cuda.is_available():
        raise SystemExit("bench_follow_elect: no GPU (there is no CPU fallback and no CPU timing)")
    r = run(torch, rg, a.n, a.seed)
    names = {"clock_idle": "clock, nothing due", "clock_32": "clock alone, 1/32 due", "campaign_32": "campaign alone, 1/32 of the groups",
             "storm_32": "clock + campaign, 1/32 due", "clock_all": "clock alone, all due", "campaign_all": "campaign alone, all groups",
             "storm_all": "clock + campaign, all due", "responses": "dense response round"}
    lines = [f"election storm (rg_follow_clock + rg_follow_campaign_device chained) and a dense vote-response round (rg_follow_vote_resps_device), "
             f"{r['n_follow']} followed groups, one run; device events around {STEPS} repetitions, median (min max) of {REGIONS} regions; call time, launch overhead included",
             f"model bytes: clock {BYTES['clock']}/group + {BYTES['due']}/due group, campaign {BYTES['campaign']}/due group, response {BYTES['response']}/group; "
             f"fraction = model bytes / time / {HBM_PEAK / 1e12:.0f} TB/s (the arena is Infinity-Cache-assisted at this size)",
             "case | us | model MB | model GB/s | fraction of the HBM peak"]
    for k in names:
        v = r["us_" + k]
        lines.append(f"{names[k]:34s} | {v[0]:8.2f} ({v[1]:.2f} {v[2]:.2f}) | {r['model_bytes'][k] / 1e6:7.1f} | {r['gb_per_s'][k]:7.1f} | {r['frac_of_hbm_peak'][k]:.3f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(json.dumps({"bench": "follow_elect", "results": [r]}))


if __name__ == "__main__":
    main()
