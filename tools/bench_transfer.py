#!/usr/bin/env python3
"""Time the batched leader transfer (rgm_transfer_leader*, include/raftgroups_transfer.h) against the road a host takes without it,
in ONE run on one MI355X.

    python tools/bench_transfer.py [--out profiles/transfer.txt] [--n 1000000]

Two sets of engines of n leader groups x 5, max_inflight 0 and 8, the leader's clock enabled (election_tick 10, heartbeat_tick 3).
Every group: five voters (own slot 0), a ten-entry log, every peer in Replicate, slots 1..3 caught up and slot 4 LAGGING (matched 5).
K of the groups, spread evenly over the shard, are named per call, K in {1, 1 000, 65 536}: the repetitions ALTERNATE between
starting a transfer to slot 4 (STARTED: the TRANSFEREE bits, election_elapsed = 0 and, with device Inflights, one
maybe_send_append -- the whole backlog in the first repetition, an empty append from then on, so that every timed repetition does
the same work) and clearing it again (the new calls: a request that names the leader itself, SELF, which aborts the transfer in
progress; the route: the word without the field). Timed with device events around the repetitions of a region (every form of the
host route synchronises; the dense form is asynchronous), the figure the median over at least five regions:
    route   what the parent commit can do: rg_read_groups of the K groups (the host does not own the cfg word), rg_set_config per
            group, rgx_lead_clock_write of the K cells. Those calls are unchanged by this extension, so this is the parent's
            behaviour measured in the same run on the same box. It sends nothing: on an engine with device Inflights the host would
            still owe the first append.
    sparse  rgm_transfer_leader (staged, synchronises, the answers come back to the host)
    dense   rgm_transfer_leader_device (asynchronous)
... and the claim "an unselected group costs its dev_to byte and its status byte": the dense form with NOTHING selected against
k_conf_dense (rgc_apply_conf_device) with nothing selected, alternating regions in the same run, with the spread of the regions.
Checked in the run: every status STARTED / SELF, and after a start and after a clearing the cfg words rg_read_groups reports for the
K groups are the same on the three roads. Every engine call raises on a non-zero status; nothing is retried.
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

FULL = 0x1F
TRANSFEREE_BITS = 0xF << 20


def make_engine(torch, rg, n, max_inflight):
    E = rg.engine
    eng = rg.Engine(n, 5, max_inflight=max_inflight)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    S = eng.stride
    host = {}
    for name, v in (("match", 10), ("next", 11), ("pr_commit", 10)):
        host[name] = np.full((5, S), v, dtype=np.uint64)
    host["match"][4, :], host["next"][4, :], host["pr_commit"][4, :] = 5, 6, 5
    for name, v in (("commit", 10), ("term_lo", 1), ("term_hi", 10), ("cur_term", 1), ("dummy_index", 0), ("dummy_term", 0)):
        host[name] = np.full(n, v, dtype=np.uint64)
    host["cfg"] = np.full(n, E.cfg_make(FULL, 0, 0), dtype=np.uint32)
    host["pflags"] = np.zeros((n, 8), dtype=np.uint8)
    host["pflags"][:, :5] = 1 | 8
    for name, a in host.items():
        eng.load_column(E.COL.NAMES.index(name), a)
    eng.lead_clock_enable(10, 3, E.LEAD_CLOCK_START_LED)
    return eng


def run(torch, rg, n, max_inflight):
    E = rg.engine
    engines = {name: make_engine(torch, rg, n, max_inflight) for name in ("route", "sparse", "dense")}
    status = torch.zeros(n, device="cuda", dtype=torch.uint8)
    count = torch.zeros(1, device="cuda", dtype=torch.int32) if max_inflight else None
    rows = []
    for K in sorted({1, min(1000, n), min(65536, n)}):
        groups = (np.arange(K, dtype=np.uint64) * np.uint64(n // K)).astype(np.uint64)
        items = torch.zeros(K * 32, device="cuda", dtype=torch.uint8) if max_inflight else None
        recs, d_to = [], []
        for slot in (4, 0):  # start a transfer to slot 4; name the leader itself: the transfer in progress is aborted
            r = np.zeros(K, dtype=E.TRANSFER_REC_DTYPE)
            r["group"], r["slot"] = groups, slot
            recs.append(r)
            to = np.zeros(n, dtype=np.uint8)
            to[groups] = slot + 1
            d_to.append(torch.from_numpy(to).cuda())
        cells = np.zeros(K, dtype=E.LEAD_CLOCK_CELL_DTYPE)
        cells["group"], cells["term"], cells["led"] = groups, 1, 1

        def dense(k):
            engines["dense"].transfer_leader_device(d_to[k & 1], status, items=items, item_cap=K if max_inflight else 0, count=count)

        def sparse(k):
            resp, got, total = engines["sparse"].transfer_leader(recs[k & 1], item_cap=K if max_inflight else None)
            assert (resp["status"] == (E.XFER_SELF if k & 1 else E.XFER_STARTED)).all()

        def route(k):
            eng = engines["route"]
            cur = eng.read_groups(groups)
            field = 0 if k & 1 else 5 << 20
            for g, old in zip(groups.tolist(), cur["cfg"].tolist()):
                eng.set_config(g, (old & ~TRANSFEREE_BITS) | field)
            eng.lead_clock_write(cells)

        row = {"K": K, "max_inflight": max_inflight}
        words_after = {}
        for name, fn, sync in (("route", route, True), ("sparse", sparse, True), ("dense", dense, False)):
            for k in (0, 1):  # one start, one clearing: warm-up and the comparison of the three roads
                fn(k)
                torch.cuda.synchronize()
                key = engines[name].read_groups(groups[:4096])["cfg"].tobytes()
                assert words_after.setdefault(k, key) == key, (K, name, k, "the roads leave different words")
            steps, regions = ((2, 5) if K >= 65536 else (10, 5)) if sync else (20, 7)
            t = [timed(torch, fn, steps) for _ in range(regions)]
            row[name] = [round(float(np.median(t)), 2), round(min(t), 2), round(max(t), 2)]
        assert int((status == E.XFER_SELF).sum()) == K and int((status == E.XFER_NONE).sum()) == n - K
        rows.append(row)
    # nothing selected: the transfer's dense kernel against the conf change's, alternating regions
    eng = engines["dense"]
    nothing = torch.zeros(n, device="cuda", dtype=torch.uint8)
    d_cfg = torch.zeros(n, device="cuda", dtype=torch.int32)
    forms = {"k_transfer_dense": lambda k: eng.transfer_leader_device(nothing, status, count=count),
             "k_conf_dense": lambda k: eng.apply_conf_device(nothing, d_cfg, status, count=count)}
    for fn in forms.values():
        timed(torch, fn, 20)
    t = {name: [] for name in forms}
    for _ in range(9):
        for name, fn in forms.items():
            t[name].append(timed(torch, fn, 50))
    idle = {name: [round(float(np.median(v)), 2), round(min(v), 2), round(max(v), 2)] for name, v in t.items()}
    for e in engines.values():
        e.close()
    return rows, idle


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transfer.txt"))
    ap.add_argument("--n", type=int, default=1_000_000)
    a = ap.parse_args()
    import torch
    import raft_rs_amd as rg
    if not torch.cuda.is_available():
        raise SystemExit("bench_transfer: no GPU (there is no CPU fallback and no CPU timing)")
    lines = [f"the batched leader transfer (rgm_transfer_leader*) against the host route, {a.n} leader groups x 5, K groups alternately starting a transfer to a lagging voter and "
             "having it cleared, one run; device events around the repetitions of a region, median (min max) over the regions, us per call; call time, launch overhead included",
             "route: rg_read_groups, rg_set_config per group, rgx_lead_clock_write (unchanged calls: the parent's behaviour, same run, same box; the route sends nothing)"]
    results = []
    f = lambda v: f"{v[0]:12.2f} ({v[1]:.2f} {v[2]:.2f})"  # noqa: E731
    for mi in (0, 8):
        rows, idle = run(torch, rg, a.n, mi)
        results.append({"max_inflight": mi, "rows": rows, "nothing_selected": idle})
        lines.append(f"max_inflight = {mi}")
        lines.append("K       | route us                     | sparse us                  | dense us                   | route/sparse | route/dense")
        for row in rows:
            h, s, d = row["route"], row["sparse"], row["dense"]
            lines.append(f"{row['K']:7d} | {f(h):28s} | {f(s):26s} | {f(d):26s} | {h[0] / s[0]:12.1f} | {h[0] / d[0]:11.1f}")
        x, c = idle["k_transfer_dense"], idle["k_conf_dense"]
        spread = max(x[2] - x[1], c[2] - c[1])
        lines.append(f"nothing selected, 9 alternating regions of 50 calls: k_transfer_dense {f(x).strip()} us, k_conf_dense {f(c).strip()} us; the medians differ by "
                     f"{abs(x[0] - c[0]):.2f} us, the regions of one kernel spread over {spread:.2f} us: "
                     + ("within the run-to-run spread" if abs(x[0] - c[0]) <= spread else "MORE than the run-to-run spread"))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
    print(json.dumps({"bench": "transfer", "n": a.n, "results": results}))


if __name__ == "__main__":
    main()
