#!/usr/bin/env python3
"""Time the batched conf change (rgc_apply_conf*, include/raftgroups_conf.h) against the road a host takes without it, in ONE run on
one MI355X.

    python tools/bench_conf_change.py [--out profiles/conf_change.txt] [--n 1000000]

Two engines of n leader groups x 5, max_inflight 0 and 8. Every group: five voters (own slot 0), a ten-entry log, every peer caught
up and in Replicate, so a change moves no commit index and sends nothing -- every repetition does the same work. K of the groups,
spread evenly over the shard, change per call, K in {1, 1 000, 65 536, all}: the repetitions ALTERNATE between removing the voter in
slot 4 and adding it back (a removal writes the cfg word; an addition also writes the six cells of the new Progress and, with device
Inflights, its window). Timed with device events around the repetitions of a region (every form of the host route synchronises; the
dense form is asynchronous), the figure the median over the regions:
    route   what the parent commit can do: rg_read_groups of the K groups (the host does not own the cfg word), rg_set_config per
            group, rg_write_cells for the added peers, rg_recompute. Those calls are unchanged by this extension, so this is the
            parent's behaviour measured in the same run on the same box. Above 65 536 groups the route is not run: its figure is
            EXTRAPOLATED linearly from 65 536 and labelled so.
    sparse  rgc_apply_conf (staged, synchronises, the answers come back to the host)
    dense   rgc_apply_conf_device (asynchronous)
Checked in the run: every status DONE, and after a removal and after an addition the cells rg_read_groups reports for the K groups
are the same on the three roads. Every engine call raises on a non-zero status; nothing is retried.
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

ROUTE_MAX = 65536
FULL, FOUR = 0x1F, 0x0F


def make_engine(torch, rg, n, max_inflight):
    E = rg.engine
    eng = rg.Engine(n, 5, max_inflight=max_inflight)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    S = eng.stride
    host = {}
    for name, v in (("match", 10), ("next", 11), ("pr_commit", 10)):
        host[name] = np.full((5, S), v, dtype=np.uint64)
    for name, v in (("commit", 10), ("term_lo", 1), ("term_hi", 10), ("cur_term", 1), ("dummy_index", 0), ("dummy_term", 0)):
        host[name] = np.full(n, v, dtype=np.uint64)
    host["cfg"] = np.full(n, E.cfg_make(FULL, 0, 0), dtype=np.uint32)
    host["pflags"] = np.zeros((n, 8), dtype=np.uint8)
    host["pflags"][:, :5] = 1 | 8
    for name, a in host.items():
        eng.load_column(E.COL.NAMES.index(name), a)
    return eng


def run(torch, rg, n, max_inflight):
    E = rg.engine
    engines = {name: make_engine(torch, rg, n, max_inflight) for name in ("route", "sparse", "dense")}
    status = torch.zeros(n, device="cuda", dtype=torch.uint8)
    count = torch.zeros(1, device="cuda", dtype=torch.int32) if max_inflight else None
    rows = []
    for K in sorted({1, min(1000, n), min(65536, n), n}):
        groups = (np.arange(K, dtype=np.uint64) * np.uint64(n // K)).astype(np.uint64)
        words = [E.cfg_make(FOUR, 0, 0, present=FOUR), E.cfg_make(FULL, 0, 0, present=FULL)]  # (self slot 0: the three fields alone)
        recs = []
        d_cfg = []
        sel = np.zeros(n, dtype=np.uint8)
        sel[groups] = 1
        d_sel = torch.from_numpy(sel).cuda()
        for w in words:
            r = np.zeros(K, dtype=E.CONF_REC_DTYPE)
            r["group"], r["cfg"] = groups, w
            recs.append(r)
            d_cfg.append(torch.from_numpy(np.full(n, w, dtype=np.uint32).view(np.int32)).cuda())

        def dense(k):
            engines["dense"].apply_conf_device(d_sel, d_cfg[k & 1], status, count=count)

        def sparse(k):
            resp, got, total = engines["sparse"].apply_conf(recs[k & 1], item_cap=0 if max_inflight else None)
            assert (resp["status"] == E.CONF_DONE).all() and total == 0

        def route(k):
            eng = engines["route"]
            cur = eng.read_groups(groups)
            add = k & 1
            for g, old in zip(groups.tolist(), cur["cfg"].tolist()):
                eng.set_config(g, (words[add] & 0xFF00FFFF) | (old & 0x00FF0000))
            if add:
                cells = (E.CellWrite * K)()
                for i, g in enumerate(groups.tolist()):
                    c = cells[i]
                    c.group, c.slot, c.field_mask, c.match, c.next, c.pflags = g, 4, 0x7F, 0, 11, 0 | 8
                eng._check(eng.L.rg_write_cells(eng.h, cells, K))
            eng.recompute()

        row = {"K": K, "max_inflight": max_inflight}
        cells_after = {}
        for name, fn, sync in (("route", route, True), ("sparse", sparse, True), ("dense", dense, False)):
            if name == "route" and K > ROUTE_MAX:
                continue
            for k in (0, 1):  # one removal, one addition: warm-up and the comparison of the three roads
                fn(k)
                torch.cuda.synchronize()
                got = engines[name].read_groups(groups[:4096])
                key = (got["cfg"].tobytes(), got["match"].tobytes(), got["next"].tobytes(), got["commit"].tobytes())
                if k == 0:  # (a removed slot's cells are without meaning: compared after the addition)
                    key = key[:1] + key[3:]
                assert cells_after.setdefault(k, key) == key, (K, name, k, "the roads leave different cells")
            steps, regions = ((2, 1) if K >= 65536 else (10, 3)) if sync else (20, 5)
            t = [timed(torch, fn, steps) for _ in range(regions)]
            row[name] = [round(float(np.median(t)), 2), round(min(t), 2), round(max(t), 2)]
        assert int((status == E.CONF_DONE).sum()) == K
        if K > ROUTE_MAX:
            base = next(r for r in rows if r["K"] == ROUTE_MAX)["route"][0]
            row["route"] = [round(base * K / ROUTE_MAX, 2)] * 3
            row["route_extrapolated"] = True
        rows.append(row)
    for eng in engines.values():
        eng.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conf_change.txt"))
    ap.add_argument("--n", type=int, default=1_000_000)
    a = ap.parse_args()
    import torch
    import raft_rs_amd as rg
    if not torch.cuda.is_available():
        raise SystemExit("bench_conf_change: no GPU (there is no CPU fallback and no CPU timing)")
    lines = [f"the batched conf change (rgc_apply_conf*) against the host route, {a.n} leader groups x 5, K groups alternately removing and adding back the voter in slot 4, one "
             "run; device events around the repetitions of a region, median (min max) over the regions, us per call; call time, launch overhead included",
             "route: rg_read_groups, rg_set_config per group, rg_write_cells for the added peers, rg_recompute (unchanged calls: the parent's behaviour, same run, same box); "
             f"above {ROUTE_MAX} groups the route is EXTRAPOLATED linearly from {ROUTE_MAX} (marked *)"]
    results = []
    for mi in (0, 8):
        rows = run(torch, rg, a.n, mi)
        results += rows
        lines.append(f"max_inflight = {mi}")
        lines.append("K       | route us                     | sparse us                  | dense us                   | route/sparse | route/dense")
        for row in rows:
            h, s, d = row["route"], row["sparse"], row["dense"]
            f = lambda v: f"{v[0]:12.2f} ({v[1]:.2f} {v[2]:.2f})"  # noqa: E731
            star = "*" if row.get("route_extrapolated") else " "
            lines.append(f"{row['K']:7d} | {f(h):27s}{star} | {f(s):26s} | {f(d):26s} | {h[0] / s[0]:12.1f} | {h[0] / d[0]:11.1f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(json.dumps({"bench": "conf_change", "n": a.n, "results": results}))


if __name__ == "__main__":
    main()
