#!/usr/bin/env python3
"""Time the promotion into an engine with device Inflights (rgh_follow_promote*, include/raftgroups_handoff.h) against the road
such an engine had before it, in ONE run on one MI355X.

    python tools/bench_promote_send.py [--out profiles/promote_send.txt] [--n 1000000]

Engine A: n leader groups x 3 with max_inflight = 8 and n followed groups. Every followed group has WON: a ten-entry log of one
term with commit 8, term 2, leader_id == self_id, three voters (own slot 0); follow group g goes to lead group g. K of them --
spread evenly over the arena -- are promoted per call, K in {1, 1 000, 65 536, all}. Timed with device events around the
repetitions of a region, the figure the median over the regions (small K: 20 repetitions x 5 regions; from 65 536 on the
host-synchronising forms run 3 x 3):
    route   what the parent commit can do on such an engine: rg_follow_read of the K groups, the nine log columns + MATCH rewritten on
            the host and loaded whole (rg_load_column), one rg_tick_device_send carrying only RG_MF_BECOME_LEADER (its message columns
            already on the device: in the baseline's favour) -- the tick's send stage empties the windows and decides the first
            appends --, one synchronisation. The items stay on the device (in the baseline's favour again).
    sparse  rgh_follow_promote (staged, synchronises, the items come back to the host)
    dense   rgh_follow_promote_device (asynchronous; dev_persisted = NULL; the items into a device list of 2 K places)
    plain   for scale, on engine B of the same shape WITHOUT device Inflights: rg_follow_promote_device
A promotion leaves the arena alone and rewrites the same leader cells every time, so every repetition does the same work. Checked in
the run: every status DONE, 2 K items, every window of the K groups empty, and on the K groups the leader columns after the dense
form, after the sparse form and after the route are the same. Every engine call raises on a non-zero status; nothing is retried.

Bytes per promoted group of the dense form, counted from the kernels (three present slots): the promotion's 485 (tools/bench_handoff.py)
+ the window cells 3 x 4 + the flag row behind the first appends 8 + two items 2 x 32 = 569; an unselected group: 1 byte read, 1
written. (The item count is one atomic per workgroup that promotes somebody: not in the model.)
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

BYTES = {"promote": 485 + 3 * 4 + 8 + 2 * 32, "plain": 485, "idle": 2}
CHUNK = 1 << 17
LOG_COLS = ("commit", "term_lo", "term_hi", "cur_term", "dummy_index", "dummy_term", "run_first", "run_term", "match")


def reps(k, sync):
    return (3, 3) if sync and k >= 65536 else (20, 5)


def make_engine(torch, rg, n, max_inflight):
    """An engine of n x 3 behind an arena of n followed groups that have all won at term 2 -> (engine, host copies of its columns)"""
    E = rg.engine
    C = E.COL
    eng = rg.Engine(n, 3, max_inflight=max_inflight)
    eng.follow_enable(n)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    eng.follow_gate_enable(10, seed=3)
    eng.follow_elect_enable()
    S = eng.stride
    host = {}
    for name in ("match", "next", "pr_commit"):
        host[name] = np.full((3, S), 5, dtype=np.uint64)
    for name in ("commit", "term_lo", "term_hi", "cur_term", "dummy_index", "dummy_term"):
        host[name] = np.zeros(n, dtype=np.uint64)
    host["term_lo"][:], host["term_hi"][:], host["cur_term"][:], host["commit"][:] = 1, 5, 1, 4
    host["run_first"], host["run_term"] = np.zeros((E.TERM_RUNS, S), dtype=np.uint64), np.zeros((E.TERM_RUNS, S), dtype=np.uint64)
    host["cfg"] = np.full(n, E.cfg_make(0x7, 0, 0), dtype=np.uint32)
    host["pflags"] = np.zeros((n, 8), dtype=np.uint8)
    host["pflags"][:, :3] = 1
    for name, a in host.items():
        eng.load_column(C.NAMES.index(name), a)
    for a in range(0, n, CHUNK):
        g = np.arange(a, min(n, a + CHUNK), dtype=np.uint64)
        st = np.zeros(len(g), dtype=E.FOLLOW_STATE_DTYPE)
        st["group"], st["committed"], st["last_index"], st["n_runs"] = g, 8, 10, 1
        st["run_first"][:, 0] = 1
        st["run_term"][:, 0] = 1
        eng.follow_write(st)
        so = eng.follow_soft_read(g)
        so["term"], so["vote"], so["leader_id"], so["role"] = 2, g + 1, g + 1, 0
        eng.follow_soft_write(so)
        ce = np.zeros(len(g), dtype=E.FOLLOW_ELECT_DTYPE)
        ce["group"], ce["self_id"], ce["conf"] = g, g + 1, E.elect_conf_make(0x7, 0, 0)
        eng.follow_elect_write(ce)
    return eng, host


def run(torch, rg, n):
    E = rg.engine
    col = lambda name: E.COL.NAMES.index(name)  # noqa: E731
    eng, host = make_engine(torch, rg, n, 8)
    plain_eng, _ = make_engine(torch, rg, n, 0)
    F, S = eng.follow_stride(), eng.stride
    lead = torch.arange(F, device="cuda", dtype=torch.int64)
    out = {"status": torch.zeros(F, device="cuda", dtype=torch.uint8), "term": torch.zeros(F, device="cuda", dtype=torch.int64),
           "last_index": torch.zeros(F, device="cuda", dtype=torch.int64)}
    m_zero = torch.zeros((3, S), device="cuda", dtype=torch.int64)
    count = torch.zeros(1, device="cuda", dtype=torch.int32)
    rows, checked = [], {}

    def lead_cells(groups):
        return eng.read_groups(groups[:4096]).tobytes()

    for K in sorted({1, min(1000, n), min(65536, n), n}):
        groups = (np.arange(K, dtype=np.uint64) * np.uint64(n // K)).astype(np.uint64)
        sel = np.zeros(F, dtype=np.uint8)
        sel[groups] = E.ELECT_WON
        d_sel = torch.from_numpy(sel).cuda()
        d_groups = torch.from_numpy(groups.astype(np.int64)).cuda()
        recs = np.zeros(K, dtype=E.HANDOFF_REC_DTYPE)
        recs["follow_group"], recs["lead_group"], recs["persisted"] = groups, groups, 10
        m_flags = np.zeros((n, 8), dtype=np.uint8)
        m_flags[groups, 0] = E.MF.BECOME_LEADER
        m_hint = np.zeros((3, S), dtype=np.uint64)
        m_hint[0, groups] = 2
        d_flags, d_hint = torch.from_numpy(m_flags).cuda(), torch.from_numpy(m_hint.view(np.int64)).cuda()
        items = torch.zeros(2 * K * 32, device="cuda", dtype=torch.uint8)

        def dense(k):
            eng.follow_promote_send_device(d_sel, lead, out, items, 2 * K, count)

        def sparse(k):
            resp, got, total = eng.follow_promote_send(recs)
            assert (resp["status"] == E.HANDOFF_DONE).all() and total == 2 * K == len(got)

        def route(k):
            logs = np.concatenate([eng.follow_read(groups[a:a + CHUNK]) for a in range(0, K, CHUNK)])
            h = host
            h["commit"][groups], h["term_hi"][groups] = logs["committed"], logs["last_index"]
            h["dummy_index"][groups], h["dummy_term"][groups] = logs["dummy_index"], logs["dummy_term"]
            tail = logs["n_runs"].astype(np.int64) - 1  # (every log of this run has one run: the tail)
            h["term_lo"][groups], h["cur_term"][groups] = logs["run_first"][np.arange(K), tail], logs["run_term"][np.arange(K), tail]
            h["run_first"][:, groups], h["run_term"][:, groups] = 0, 0
            h["match"][0, groups] = logs["last_index"]
            for name in LOG_COLS:
                eng.load_column(col(name), h[name])
            eng.tick_device_send(m_zero.data_ptr(), m_zero.data_ptr(), d_hint.data_ptr(), m_zero.data_ptr(), d_flags.data_ptr())
            eng.sync()

        def plain(k):
            plain_eng.follow_promote_device(d_sel, lead, out)
        row = {"K": K}
        for name, fn, sync in (("route", route, True), ("sparse", sparse, True), ("dense", dense, False)):
            fn(0)
            torch.cuda.synchronize()
            cells = lead_cells(groups)
            assert checked.setdefault(K, cells) == cells, (K, name, "the three roads leave different leader cells")
            meta = np.empty((3, S), dtype=np.uint32)
            eng._check(eng.L.rg_read_inflights(eng.h, meta.ctypes.data, None))  # (the window cells alone: no ring)
            assert not meta[:, groups[:4096]].any(), (K, name, "a window of a promoted group is not empty")
            steps, regions = reps(K, sync)
            t = [timed(torch, fn, steps) for _ in range(regions)]
            row[name] = [round(float(np.median(t)), 2), round(min(t), 2), round(max(t), 2)]
        assert int(count.cpu()[0]) == 2 * K and bool((out["status"][d_groups] == E.HANDOFF_DONE).all())
        assert int((out["status"] == E.HANDOFF_DONE).sum()) == K and bool((out["last_index"][:1] == 11).all())
        got = items.cpu().numpy().view(E.SEND_ITEM_DTYPE)
        assert set(got["group"].tolist()) == set(groups.tolist()) and (got["last_index"] == 11).all() and (got["prev_index"] == 10).all() and (got["slot"] != 0).all()
        plain(0)
        torch.cuda.synchronize()
        steps, regions = reps(K, False)
        t = [timed(torch, plain, steps) for _ in range(regions)]
        row["plain"] = [round(float(np.median(t)), 2), round(min(t), 2), round(max(t), 2)]
        rows.append(row)
    eng.close()
    plain_eng.close()
    return {"n": n, "follow_stride": int(F), "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "promote_send.txt"))
    ap.add_argument("--n", type=int, default=1_000_000)
    a = ap.parse_args()
    import torch
    import raft_rs_amd as rg
    if not torch.cuda.is_available():
        raise SystemExit("bench_promote_send: no GPU (there is no CPU fallback and no CPU timing)")
    r = run(torch, rg, a.n)
    lines = [f"the promotion into an engine with device Inflights (rgh_follow_promote*) against the parent's route, {r['n']} leader groups x 3 with max_inflight = 8 and "
             f"{r['n']} followed groups, one run; device events around the repetitions of a region, median (min max) over the regions, us per call; call time, "
             "launch overhead included",
             "route: rg_follow_read, the column loads, rg_tick_device_send with the RG_MF_BECOME_LEADER event, one synchronisation; plain: rg_follow_promote_device on an "
             "engine of the same shape without Inflights, for scale",
             f"model bytes per promoted group of the dense form: the promotion's 485 + window cells 3 x 4 + flag row 8 + items 2 x 32 = {BYTES['promote']}; an unselected "
             f"group {BYTES['idle']}",
             "K       | route us                   | sparse us                  | dense us                   | plain us                   | route/sparse | route/dense | dense model GB/s"]
    for row in r["rows"]:
        h, s, d, p = row["route"], row["sparse"], row["dense"], row["plain"]
        gbs = (BYTES["promote"] * row["K"] + BYTES["idle"] * (r["n"] - row["K"])) / d[0] / 1e3
        f = lambda v: f"{v[0]:10.2f} ({v[1]:.2f} {v[2]:.2f})"  # noqa: E731
        lines.append(f"{row['K']:7d} | {f(h):26s} | {f(s):26s} | {f(d):26s} | {f(p):26s} | {h[0] / s[0]:12.1f} | {h[0] / d[0]:11.1f} | {gbs:8.1f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(json.dumps({"bench": "promote_send", "results": [r]}))


if __name__ == "__main__":
    main()
