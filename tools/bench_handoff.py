#!/usr/bin/env python3
"""Time the hand-off between the follower arena and the leader columns against the road a host had before it, in ONE run on one
MI355X.

    python tools/bench_handoff.py [--out profiles/handoff_storm.txt] [--n 1000000]

One engine: n leader groups x 3 and n followed groups. Every followed group has WON: a ten-entry log of one term with commit 8,
term 2, leader_id == self_id, three voters (own slot 0); follow group g goes to lead group g. K of them -- spread evenly over the
arena -- are handed over per call, K in {1, 1 000, 65 536, all}. Timed with device events around the repetitions of a region, the
figure the median over the regions (small K: 20 repetitions x 5 regions; from 65 536 on the host-synchronising forms run 3 x 3):
    promote   dense   rg_follow_promote_device (asynchronous; dev_persisted = NULL)
              sparse  rg_follow_promote (staged, synchronises)
              host    what the parent commit can do: rg_follow_read of the K groups, the nine log columns + MATCH rewritten on the
                      host and loaded whole (rg_load_column), one rg_tick_device carrying only RG_MF_BECOME_LEADER (its message
                      columns already on the device: in the baseline's favour), one synchronisation
    demote    dense   rg_follow_demote_device
              sparse  rg_follow_demote
              host    rg_read_groups of the K groups + rg_read_column of the table, the dummy entry and the term, rg_follow_write
A promotion leaves the arena alone and rewrites the same leader cells every time, so every repetition does the same work; the
demotions run last (they move the arena's logs on to what the promotions left). Checked in the run: every status DONE, and on the
K groups the leader columns after the dense form, after the sparse form and after the host route are the same.

Bytes per handed-over group, counted from the kernels ("The hand-off"), three present slots:
    promote   result 1 + lead 8 + log cells 48 + n_old 1 + the run table 128 + term, leader_id 16 + role 1 + self_id, conf 12 + cfg 4
              + flag row 8 read = 227; log columns 48 + run count 1 + the run table 128 + matched, next 16 per present slot 48
              + own committed_index 8 + flag row 8 + status, term, last_index 17 written = 258; 485 in all (+ 8 with dev_persisted)
    demote    select 1 + lead 8 + log columns 48 + run count 1 + the run table 128 read = 186; log cells 48 + n_old 1 + the run
              table 128 + status, term, last_index 17 written = 194; 380 in all
An unselected group of a dense call: 1 byte read, 1 written.
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

BYTES = {"promote": 485, "demote": 380, "idle": 2}
CHUNK = 1 << 17
LOG_COLS = ("commit", "term_lo", "term_hi", "cur_term", "dummy_index", "dummy_term", "run_first", "run_term", "match")


def reps(k, sync):
    return (3, 3) if sync and k >= 65536 else (20, 5)


def run(torch, rg, n):
    E = rg.engine
    C = E.COL
    eng = rg.Engine(n, 3)
    eng.follow_enable(n)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    eng.follow_gate_enable(10, seed=3)
    eng.follow_elect_enable()
    F, S = eng.follow_stride(), eng.stride
    col = lambda name: C.NAMES.index(name)  # noqa: E731
    # the leader side: every group led before at term 1 (what the cells hold is overwritten by the hand-off)
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
        eng.load_column(col(name), a)
    # the arena: every group has won at term 2
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
    lead = torch.arange(F, device="cuda", dtype=torch.int64)
    out = {"status": torch.zeros(F, device="cuda", dtype=torch.uint8), "term": torch.zeros(F, device="cuda", dtype=torch.int64),
           "last_index": torch.zeros(F, device="cuda", dtype=torch.int64)}
    m_zero = torch.zeros((3, S), device="cuda", dtype=torch.int64)
    rows, checked = [], {}

    def lead_cells(groups):
        st = eng.read_groups(groups[:4096])
        return st.tobytes()

    for K in sorted({1, min(1000, n), min(65536, n), n}):
        groups = (np.arange(K, dtype=np.uint64) * np.uint64(n // K)).astype(np.uint64)
        sel = np.zeros(F, dtype=np.uint8)
        sel[groups] = E.ELECT_WON
        d_sel = torch.from_numpy(sel).cuda()
        recs = np.zeros(K, dtype=E.HANDOFF_REC_DTYPE)
        recs["follow_group"], recs["lead_group"], recs["persisted"] = groups, groups, 10
        m_flags = np.zeros((n, 8), dtype=np.uint8)
        m_flags[groups, 0] = E.MF.BECOME_LEADER
        m_hint = np.zeros((3, S), dtype=np.uint64)
        m_hint[0, groups] = 2
        d_flags, d_hint = torch.from_numpy(m_flags).cuda(), torch.from_numpy(m_hint.view(np.int64)).cuda()

        def dense(k):
            eng.follow_promote_device(d_sel, lead, out)

        def sparse(k):
            resp = eng.follow_promote(recs)
            assert (resp["status"] == E.HANDOFF_DONE).all()

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
            eng.tick_device(m_zero.data_ptr(), m_zero.data_ptr(), d_hint.data_ptr(), m_zero.data_ptr(), d_flags.data_ptr())
            eng.sync()
        row = {"K": K}
        for name, fn, sync in (("host", route, True), ("sparse", sparse, True), ("dense", dense, False)):
            fn(0)
            torch.cuda.synchronize()
            cells = lead_cells(groups)
            assert checked.setdefault(K, cells) == cells, (K, name, "the three roads leave different leader cells")
            steps, regions = reps(K, sync)
            t = [timed(torch, fn, steps) for _ in range(regions)]
            row["promote_" + name] = [round(float(np.median(t)), 2), round(min(t), 2), round(max(t), 2)]
        assert bool((out["status"][torch.from_numpy(groups.astype(np.int64)).cuda()] == E.HANDOFF_DONE).all())
        assert int((out["status"] == E.HANDOFF_DONE).sum()) == K and bool((out["last_index"][:1] == 11).all())
        rows.append(row)
    # the demotions, on the leaders the promotions left (K ascending: all groups were promoted by the last round)
    for row in rows:
        K = row["K"]
        groups = (np.arange(K, dtype=np.uint64) * np.uint64(n // K)).astype(np.uint64)
        sel = np.zeros(F, dtype=np.uint8)
        sel[groups] = 1
        d_sel = torch.from_numpy(sel).cuda()
        recs = np.zeros(K, dtype=E.HANDOFF_REC_DTYPE)
        recs["follow_group"], recs["lead_group"] = groups, groups

        def dense(k):
            eng.follow_demote_device(d_sel, lead, out)

        def sparse(k):
            assert (eng.follow_demote(recs)["status"] == E.HANDOFF_DONE).all()

        def route(k):
            status = np.concatenate([eng.read_groups(groups[a:a + CHUNK]) for a in range(0, K, CHUNK)])
            cols = {name: eng.read_column(col(name)) for name in ("run_first", "run_term", "dummy_index", "dummy_term", "cur_term", "run_count")}
            st = np.zeros(K, dtype=E.FOLLOW_STATE_DTYPE)
            cnt = cols["run_count"][groups].astype(np.int64)
            tail = status["term_lo"] <= status["last_index"]
            st["group"], st["committed"], st["last_index"] = groups, status["commit"], status["last_index"]
            st["dummy_index"], st["dummy_term"], st["n_runs"] = cols["dummy_index"][groups], cols["dummy_term"][groups], cnt + tail
            for j in range(E.TERM_RUNS):
                st["run_first"][:, j] = np.where(j < cnt, cols["run_first"][j, groups], 0)
                st["run_term"][:, j] = np.where(j < cnt, cols["run_term"][j, groups], 0)
            idx = np.arange(K)
            st["run_first"][idx[tail], cnt[tail]] = status["term_lo"][tail]
            st["run_term"][idx[tail], cnt[tail]] = cols["cur_term"][groups][tail]
            for a in range(0, K, CHUNK):
                eng.follow_write(st[a:a + CHUNK])
        for name, fn, sync in (("host", route, True), ("sparse", sparse, True), ("dense", dense, False)):
            fn(0)
            torch.cuda.synchronize()
            got = eng.follow_read(groups[:4096])
            assert (got["last_index"] == 11).all() and (got["n_runs"] == 2).all() and (got["run_term"][:, 1] == 2).all(), (K, name)
            steps, regions = reps(K, sync)
            t = [timed(torch, fn, steps) for _ in range(regions)]
            row["demote_" + name] = [round(float(np.median(t)), 2), round(min(t), 2), round(max(t), 2)]
    eng.close()
    return {"n": n, "follow_stride": int(F), "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "handoff_storm.txt"))
    ap.add_argument("--n", type=int, default=1_000_000)
    a = ap.parse_args()
    import torch
    import raft_rs_amd as rg
    if not torch.cuda.is_available():
        raise SystemExit("bench_handoff: no GPU (there is no CPU fallback and no CPU timing)")
    r = run(torch, rg, a.n)
    lines = [f"the hand-off (rg_follow_promote* / rg_follow_demote*) against the host route, {r['n']} leader groups x 3 and {r['n']} followed groups, one run; "
             "device events around the repetitions of a region, median (min max) over the regions, us per call; call time, launch overhead included",
             f"model bytes per handed-over group: promote {BYTES['promote']}, demote {BYTES['demote']}; an unselected group of a dense call {BYTES['idle']}",
             "move    | K       | host route us              | sparse us                  | dense us                   | host/sparse | host/dense | dense model GB/s"]
    for move in ("promote", "demote"):
        for row in r["rows"]:
            h, s, d = row[move + "_host"], row[move + "_sparse"], row[move + "_dense"]
            gbs = (BYTES[move] * row["K"] + BYTES["idle"] * (r["n"] - row["K"])) / d[0] / 1e3
            f = lambda v: f"{v[0]:10.2f} ({v[1]:.2f} {v[2]:.2f})"  # noqa: E731
            lines.append(f"{move:7s} | {row['K']:7d} | {f(h):26s} | {f(s):26s} | {f(d):26s} | {h[0] / s[0]:11.1f} | {h[0] / d[0]:10.1f} | {gbs:8.1f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(json.dumps({"bench": "handoff", "results": [r]}))


if __name__ == "__main__":
    main()
