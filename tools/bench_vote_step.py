#!/usr/bin/env python3
"""Time rgv_follow_vote_device at 1 M followed groups against the parent commit's way for the same records, in ONE process on one
MI355X.

    python tools/bench_vote_step.py [--n 1048576] [--out profiles/vote_step.txt]

One engine: n followed groups, n / 3 leader groups x 3 slots with the leader's clock. Follow group g with g % 3 == 0 holds the win
state of lead group g / 3 (term 2, a five-entry log of term 2); every other group follows nobody at term 2 over a ten-entry log of
term 1. A request is of term 3 with a log ahead of both. Three mixes:
    1_in_32     MsgRequestPreVote in every 32nd group, dev_lead NULL          (every request is granted, nothing changes)
    every       MsgRequestPreVote in every group, dev_lead NULL               (likewise)
    led_third   MsgRequestVote in every group, dev_lead names the led third   (the led third is DEPOSED and grants; the others
                                                                               become followers of term 3 and record the vote)
The first two change no state: the dense call is timed with device events around 20 repetitions, the figure the median of 5 such
regions, with the answered list (capacity = everything) and without one. led_third changes what the next call meets, so every
timed region is ONE call behind an rg_restore, the figure the median of 9. The parent's way, same records, same process, wall clock around whole synchronising calls behind the same rg_restore (median
of 3):
    not led     rg_follow_step_gated over the request records (staged, one round trip)
    led         rgx_lead_clock_read, rg_follow_demote, rg_follow_step_gated, rgx_lead_clock_write(led = 0) over the led third

Byte model per group, counted from k_vote_dense ("The dense vote step"):
    no request  the flag byte read, status / gate / events written                                                      4 B
    not led     flag 1 + term, from, index, log_term, commit, commit_term, priority 56 + hdr 1 + the soft hot cells 20 + the vote
                cell 8 + the log's hot cells 32 read; 3 answer bytes + term, commit, log_term 24 written               145 B
                (a recorded vote: + term 8, leader_id 8, clock 4, vote 8, role 1 read-modify-written                    174 B)
    deposed     the request 58 + dev_lead 8 + soft hot cells 20 + self_id 8 + role 1 + priority 8 + the lead log 49 + its run table
                128 + clock cell, tag, cfg 16 read; the arena's log 49 + run table 128 + term, leader_id, clock, vote 28 + clock
                cell 4 + 27 of answers written                                                                         532 B
The last column is the model's bytes over the call time over 8 TB/s (HBM peak); the columns of this run are larger than the
Infinity Cache only in the led_third mix.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_follow_gate import timed  # noqa: E402

PEAK = 8e12
NONE_B, FOLLOW_B, VOTED_B, DEPOSED_B = 4, 145, 174, 532
CHUNK = 1 << 17


def main():
    import torch
    import raft_rs_amd as rg
    E = rg.engine
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, nl = a.n, (a.n + 2) // 3
    eng = rg.Engine(nl, 3)
    eng.follow_enable(n)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    eng.follow_gate_enable(10, seed=3)
    eng.follow_elect_enable()
    F, S = eng.follow_stride(), eng.stride
    col = E.COL.NAMES.index
    host = {name: np.full((3, S), 5, dtype=np.uint64) for name in ("match", "next", "pr_commit")}
    for name in ("commit", "term_lo", "term_hi", "cur_term", "dummy_index", "dummy_term"):
        host[name] = np.zeros(nl, dtype=np.uint64)
    host["term_lo"][:], host["term_hi"][:], host["cur_term"][:], host["commit"][:] = 1, 5, 2, 4
    host["run_first"], host["run_term"] = np.zeros((E.TERM_RUNS, S), dtype=np.uint64), np.zeros((E.TERM_RUNS, S), dtype=np.uint64)
    host["cfg"] = np.full(nl, E.cfg_make(0x7, 0, 0), dtype=np.uint32)
    host["pflags"] = np.zeros((nl, 8), dtype=np.uint8)
    host["pflags"][:, :3] = 1
    for name, arr in host.items():
        eng.load_column(col(name), arr)
    for lo in range(0, n, CHUNK):
        g = np.arange(lo, min(n, lo + CHUNK), dtype=np.uint64)
        led = g % 3 == 0
        st = np.zeros(len(g), dtype=E.FOLLOW_STATE_DTYPE)
        st["group"], st["committed"], st["last_index"], st["n_runs"] = g, 8, 10, 1
        st["run_first"][:, 0] = 1
        st["run_term"][:, 0] = 1
        eng.follow_write(st)
        so = eng.follow_soft_read(g)
        so["term"], so["role"] = 2, 0
        so["vote"], so["leader_id"] = np.where(led, g + 1, 0), np.where(led, g + 1, 0)
        eng.follow_soft_write(so)
        ce = np.zeros(int(led.sum()), dtype=E.FOLLOW_ELECT_DTYPE)
        ce["group"], ce["self_id"], ce["conf"] = g[led], g[led] + 1, E.elect_conf_make(0x7, 0, 0)
        eng.follow_elect_write(ce)
    eng.lead_clock_enable(10, 3, E.LEAD_CLOCK_START_LED)
    eng.checkpoint()

    def dev(x):
        return torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).cuda()
    every = np.arange(n, dtype=np.uint64)
    led_groups = every[every % 3 == 0]
    lead_col = np.full(F, E.HANDOFF_NO_LEAD, np.uint64)
    lead_col[led_groups] = led_groups // 3
    d_lead = dev(lead_col)
    full = lambda v: dev(np.full(F, v, np.uint64))  # noqa: E731
    cols = {"index": full(11), "log_term": full(3), "commit": full(0), "ent_term": full(0)}
    d_term, d_from = full(3), full(7)
    out = {k: torch.zeros(F, dtype=torch.uint8, device="cuda") for k in ("status", "gate", "events")}
    out.update({k: torch.zeros(F, dtype=torch.int64, device="cuda") for k in ("term", "commit", "log_term")})
    answered = torch.zeros(F, dtype=torch.int64, device="cuda")

    def flags_of(groups, kind):
        f = np.zeros(F, np.uint8)
        f[groups] = kind
        return dev(f)

    def dense(flags, lead, listed=True):
        return eng.follow_vote_device(dict(cols, flags=flags), d_term, d_from, out, lead=lead, answered=answered if listed else None,
                                      answered_cap=F if listed else 0, sync=False)

    def records(groups, kind):
        msgs, hdrs = np.zeros(len(groups), dtype=E.FOLLOW_MSG_DTYPE), np.zeros(len(groups), dtype=E.FOLLOW_HDR_DTYPE)
        msgs["group"], msgs["flags"], msgs["index"], msgs["log_term"] = groups, kind, 11, 3
        hdrs["term"], hdrs["from"] = 3, 7
        return msgs, hdrs

    def wall(fn, repeats=3):
        ts = []
        for _ in range(repeats):
            eng.restore()
            eng.sync()
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts) * 1e6

    lines = []
    for name, groups in (("1_in_32", every[::32]), ("every", every)):
        d_flags = flags_of(groups, E.FOLLOW_MSG_PREVOTE)
        eng.restore()
        counts = eng.follow_vote_device(dict(cols, flags=d_flags), d_term, d_from, out, answered=answered, answered_cap=F)
        assert counts == (len(groups), len(groups), 0, 0, 0), counts
        t = statistics.median(timed(torch, lambda k: dense(d_flags, None), 20) for _ in range(5))
        model = len(groups) * FOLLOW_B + (n - len(groups)) * NONE_B
        msgs, hdrs = records(groups, E.FOLLOW_MSG_PREVOTE)
        tp = wall(lambda: eng.follow_step_gated(msgs, hdrs))
        t0 = statistics.median(timed(torch, lambda k: dense(d_flags, None, False), 20) for _ in range(5))
        lines.append("%-10s dense %10.2f us   %6.1f B/group  %.3f of 8 TB/s   (without the answered list %10.2f us)   | parent: sparse rg_follow_step_gated of %d records %12.2f us" %
                     (name, t, model / n, model / (t * 1e-6) / PEAK, t0, len(groups), tp))
    # ---- the led third ----
    d_flags = flags_of(every, E.FOLLOW_MSG_VOTE)
    ts = []
    for k in range(9):
        eng.restore()
        ts.append(timed(torch, lambda _: dense(d_flags, d_lead), 1))
    eng.restore()
    counts = eng.follow_vote_device(dict(cols, flags=d_flags), d_term, d_from, out, lead=d_lead, answered=answered, answered_cap=F)
    assert counts == (n, n, 0, 0, len(led_groups)), counts
    t = statistics.median(ts)
    model = len(led_groups) * DEPOSED_B + (n - len(led_groups)) * VOTED_B
    others = every[every % 3 != 0]
    msgs_o, hdrs_o = records(others, E.FOLLOW_MSG_VOTE)
    msgs_l, hdrs_l = records(led_groups, E.FOLLOW_MSG_VOTE)
    demote = np.zeros(len(led_groups), dtype=E.HANDOFF_REC_DTYPE)
    demote["follow_group"], demote["lead_group"] = led_groups, led_groups // 3
    stop = np.zeros(len(led_groups), dtype=E.LEAD_CLOCK_CELL_DTYPE)
    stop["group"], stop["term"] = led_groups // 3, 2

    def four_calls():
        eng.lead_clock_read(led_groups // 3)
        assert (eng.follow_demote(demote)["status"] == E.HANDOFF_DONE).all()
        eng.follow_step_gated(msgs_l, hdrs_l)
        eng.lead_clock_write(stop)
    t_others, t_led = wall(lambda: eng.follow_step_gated(msgs_o, hdrs_o)), wall(four_calls)
    lines.append("%-10s dense %10.2f us   %6.1f B/group  %.3f of 8 TB/s   | parent: sparse step of the %d others %12.2f us + the four-call flow of the %d led %12.2f us" %
                 ("led_third", t, model / n, model / (t * 1e-6) / PEAK, len(others), t_others, len(led_groups), t_led))
    eng.close()
    text = "rgv_follow_vote_device, %d followed groups, %d leader groups x 3 slots, medians\n" % (n, nl) + "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
