"""CPU only: the batched conf change (include/raftgroups_conf.h). (1) tests/conf_model.py -- apply_conf and post_conf_change line by
line -- against the oracle's route (ro_store_soa, the membership edit on the columns, ro_load_soa, ro_maybe_commit,
ro_maybe_send_append per peer with the oracle's own Inflights): every leader column, every window, the item set, exactly; (2) the
reference's own tests restated by hand; (3) csrc/rg_conf.h -- what the kernels run -- compiled for the HOST with g++
(tests/host_check/conf_twin.cpp, a stand-alone program) against the model over a seeded sweep, once more under AddressSanitizer +
UBSan, and against rg_group_send's literal road (tests/host_check/host_tick.hip) for the single-pass send; (4) every rgc_* name is
declared, exported and bound, the older export sets are what they were, the refusals are host checks; no kernel instantiation carries
scratch (tools/kernel_resources.py: resource metadata only).

Citations: pingcap/raft-rs v0.6.0."""
import copy
import ctypes
import os
import random
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import conf_model as M
import handoff_rig as R
import sendstage
from test_host_check import host_send  # noqa: F401  (the fixture: rg_group_send on the host)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_NAMES = ("rgc_conf_version", "rgc_apply_conf", "rgc_apply_conf_device")
U64_MAX = (1 << 64) - 1
N_GROUPS = 40


# ---------------------------------------------------------------------------------------------------------------------
# 1. the model against the oracle's route
# ---------------------------------------------------------------------------------------------------------------------
def state_of(P, cases):
    st = R.base_state(N_GROUPS, P, 256)
    for g, (name, d, W, win, expect) in enumerate(cases):
        R.put_lead(st, g, d)
    return st


def oracle_route(O, st, recs, answers, cap, max_entries=0, max_bytes=None, sizes=None, cl=None, windows=None, added_pflags=M.PROBE | M.PF_RECENT_ACTIVE):
    """ro_store_soa's columns with the membership edit on them (the cfg word's three fields; an added slot's cells = Progress::new
    with recent_active), ro_load_soa, ro_maybe_commit, ro_maybe_send_append(to, allow_empty = committed, max) per peer in slot order
    with the oracle's own Inflights (empty at the load), the transfer abort of raft.rs:2666-2671 -> (state after, messages, cluster).
    cl, windows: a cluster that lives on (tests/test_lead_sequences_host.py) is loaded in place of a new one, and gets back the windows
    {(group, slot): entries} it held -- but an added slot's, which Progress::new leaves empty; cap 0 (no device Inflights): no
    sends. added_pflags: the flag byte of an added slot (a mutation of that test changes it)."""
    P = st["n_slots"]
    edited = R.copy_state(st)
    added = set()
    for (g, W), a in zip(recs, answers):
        if a["status"] not in (M.DONE, M.DEMOTED):
            continue
        old, hi = int(edited["cfg"][g]), int(edited["term_hi"][g])
        for s in range(P):
            if (W >> 24 & ~(old >> 24)) >> s & 1:
                edited["match"][s, g], edited["next"][s, g] = 0, hi + 1
                for k in ("pr_commit", "pend_snap", "pend_rs", "gid"):
                    edited[k][s, g] = 0
                edited["pflags"][g, s] = added_pflags
                added.add((g, s))
        edited["cfg"][g] = (W & M.FIELDS) | (old & M.KEPT)
    cl = O.Cluster(st["n_groups"]) if cl is None else cl
    cl.load_soa(edited, term=3, max_inflight=cap)
    cl.set_own_inflights(cap > 0)
    for (g, s), entries in (windows or {}).items():
        if (g, s) not in added and int(edited["cfg"][g]) >> 24 >> s & 1:
            for e in entries:
                cl.L.ro_ins_add(ctypes.byref(cl.L.ro_group_progress(cl.h, g, s + 1).contents.ins), e)
    if max_bytes is not None:
        cl.set_limit_bytes(True)
        for g in range(st["n_groups"]):
            cl.append_entry_sizes(g, 1, [sizes[i] for i in range(1, int(edited["term_hi"][g]) + 1)])
    sent = []
    for (g, W), a in zip(recs, answers):
        if a["status"] != M.DONE:
            continue
        Wi, Wo, _, _, Wp = M.fields(W)
        self_slot, tr = int(edited["cfg"][g]) >> 16 & 7, int(edited["cfg"][g]) >> 20 & 0xF
        committed = bool(cl.maybe_commit(g))
        assert committed == bool(a["events"] & M.EV_COMMITTED), (g, a)
        for s in range(P if cap else 0):
            if Wp >> s & 1 and s != self_slot:
                ok, m = cl.maybe_send_append(g, s + 1, committed, max_bytes if max_bytes is not None else max_entries)
                if ok:
                    sent.append((m.group, m.to, m.index, m.n_entries, m.kind, 0))
        if tr and not (Wi | Wo) >> (tr - 1) & 1:
            cl.L.ro_group_set_transferee(cl.h, g, 0)
    after = R.copy_state(edited)
    cl.store_soa(after)
    return after, np.array(sent, dtype=O.SEND_MSG_DTYPE), cl


def model_and_route(O, P, cap, **limits):
    cases = M.edge_cases(P)
    st = state_of(P, cases)
    recs = [(g, c[2]) for g, c in enumerate(cases)]
    windows = {}
    kw = dict(limits)
    if "max_bytes" in limits:
        kw.update(sizes={i: 3 + i % 5 for i in range(64)}, esz_w=64)
    want, answers, items = M.apply_state(st, windows, recs, cap, **kw)
    assert [a["status"] for a in answers] == [c[4] for c in cases]
    after, sent, cl = oracle_route(O, st, recs, answers, cap, limits.get("max_entries", 0), limits.get("max_bytes"), kw.get("sizes"))
    diffs = R.diff(want, after)
    assert not diffs, (P, cap, limits, diffs)
    sendstage.compare_items(M.items_array(items), sent)
    for (g, W), a in zip(recs, answers):  # every window of a served group
        if a["status"] != M.DONE:
            continue
        for s in range(P):
            if W >> 24 >> s & 1:
                assert cl.ins_contents(g, s + 1) == windows.get((g, s), []), (g, s)
    return cases, answers, items, want


@pytest.mark.parametrize("cap", [1, 4, 8])
@pytest.mark.parametrize("P", [1, 3, 5, 8])
def test_model_equals_the_route_through_the_oracle(oracle, P, cap):
    """Slot counts 1, 3, 5 and 8, window caps 1, 4 and 8: every leader column, every window and the item set of the oracle's route."""
    cases, answers, items, want = model_and_route(oracle, P, cap)
    assert {a["status"] for a in answers} >= ({M.DONE, M.FAULT} if P == 1 else {M.DONE, M.DEMOTED, M.HOST, M.FAULT})
    if P > 1:
        assert any(a["events"] & M.EV_COMMITTED for a in answers) and any(a["events"] & M.EV_TRANSFER_ABORTED for a in answers)
        assert any(a["added"] for a in answers) and any(a["removed"] for a in answers)
        assert {k for _, (k, _, _, _) in items.items()} == {M.SEND_APPEND, M.SEND_SNAPSHOT}


@pytest.mark.parametrize("limits", [{"max_entries": 1}, {"max_bytes": 0}, {"max_bytes": 1}, {"max_bytes": U64_MAX}])
@pytest.mark.parametrize("cap", [1, 4, 8])
@pytest.mark.parametrize("P", [1, 3, 5, 8])
def test_limits_against_the_oracle(oracle, P, cap, limits):
    """max_entries_per_msg 1 and Config::max_size_per_msg of 0, 1 and NO_LIMIT bytes: one message per peer, cut as the reference cuts it"""
    cases, answers, items, want = model_and_route(oracle, P, cap, **limits)
    whole = model_and_route(oracle, P, cap)[2]
    cut = [k for k in items if items[k][0] == M.SEND_APPEND and items[k][2] < whole[k][2]]
    assert bool(cut) == (P > 1 and limits.get("max_bytes") != U64_MAX)
    assert all(v[3] == 1 for v in items.values()) and set(items) == set(whole)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the reference's own tests, by hand
# ---------------------------------------------------------------------------------------------------------------------
def run(d, W, P=3, cap=4, windows=None, **kw):
    d = copy.deepcopy(d)
    win = [list(w) for w in windows] if windows else [[] for _ in range(P)]
    a, items = M.apply_conf(d, win, P, cap, W, **kw)
    return d, win, a, {s: (k, p, l) for s, k, p, l, n in items}


def test_add_node_and_add_learner():
    """harness/tests/integration_cases/test_raft.rs: test_add_node (the new node is a voter with a Progress), test_add_learner (a
    learner: a Progress, no vote)"""
    d0 = M.make_group(3, 0b001, match=[20, 0, 0])
    d, win, a, items = run(d0, M.word(0b011))
    assert a["status"] == M.DONE and a["added"] == 0b010 and M.fields(d["cfg"])[0] == 0b011 and M.fields(d["cfg"])[4] == 0b011
    assert (d["match"][1], d["next"][1], d["pflags"][1]) == (0, 21, M.PROBE | M.PF_RECENT_ACTIVE) and not items  # (nothing to probe with)
    d, win, a, items = run(d0, M.word(0b001, 0, 0b011))
    assert a["added"] == 0b010 and M.fields(d["cfg"])[0] == 0b001 and M.fields(d["cfg"])[4] == 0b011 and d["next"][1] == 21


def test_remove_node_and_remove_learner():
    """test_remove_node, test_remove_learner: the Progress is gone from the configuration; its cells are without meaning"""
    d0 = M.make_group(3, 0b011, 0, 0b111)
    d, win, a, items = run(d0, M.word(0b001, 0, 0b101))
    assert a["removed"] == 0b010 and M.fields(d["cfg"])[4] == 0b101 and 1 not in items and d["match"][1] == d0["match"][1]
    d, win, a, items = run(d0, M.word(0b011))
    assert a["removed"] == 0b100 and M.fields(d["cfg"])[4] == 0b011 and 2 not in items


def test_learner_promotion_keeps_the_progress():
    """test_learner_promotion: the learner's Progress survives -- matched, next, state, its window"""
    d0 = M.make_group(3, 0b011, 0, 0b111)
    d0["match"][2], d0["next"][2] = 17, 20
    d, win, a, items = run(d0, M.word(0b111), windows=[[], [], [18, 19]])
    assert a["added"] == a["removed"] == 0 and d["match"][2] == 17 and win[2] == [18, 19, 20] and items[2] == (M.SEND_APPEND, 19, 20)


def test_commit_after_remove_node():
    """test_commit_after_remove_node: with two voters the entry waits for node 2; removing node 2 commits it -- COMMITTED, then the
    broadcast (here: to the learner that stays)"""
    d0 = M.make_group(3, 0b011, 0, 0b111, match=[20, 8, 12], commit=8)
    d, win, a, items = run(d0, M.word(0b001, 0, 0b101))
    assert a["events"] == M.EV_COMMITTED and a["out"] == M.OUT_CHANGED and d["commit"] == 20 and d["pr_commit"][0] == 20
    assert items == {2: (M.SEND_APPEND, 12, 20)}
    d0["match"][2], d0["next"][2] = 20, 21  # a peer that has everything still gets the (empty) append: allow_empty
    assert run(d0, M.word(0b001, 0, 0b101))[3] == {2: (M.SEND_APPEND, 20, 20)}


def test_leader_transfer_remove_node():
    """test_leader_transfer_remove_node: removing the transferee aborts the transfer; a transferee that stays a voter keeps it"""
    d0 = M.make_group(3, 0b111, transferee=3)
    d, win, a, items = run(d0, M.word(0b011))
    assert a["events"] & M.EV_TRANSFER_ABORTED and M.fields(d["cfg"])[3] == 0 and M.fields(a["cfg"])[3] == 0
    d, win, a, items = run(d0, M.word(0b111, 0b011))
    assert not a["events"] & M.EV_TRANSFER_ABORTED and M.fields(d["cfg"])[3] == 3
    d, win, a, items = run(d0, M.word(0b011, 0, 0b111))  # demoted to learner: no voter any more
    assert a["events"] & M.EV_TRANSFER_ABORTED


def test_joint_commit_is_the_minimum_of_both_majorities():
    """enter_joint / leave_joint (src/quorum/joint.rs:47-51): in the joint configuration the commit index is the minimum of both
    majorities and moves only at the leave"""
    d0 = M.make_group(5, 0b00111, match=[20, 9, 9, 20, 20], present=0b11111, commit=9)
    d, win, a, items = run(d0, M.word(0b11001, 0b00111, 0b11111), P=5)  # incoming {0,3,4} is at 20, outgoing {0,1,2} at 9
    assert a["status"] == M.DONE and not a["events"] and d["commit"] == 9 and M.fields(d["cfg"])[1] == 0b00111
    d, win, a, items = run(d, M.word(0b11001, 0, 0b11001), P=5, windows=win)
    assert a["events"] == M.EV_COMMITTED and d["commit"] == 20 and a["removed"] == 0b00110


def test_refusal_order_and_demotion():
    d0 = M.make_group(3, 0b111, self_slot=1)
    for W, kw, want in ((M.word(0b111) | 1 << 16, {"clock": True, "led": False}, M.FAULT), (M.word(0b101), {"clock": True, "led": False}, M.NOT_LED),
                        (M.word(0b101), {}, M.HOST), (M.word(0b101, 0, 0b111), {}, M.DEMOTED), (M.word(0b111), {"clock": True, "led": True}, M.DONE)):
        d, win, a, items = run(d0, W, **kw)
        assert a["status"] == want, (hex(W), kw, a)
        if want not in (M.DONE, M.DEMOTED):
            assert d == d0 and not items
    d0["match"] = [20, 20, 3]
    d, win, a, items = run(d0, M.word(0b101, 0, 0b111))  # raft.rs:2609-2622: the reference returns before the commit and the sends
    assert a["status"] == M.DEMOTED and not a["events"] and not items and d["commit"] == d0["commit"]


def test_model_cites_the_reference():
    src = open(os.path.join(HERE, "conf_model.py")).read()
    for needle in ("tracker.rs:380-397", "raft.rs:2604-2673", "raft.rs:773-819", ":2609-2622", ":2630", ":2633", ":2634-2646", ":2666-2671", "progress.rs:210-216",
                   "progress.rs:231-243", "util.rs:52-76", "changer.rs:285-355", "raft_log.rs:487-499"):
        assert needle in src, needle


# ---------------------------------------------------------------------------------------------------------------------
# 3. the stand-alone twin of csrc/rg_conf.h
# ---------------------------------------------------------------------------------------------------------------------
def build_twin(tmp_path, name, extra):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build the host twin")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, os.path.join(HERE, "host_check", "conf_twin.cpp"), "-o", exe])
    return exe


def sweep_cases(seed, n):
    rng = random.Random(seed)
    out = []
    for k in range(n):
        P = rng.choice((1, 3, 3, 5, 7, 8))
        full = (1 << P) - 1
        oldp = rng.randrange(1, full + 1)
        oldi = rng.randrange(1, full + 1) & oldp or oldp & -oldp
        oldo = rng.randrange(0, full + 1) & oldp if rng.random() < 0.4 else 0
        self_slot = rng.choice([s for s in range(P) if oldp >> s & 1]) if rng.random() < 0.95 else rng.randrange(P)
        tr = rng.choice([0, 0] + [s + 1 for s in range(P)])
        hi = rng.randrange(8, 40)
        dummy = rng.randrange(0, 8)
        lo = rng.randrange(dummy + 1, hi + 1)
        d = {"cfg": oldi | oldo << 8 | self_slot << 16 | tr << 20 | oldp << 24, "term_hi": hi, "term_lo": lo, "dummy_index": dummy, "commit": rng.randrange(dummy, hi + 1)}
        cap = rng.choice((1, 2, 4, 8))
        d["match"], d["next"], d["pflags"], d["pend_rs"], windows = [], [], [], [], []
        for s in range(P):
            m = hi if s == self_slot else rng.choice((0, rng.randrange(0, hi + 1), hi))
            state = rng.choice((M.PROBE, M.PROBE, M.REPLICATE, M.REPLICATE, M.REPLICATE, M.SNAPSHOT))
            pb = state | (M.PF_RECENT_ACTIVE if rng.random() < 0.8 else 0) | (M.PF_PAUSED if state == M.PROBE and rng.random() < 0.4 else 0)
            prs = rng.randrange(1, 30) if rng.random() < 0.1 else 0
            pb |= M.PF_PEND_RS if prs else 0
            cnt = rng.choice((0, 0, 1, cap)) if state == M.REPLICATE else 0
            pb |= M.PF_INS_FULL if state == M.REPLICATE and cnt == cap else 0
            d["match"].append(m)
            d["next"].append(rng.choice((m + 1, m + 1, rng.randrange(1, hi + 2))))
            d["pflags"].append(pb)
            d["pend_rs"].append(prs)
            windows.append([1] * cnt)
        d["pr_commit"], d["pend_snap"], d["gid"] = [0] * P, [0] * P, [0] * P
        r = rng.random()
        if r < 0.08:
            W = rng.randrange(1 << 32)
        else:
            Wp = oldp if r < 0.3 else rng.randrange(1, full + 1)
            Wi = rng.randrange(1, full + 1) & Wp or Wp & -Wp
            Wo = rng.randrange(0, full + 1) & Wp if rng.random() < 0.4 else 0
            W = M.word(Wi, Wo, Wp)
            if r > 0.97:
                W |= 1 << rng.randrange(8, 16) if P < 8 else 1 << 17
        clock, led = rng.random() < 0.3, rng.random() < 0.7
        flags = rng.choice((0, 0, 1, 2, 2))
        max_entries = rng.choice((0, 0, 1, 3, U64_MAX)) if not flags & 2 else rng.choice((0, 1, 9, 20, U64_MAX))
        esz_w = rng.choice((8, 16, 64)) if flags & 2 else 0
        sizes = [rng.choice((0, 1, 3, 7)) for _ in range(hi + 1)] if flags & 2 else []
        out.append((d, windows, P, cap, W, clock, led, max_entries, flags, esz_w, sizes, rng.random() < 0.85))
    return out


def run_twin(exe, cases):
    lines = []
    for d, windows, P, cap, W, clock, led, max_entries, flags, esz_w, sizes, has_ins in cases:
        pf = sum(b << (8 * s) for s, b in enumerate(d["pflags"]))
        head = [P, cap, int(has_ins), int(clock), int(led), W, d["cfg"], pf, d["term_hi"], d["term_lo"], d["commit"], d["dummy_index"], max_entries, flags, esz_w, len(sizes)]
        slots = [v for s in range(P) for v in (d["match"][s], d["next"][s], d["pend_rs"][s], len(windows[s]))]
        lines.append("C " + " ".join(str(v) for v in head + sizes + slots))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    got = out.stdout.split("\n")[:-1]
    assert len(got) == len(cases)
    seen = {"status": set(), "events": 0, "added": 0, "removed": 0, "joint": set(), "learner": 0, "peer": set(), "kinds": set()}
    for k, (line, (d, windows, P, cap, W, clock, led, max_entries, flags, esz_w, sizes, has_ins)) in enumerate(zip(got, cases)):
        w = [int(x) for x in line.split()[1:]]
        m, win = copy.deepcopy(d), ([list(x) for x in windows] if has_ins else None)
        limits = {"max_bytes": max_entries, "sizes": dict(enumerate(sizes)), "esz_w": esz_w} if flags & 2 else {"max_entries": max_entries}
        if has_ins and not M.word_check(W, P) and M.fields(d["cfg"])[4] >> M.fields(d["cfg"])[2] & 1 and (led or not clock):
            for s in range(P):  # what the sweep reached, of the peers the call looks at
                if W >> 24 >> s & 1 and s != M.fields(d["cfg"])[2] and M.fields(W)[4] >> M.fields(d["cfg"])[2] & 1 and (W | W >> 8) >> M.fields(d["cfg"])[2] & 1:
                    pb, nxt = d["pflags"][s], d["next"][s]
                    if M.fields(d["cfg"])[4] >> s & 1:
                        st = pb & 3
                        seen["peer"].add("probe" if st == M.PROBE and not pb & M.PF_PAUSED else "paused" if st == M.PROBE else
                                         "full" if st == M.REPLICATE and len(windows[s]) == cap else "replicate" if st == M.REPLICATE else "snapshot")
                        if pb & M.PF_PEND_RS:
                            seen["peer"].add("pend_rs")
                        if nxt <= d["term_hi"] and nxt < d["dummy_index"] + 1:
                            seen["peer"].add("compacted")
        a, items = M.apply_conf(m, win, P, cap, W, clock=clock, led=led, **limits)
        want = [a["status"], a["cfg"], sum(b << (8 * s) for s, b in enumerate(m["pflags"])), a["commit"], a["out"], a["events"], a["added"], a["removed"], a["n_items"]]
        assert w[:9] == want, (k, line, want, d, hex(W))
        its = {s: (kind, prev, last) for s, kind, prev, last, n in items}
        for s in range(P):
            nxt, cnt, kind, prev, last = w[9 + 5 * s:14 + 5 * s]
            assert nxt == m["next"][s] or (a["added"] >> s & 1 and nxt == d["term_hi"] + 1), (k, s, line)
            if has_ins:
                assert cnt == len(win[s]), (k, s, line)
            assert (kind, prev, last) == its.get(s, (0, 0, 0)), (k, s, line, its)
        seen["status"].add(a["status"])
        seen["events"] |= a["events"]
        seen["added"] |= a["added"]
        seen["removed"] |= a["removed"]
        seen["kinds"] |= {v[0] for v in its.values()}
        if a["status"] == M.DONE:
            seen["joint"].add(bool(W >> 8 & 0xFF))
            seen["learner"] |= W >> 24 & ~(W | W >> 8) & 0xFF
    return seen


def test_host_twin_matches_the_model(tmp_path):
    """A seeded sweep: every answer field, the flag row, the next cells, the window counts and the items the kernels would store --
    and what the sweep reached: every status, both events, slots added and removed, joint and simple words, a learner, and a peer in
    each of Probe, paused Probe, Replicate, Replicate with a full window, Snapshot, pend_rs != 0 and compacted."""
    exe = build_twin(tmp_path, "conf_twin", [])
    seen = run_twin(exe, sweep_cases(31, 6000))
    assert seen["status"] == {M.DONE, M.DEMOTED, M.NOT_LED, M.HOST, M.FAULT}
    assert seen["events"] == M.EV_COMMITTED | M.EV_TRANSFER_ABORTED and seen["added"] and seen["removed"]
    assert seen["joint"] == {True, False} and seen["learner"]
    assert seen["peer"] == {"probe", "paused", "replicate", "full", "snapshot", "pend_rs", "compacted"}
    assert seen["kinds"] == {M.SEND_APPEND, M.SEND_SNAPSHOT, M.SEND_HOST}


def test_host_twin_is_clean_under_asan_and_ubsan(tmp_path):
    """The same program, -fsanitize=address,undefined -fno-sanitize-recover=all, run directly (a stand-alone executable)."""
    exe = build_twin(tmp_path, "conf_twin_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    run_twin(exe, sweep_cases(32, 1500))


@pytest.mark.parametrize("P,cap,max_entries,flags", [(3, 4, 0, 0), (5, 8, 1, 0), (5, 1, 0, 0), (8, 8, 3, 0), (5, 8, 9, 2), (5, 8, U64_MAX, 2)])
def test_single_pass_is_rg_group_sends_first_pass(host_send, P, cap, max_entries, flags):  # noqa: F811
    """rg_group_send (csrc/rg_send.h, compiled for the host) over the cells apply_conf and maybe_commit leave, with the result word
    "send_append to every peer" (RG_OUT_SEND_APPEND bits: allow_empty) for a group that committed: where no limit splits a peer its
    items, its cells and its windows are the model's; where one does, the stage's FIRST message is the model's one."""
    cases = [c for c in M.edge_cases(P) if c[4] == M.DONE]
    st = state_of(P, cases)
    recs = [(g, c[2]) for g, c in enumerate(cases)]
    limits = {"max_bytes": max_entries, "sizes": {i: 5 for i in range(64)}, "esz_w": 64} if flags & 2 else {"max_entries": max_entries}
    windows = {}
    want, answers, items = M.apply_state(st, windows, recs, cap, **limits)
    # the stage's input: the model's state with the send effects taken back = apply_conf + maybe_commit only
    pre, _, _ = M.apply_state(st, None, recs, cap)
    out = np.zeros(N_GROUPS, dtype=np.uint32)
    for (g, W), a in zip(recs, answers):
        if a["events"] & M.EV_COMMITTED:
            out[g] = (W >> 24 & 0xFF & ~(1 << (int(pre["cfg"][g]) >> 16 & 7))) << 8
    meta, ring = np.zeros((P, 256), dtype=np.uint32), np.zeros((N_GROUPS, P, cap), dtype=np.uint64)
    head, tail = np.zeros((P, 256), dtype=np.uint64), np.zeros((P, 256), dtype=np.uint64)
    esz = np.zeros((N_GROUPS, 64), dtype=np.uint32)
    for i in range(64):
        esz[:, i] = 5 * i
    got = sendstage.items_dict(host_send(pre, out, meta, (head, tail), ring, cap, max_entries, flags, esz=esz if flags & 2 else None))
    checked = 0
    for (g, W), a in zip(recs, answers):
        if not a["events"] & M.EV_COMMITTED:
            continue
        for s in range(P):
            mine, theirs = items.get((g, s)), got.get((g, s))
            assert (mine is None) == (theirs is None), (g, s, mine, theirs)
            if mine is None:
                continue
            assert mine[:2] == theirs[:2], (g, s, mine, theirs)
            if theirs[3] == 1:
                assert mine == theirs and int(pre["next"][s, g]) == int(want["next"][s, g]) and int(pre["pflags"][g, s]) == int(want["pflags"][g, s]), (g, s, mine, theirs)
                assert int(meta[s, g]) >> 16 == len(windows[(g, s)])
            checked += 1
    assert checked


# ---------------------------------------------------------------------------------------------------------------------
# 4. declared, exported, bound; refusals are host checks; kernel resources
# ---------------------------------------------------------------------------------------------------------------------
def test_every_new_name_is_declared_exported_and_bound(rg):
    """include/raftgroups_conf.h: every function it declares is exported (as rgc_*, nothing else with that prefix) and bound, in
    Python and in the generated bindings/raftgroups_conf.rs with the header's arity; the five older headers, their export sets and
    their generated bindings are what they were."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_bindings
    from raft_rs_amd import engine as E
    hdr = open(os.path.join(ROOT, "include", "raftgroups_conf.h"), encoding="utf-8").read()
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(rgc_\w+)\s*\([^()]*\)\s*;", plain))
    assert declared == set(NEW_NAMES)
    assert not re.findall(r"\b(rg[xtvh]?_\w+)\s*\([^()]*\)\s*;", plain)  # ... and it declares no function of an older prefix
    for needle in ('#include "raftgroups.h"', "RG_SEND_SKIP_BCAST_COMMIT is accepted and has NO effect", "RG_READ_ACK_LAST_SELF", "raft.rs:2648-2664", "COST."):
        assert needle in hdr, needle
    older = {k: open(os.path.join(ROOT, "include", k), encoding="utf-8").read() for k in ("raftgroups.h", "raftgroups_lead.h", "raftgroups_term.h", "raftgroups_vote.h",
                                                                                       "raftgroups_handoff.h")}
    assert all("rgc_" not in v and "RGC_" not in v for v in older.values())
    nm = subprocess.run(["nm", "-D", "--defined-only", rg.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split() and " T " in l}
    assert {s for s in exported if s.startswith("rgc_")} == declared
    for prefix, n in {"rg_": 129, "rgx_": 8, "rgt_": 6, "rgv_": 4, "rgh_": 3}.items():  # nothing new under the older prefixes
        assert len({s for s in exported if s.startswith(prefix)}) == n, prefix
    lib = ctypes.CDLL(rg.LIB_PATH)
    for name in NEW_NAMES:
        assert hasattr(lib, name) and name in E.SYMBOLS, name
    rs = open(os.path.join(ROOT, "bindings", "raftgroups_conf.rs")).read()
    assert rs == gen_rust_bindings.generate_conf()
    for path, gen in (("raftgroups.rs", gen_rust_bindings.generate), ("raftgroups_lead.rs", gen_rust_bindings.generate_lead), ("raftgroups_term.rs", gen_rust_bindings.generate_term),
                      ("raftgroups_vote.rs", gen_rust_bindings.generate_vote), ("raftgroups_handoff.rs", gen_rust_bindings.generate_handoff)):
        assert open(os.path.join(ROOT, "bindings", path)).read() == gen(), path
    rust = {m.group(1): m.group(2) for m in re.finditer(r"pub fn (rgc_\w+)\((.*?)\)(?: -> [^;]+)?;", rs)}
    assert set(rust) == declared
    for name in declared:
        c_args = [x for x in re.search(r"\b" + name + r"\s*\(([^()]*)\)\s*;", plain, flags=re.S).group(1).split(",") if x.strip() and x.strip() != "void"]
        assert len(c_args) == len([x for x in rust[name].split(",") if x.strip()]) == len(E.SYMBOLS[name][1]), name
    for needle in ("pub struct RgcConfRec", "pub struct RgcConfResp", "pub struct RgcConfOut", "pub items: *mut RgSendItem", "pub count: *mut u32", "pub const RGC_CONF_VERSION: u32 = 1;",
                   "pub const RGC_CONF_FAULT: u32 = 5;", "host_recs: *const RgcConfRec", "dev_out: *const RgcConfOut", "use super::raftgroups::*;"):
        assert needle in rs, needle
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_bindings.py"), "--check"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lib.rgc_conf_version.restype = ctypes.c_uint32
    assert lib.rgc_conf_version() == int(re.search(r"#define RGC_CONF_VERSION (\d+)u", hdr).group(1)) == E.CONF_VERSION
    assert [f for f, _ in E.ConfOut._fields_] == list(E.CONF_OUT_FIELDS) and ctypes.sizeof(E.ConfOut) == 48
    assert E.CONF_REC_DTYPE.itemsize == 16 and E.CONF_RESP_DTYPE.itemsize == 32
    for k, v in (("NONE", M.NONE), ("DONE", M.DONE), ("DEMOTED", M.DEMOTED), ("NOT_LED", M.NOT_LED), ("HOST", M.HOST), ("FAULT", M.FAULT)):
        assert getattr(E, "CONF_" + k) == v == int(re.search(r"#define RGC_CONF_%s (\d+)u" % k, hdr).group(1))
    for method in ("apply_conf", "apply_conf_device"):
        assert callable(getattr(E.Engine, method)), method
    assert (E.ABI_VERSION, E.LEAD_VERSION, E.TERM_VERSION, E.VOTE_VERSION, E.HANDOFF_EXT_VERSION) == (12, 1, 1, 1, 1)


def test_api_refusals_are_host_checks(rg):
    """What the two calls refuse is decided on the host, before anything is staged or launched: a NULL engine comes back as
    RG_ERR_INVALID_ARG without a device; the state checks and the record walk stand in front of RG_ENTER_STEP (which refuses
    unresolved host hints where every next step does); every int entry point is a function-try-block that ends in RG_ABI_GUARD; the
    arithmetic's header needs no device header; the unit touches none of the engine's send-stage bookkeeping."""
    lib = rg.load_library()
    n = ctypes.c_uint64(7)
    assert lib.rgc_apply_conf(None, None, 0, None, 0, 0, None, 0, ctypes.byref(n)) == -1 and b"rgc_apply_conf" in lib.rg_last_error()
    assert lib.rgc_apply_conf_device(None, None, None, 0, 0, None) == -1 and b"rgc_apply_conf_device" in lib.rg_last_error()
    csrc = os.path.join(ROOT, "raft_rs_amd", "csrc")
    src = open(os.path.join(csrc, "ext_conf.hip")).read()
    for fn, needles in (("rgc_apply_conf", ("rgc_conf_state", "q.group >= h->G", "q.reserved", "rg_conf_word_check", "rg_named_once", "item_cap && !host_items")),
                        ("rgc_apply_conf_device", ("rgc_conf_state", "!dev_out->status", "dev_out->item_cap && !dev_out->items", "!dev_sel", "!dev_cfg"))):
        body = src[src.index('extern "C" int %s(' % fn):]
        body = body[:body.index("} RG_ABI_GUARD")]
        assert ") try {" in body[:700], fn
        enter = body.index("RG_ENTER_STEP(h")
        assert "RG_ENTER(h)" not in body
        for needle in needles:
            assert 0 <= body.find(needle) < enter, (fn, needle)
        for later in ("rg_stage_reserve", "hipMemsetAsync", "RGC_LAUNCH", "rg_follow_round_trip", "rgc_conf_applied", "cls_stale = true", "host_cfg_valid = false"):
            assert body.find(later) == -1 or body.find(later) > enter, (fn, later)
        assert "rgc_conf_applied(h)" in body
    state = src[src.index("static int rgc_conf_state"):src.index("// ... and what a launched call leaves behind")]
    for needle in ("unknown flags", "h->host_mirror", "RG_SEND_BYTES", "!h->esz", "h->send_ready", "h->ingested_upper", "RG_ERR_STATE", "RG_ERR_INVALID_ARG", "!h->ins_arena"):
        assert needle in state, needle
    dense = src[src.index('extern "C" int rgc_apply_conf_device('):]
    assert "h->host_cfg_valid = false" in dense and "h->cls_stale = true" in dense
    for unit in ("send_items", "send_cols", "send_last_dense", "stage_max_entries", "stage_flags", "send_counter", "rg_list_stage_ran", "send_bound"):
        assert unit not in src, unit  # the engine's send-stage bookkeeping is not this unit's
    assert "h->send_ready = " not in src
    kernels = open(os.path.join(csrc, "rg_kernels_conf.h")).read()
    code = re.sub(r"//.*", "", kernels)
    assert "__restrict__" not in code and code.count("atomicAdd(") == 1 and "__syncthreads_or(" in code and "rg_wld<" in code and "rg_wst<" in code
    assert "template <int P, typename IX, bool GC>" in code and "rg_mci_group<P>" in code
    header = open(os.path.join(csrc, "rg_conf.h")).read()
    assert '#include "rg_term.h"' in header and "hip" not in re.sub(r"//.*", "", header).lower()
    build = open(os.path.join(ROOT, "raft_rs_amd", "build.py")).read()
    assert '"ext_conf.hip"' in build and '"rg_conf.h"' in build and '"rg_kernels_conf.h"' in build and "raftgroups_conf.h" in build
    old = open(os.path.join(csrc, "abi_state.hip")).read()
    assert 'extern "C" int rg_set_config(rg_engine *h, uint64_t group, uint32_t cfg_word) try {' in old  # (the old road stays)


def test_no_instantiation_carries_scratch():
    """tools/kernel_resources.py over ext_conf.hip: exactly k_conf_list and k_conf_dense, every slot count x both index widths x
    with and without group commit, no scratch (the resource metadata of the code objects; the instruction text is not searched)."""
    if not os.path.exists(shutil.which("hipcc") or "/opt/rocm/bin/hipcc"):
        pytest.fail("hipcc is needed (the engine is built with it)")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--src=raft_rs_amd/csrc/ext_conf.hip"], cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines()[1:]:
        m = re.match(r"(\S.*?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)$", line)
        if m:
            rows[m.group(1)] = (int(m.group(2)), int(m.group(5)), int(m.group(6)))
    want = sorted("%s<%d, %s, %s>" % (k, p, ix, gc) for k in ("k_conf_list", "k_conf_dense") for p in range(1, 9) for ix in ("unsigned int", "unsigned long")
                  for gc in ("false", "true"))
    assert sorted(rows) == want, (sorted(rows), out.stderr[-1000:])
    for k, (vgpr, scratch, lds) in rows.items():
        print(k, vgpr, scratch, lds)
        assert scratch == 0 and lds <= 512, (k, vgpr, scratch, lds)
