"""CPU only: the batched leader transfer (include/raftgroups_transfer.h). (1) tests/transfer_model.py -- handle_transfer_leader line
by line -- against the oracle's route (ro_load_soa, the model's checks, ro_group_set_transferee, ro_maybe_send_append(allow_empty =
true) with the oracle's own Inflights, ro_store_soa): every leader column, every window, the item set, exactly; (2) the reference's
test_leader_transfer_* restated by hand as far as they concern the leader's handler; (3) csrc/rg_transfer.h -- what the kernels run --
compiled for the HOST with g++ (tests/host_check/transfer_twin.cpp, a stand-alone program) against the model over the edge cases and
a seeded sweep, once more under AddressSanitizer + UBSan; (4) every rgm_* name is declared, exported and bound, the older export sets
are what they were, the refusals are host checks; no kernel instantiation carries scratch (tools/kernel_resources.py: resource
metadata only).

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

import conf_model as CM
import handoff_rig as R
import sendstage
import transfer_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_NAMES = ("rgm_transfer_version", "rgm_transfer_leader", "rgm_transfer_leader_device")
U64_MAX = (1 << 64) - 1
N_GROUPS = 40
ALL_STATUSES = {M.STARTED, M.SELF, M.IN_PROGRESS, M.LEARNER, M.NO_PROGRESS, M.NOT_LED, M.FAULT}


# ---------------------------------------------------------------------------------------------------------------------
# 1. the model against the oracle's route
# ---------------------------------------------------------------------------------------------------------------------
def model_and_route(O, P, cap, **limits):
    cases = M.edge_cases(P)
    st = R.base_state(N_GROUPS, P, 256)
    windows, led = {}, {}
    for g, (name, d, t, win, expect) in enumerate(cases):
        R.put_lead(st, g, d)
        for s, shape in win.items():
            windows[(g, s)] = M.window_entries(shape, cap, d["match"][s])
        if expect == M.NOT_LED:
            led[g] = False
    loaded = {k: list(v) for k, v in windows.items()}
    recs = [(g, c[2]) for g, c in enumerate(cases)]
    kw = dict(limits)
    if "max_bytes" in limits:
        kw.update(sizes={i: 3 + i % 5 for i in range(64)}, esz_w=64)
    want, answers, items = M.apply_state(st, windows, recs, cap, led=led, **kw)
    assert [a["status"] for a in answers] == [c[4] for c in cases]
    # the route: the checks are the model's; what they lead to is the oracle's
    cl = O.Cluster(N_GROUPS)
    cl.load_soa(st, term=3, max_inflight=cap)
    cl.set_own_inflights(True)
    for (g, s), entries in loaded.items():
        for e in entries:
            cl.L.ro_ins_add(ctypes.byref(cl.L.ro_group_progress(cl.h, g, s + 1).contents.ins), e)
    if "max_bytes" in limits:
        cl.set_limit_bytes(True)
        for g in range(N_GROUPS):
            cl.append_entry_sizes(g, 1, [kw["sizes"][i] for i in range(1, int(st["term_hi"][g]) + 1)])
    sent = []
    for (g, t), a in zip(recs, answers):
        if a["previous"]:
            cl.L.ro_group_set_transferee(cl.h, g, 0)
        if a["status"] != M.STARTED:
            continue
        cl.L.ro_group_set_transferee(cl.h, g, t + 1)
        assert bool(a["events"] & M.EV_TIMEOUT_NOW) == (cl.pr(g, t + 1).matched == cl.last_index(g)), (g, a)
        if a["events"] & M.EV_APPEND:
            ok, m = cl.maybe_send_append(g, t + 1, True, limits["max_bytes"] if "max_bytes" in limits else limits.get("max_entries", 0))
            if ok:
                sent.append((m.group, m.to, m.index, m.n_entries, m.kind, 0))
    after = R.copy_state(st)
    cl.store_soa(after)
    diffs = R.diff(want, after)
    assert not diffs, (P, cap, limits, diffs)
    sendstage.compare_items(M.items_array(items), np.array(sent, dtype=O.SEND_MSG_DTYPE))
    for g in range(len(cases)):
        for s in range(P):
            if int(st["cfg"][g]) >> 24 >> s & 1:
                assert cl.ins_contents(g, s + 1) == windows.get((g, s), []), (g, s)
    return cases, answers, items, want


@pytest.mark.parametrize("cap", [1, 4, 8])
@pytest.mark.parametrize("P", [1, 3, 5, 8])
def test_model_equals_the_route_through_the_oracle(oracle, P, cap):
    """Slot counts 1, 3, 5 and 8, window caps 1, 4 and 8: every leader column, every window and the item set of the oracle's route."""
    cases, answers, items, want = model_and_route(oracle, P, cap)
    seen = {a["status"] for a in answers}
    assert seen == (ALL_STATUSES if P > 1 else {M.SELF, M.NOT_LED, M.FAULT, M.LEARNER, M.IN_PROGRESS})
    if P > 1:
        by_name = {c[0]: (a, g) for g, (c, a) in enumerate(zip(cases, answers))}
        assert by_name["started_uptodate"][0]["events"] == M.EV_TIMEOUT_NOW and by_name["started_lagging"][0]["events"] == M.EV_APPEND
        assert by_name["second_to_another"][0]["events"] == M.EV_APPEND | M.EV_ABORTED_PREVIOUS and by_name["second_to_another"][0]["previous"] == 3
        assert by_name["to_self_previous"][0]["events"] == M.EV_ABORTED_PREVIOUS and by_name["to_self_previous"][0]["previous"] == 2
        assert by_name["to_self"][0]["events"] == 0 and by_name["outgoing_only"][0]["status"] == M.STARTED
        for quiet in ("started_paused_probe", "started_full_window", "started_snapshot_state"):
            a, g = by_name[quiet]
            assert a["events"] & M.EV_APPEND and a["n_items"] == 0 and not [k for k in items if k[0] == g], quiet
        assert {v[0] for v in items.values()} == {CM.SEND_APPEND, CM.SEND_SNAPSHOT}
        assert items[(by_name["started_pending_request"][1], 1)][:3] == (CM.SEND_SNAPSHOT, 9, 17)
        assert items[(by_name["started_compacted"][1], 1)][:3] == (CM.SEND_SNAPSHOT, 4, 0)


@pytest.mark.parametrize("limits", [{"max_entries": 1}, {"max_bytes": 0}, {"max_bytes": 1}, {"max_bytes": U64_MAX}])
@pytest.mark.parametrize("cap", [1, 4, 8])
@pytest.mark.parametrize("P", [1, 3, 5, 8])
def test_limits_against_the_oracle(oracle, P, cap, limits):
    """max_entries_per_msg 1 and Config::max_size_per_msg of 0, 1 and NO_LIMIT bytes: one message, cut as the reference cuts it"""
    cases, answers, items, want = model_and_route(oracle, P, cap, **limits)
    whole = model_and_route(oracle, P, cap)[2]
    cut = [k for k in items if items[k][0] == CM.SEND_APPEND and items[k][2] < whole[k][2]]
    assert bool(cut) == (P > 1 and limits.get("max_bytes") != U64_MAX)
    assert all(v[3] == 1 for v in items.values()) and set(items) == set(whole)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the reference's own tests, by hand (harness/tests/integration_cases/test_raft.rs)
# ---------------------------------------------------------------------------------------------------------------------
def run(d, t, P=3, cap=4, windows=None, **kw):
    d = copy.deepcopy(d)
    win = [list(w) for w in windows] if windows else [[] for _ in range(P)]
    a, items = M.transfer_leader(d, win, P, cap, t, **kw)
    return d, win, a, {s: (k, p, l) for s, k, p, l, n in items}


def test_leader_transfer_to_uptodate_node():
    """test_leader_transfer_to_uptodate_node: the transferee has the whole log: MsgTimeoutNow at once, no append"""
    d0 = M.make_group(3, 0b111, match=[20, 20, 20])
    d, win, a, items = run(d0, 1)
    assert a["status"] == M.STARTED and a["events"] == M.EV_TIMEOUT_NOW and not items and M.fields(d["cfg"])[3] == 2
    d["cfg"] = d0["cfg"]
    assert d == d0  # (nothing but the TRANSFEREE bits)


def test_leader_transfer_to_slow_follower():
    """test_leader_transfer_to_slow_follower: the transferee lags: the leader sends the append first; MsgTimeoutNow is the tick's, once
    the ack arrives"""
    d0 = M.make_group(3, 0b111, match=[20, 20, 12])
    d, win, a, items = run(d0, 2)
    assert a["status"] == M.STARTED and a["events"] == M.EV_APPEND and a["matched"] == 12 and a["last_index"] == 20
    assert items == {2: (CM.SEND_APPEND, 12, 20)} and win[2] == [20] and d["next"][2] == 21 and M.fields(d["cfg"])[3] == 3


def test_leader_transfer_to_self():
    """test_leader_transfer_to_self: ignored, the leader stays"""
    d0 = M.make_group(3, 0b111)
    d, win, a, items = run(d0, 0)
    assert a["status"] == M.SELF and not a["events"] and not items and d == d0


def test_leader_transfer_to_non_existing_node():
    """test_leader_transfer_to_non_existing_node: no Progress: ignored"""
    d0 = M.make_group(3, 0b011)
    d, win, a, items = run(d0, 2)
    assert a["status"] == M.NO_PROGRESS and a["matched"] == 0 and not items and d == d0


def test_leader_transfer_to_learner():
    """test_leader_transfer_to_learner: a learner cannot become the leader: ignored"""
    d0 = M.make_group(3, 0b011, 0, 0b111)
    d, win, a, items = run(d0, 2)
    assert a["status"] == M.LEARNER and not items and d == d0
    d0 = M.make_group(3, 0b011, 0b111)  # ... a voter of the outgoing majority alone is no learner
    assert run(d0, 2)[2]["status"] == M.STARTED


def test_leader_transfer_second_transfer_to_another_node():
    """test_leader_transfer_second_transfer_to_another_node: the first transfer is aborted, the second starts -- and
    election_elapsed starts again"""
    d0 = M.make_group(3, 0b111, match=[20, 20, 12], transferee=3)
    cell = {"tag": 3, "hb": 1, "el": 6}
    d, win, a, items = run(d0, 1, clock=True, cell=cell)
    assert a["status"] == M.STARTED and a["events"] == M.EV_TIMEOUT_NOW | M.EV_ABORTED_PREVIOUS and a["previous"] == 3
    assert M.fields(d["cfg"])[3] == 2 and cell == {"tag": 3, "hb": 1, "el": 0}


def test_leader_transfer_second_transfer_to_same_node():
    """test_leader_transfer_second_transfer_to_same_node: ignored -- the election counter is NOT reset, so the first transfer's
    timeout still holds"""
    d0 = M.make_group(3, 0b111, match=[20, 20, 12], transferee=3)
    cell = {"tag": 3, "hb": 1, "el": 6}
    d, win, a, items = run(d0, 2, clock=True, cell=cell)
    assert a["status"] == M.IN_PROGRESS and not a["events"] and not items and d == d0 and cell == {"tag": 3, "hb": 1, "el": 6}


def test_check_order_and_the_unarmed_clock_cell():
    d0 = M.make_group(3, 0b110, 0, 0b111, self_slot=0, transferee=2)  # the leader is a learner by now
    for t, kw, want in ((3, {"clock": True, "led": False}, M.FAULT), (1, {"clock": True, "led": False}, M.NOT_LED), (0, {}, M.LEARNER), (1, {}, M.IN_PROGRESS),
                        (2, {}, M.STARTED)):
        d, win, a, items = run(d0, t, **kw)
        assert a["status"] == want, (t, kw, a)
        if want != M.STARTED:
            assert d == d0 and not items
    cell = {"tag": 2, "hb": 2, "el": 7}  # a leadership the clock has not armed yet: the cell is left alone
    d, win, a, items = run(M.make_group(3, 0b111), 1, clock=True, cell=cell)
    assert a["status"] == M.STARTED and cell == {"tag": 2, "hb": 2, "el": 7}


def test_model_cites_the_reference():
    src = open(os.path.join(HERE, "transfer_model.py")).read()
    for needle in ("raft.rs:1821-1889", "raft.rs:1822-1829", ":1832-1839", ":1841-1851", ":1852", ":1860-1866", ":1876", ":1877", ":1879-1885", ":1887", "raft.rs:773-819"):
        assert needle in src, needle


# ---------------------------------------------------------------------------------------------------------------------
# 3. the stand-alone twin of csrc/rg_transfer.h
# ---------------------------------------------------------------------------------------------------------------------
def build_twin(tmp_path, name, extra):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build the host twin")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, os.path.join(HERE, "host_check", "transfer_twin.cpp"), "-o", exe])
    return exe


def edge_twin_cases():
    """the model's edge cases for every slot count, with and without windows, the NOT_LED ones under a stopped clock cell"""
    out = []
    for P in (1, 3, 5, 8):
        for cap in (1, 4):
            for name, d, t, win, expect in M.edge_cases(P):
                windows = [M.window_entries(win.get(s, "empty"), cap, d["match"][s]) for s in range(P)]
                clock = expect == M.NOT_LED
                cell = {"tag": d["cur_term"], "hb": 1, "el": 4, "stopped": clock}
                for has_ins in (True, False):
                    out.append((copy.deepcopy(d), windows, P, cap, t, clock, not clock, cell, 0, 0, 0, [], has_ins))
    return out


def sweep_cases(seed, n):
    rng = random.Random(seed)
    out = []
    for k in range(n):
        P = rng.choice((1, 3, 3, 5, 7, 8))
        full = (1 << P) - 1
        present = rng.randrange(1, full + 1)
        incoming = rng.randrange(1, full + 1) & present or present & -present
        outgoing = rng.randrange(0, full + 1) & present if rng.random() < 0.4 else 0
        self_slot = rng.choice([s for s in range(P) if present >> s & 1]) if rng.random() < 0.95 else rng.randrange(P)
        tr = rng.choice([0, 0] + [s + 1 for s in range(P)])
        hi = rng.randrange(8, 40)
        dummy = rng.randrange(0, 8)
        cur_term = rng.randrange(1, 9)
        d = {"cfg": incoming | outgoing << 8 | self_slot << 16 | tr << 20 | present << 24, "term_hi": hi, "dummy_index": dummy, "cur_term": cur_term}
        cap = rng.choice((1, 2, 4, 8))
        d["match"], d["next"], d["pflags"], d["pend_rs"], windows = [], [], [], [], []
        for s in range(P):
            m = hi if s == self_slot else rng.choice((0, rng.randrange(0, hi + 1), hi))
            state = rng.choice((CM.PROBE, CM.PROBE, CM.REPLICATE, CM.REPLICATE, CM.REPLICATE, CM.SNAPSHOT))
            pb = state | (CM.PF_RECENT_ACTIVE if rng.random() < 0.8 else 0) | (CM.PF_PAUSED if state == CM.PROBE and rng.random() < 0.4 else 0)
            prs = rng.randrange(1, 30) if rng.random() < 0.1 else 0
            pb |= CM.PF_PEND_RS if prs else 0
            cnt = rng.choice((0, 0, 1, cap)) if state == CM.REPLICATE else 0
            pb |= CM.PF_INS_FULL if state == CM.REPLICATE and cnt == cap else 0
            d["match"].append(m)
            d["next"].append(rng.choice((m + 1, m + 1, rng.randrange(1, hi + 2))))
            d["pflags"].append(pb)
            d["pend_rs"].append(prs)
            windows.append([1] * cnt)
        t = rng.randrange(P) if rng.random() < 0.93 else rng.choice((P, P + 1, 200, 254))
        clock = rng.random() < 0.5
        cell = {"tag": cur_term if rng.random() < 0.7 else cur_term - 1, "hb": rng.randrange(0, 3), "el": rng.randrange(0, 10), "stopped": rng.random() < 0.25}
        led = cell["tag"] != cur_term or not cell["stopped"]
        flags = rng.choice((0, 0, 2, 2))
        max_entries = rng.choice((0, 0, 1, 3, U64_MAX)) if not flags & 2 else rng.choice((0, 1, 9, 20, U64_MAX))
        esz_w = rng.choice((8, 16, 64)) if flags & 2 else 0
        sizes = [rng.choice((0, 1, 3, 7)) for _ in range(hi + 1)] if flags & 2 else []
        out.append((d, windows, P, cap, t, clock, led, cell, max_entries, flags, esz_w, sizes, rng.random() < 0.85))
    return out


def run_twin(exe, cases):
    lines = []
    for d, windows, P, cap, t, clock, led, cell, max_entries, flags, esz_w, sizes, has_ins in cases:
        pf = sum(b << (8 * s) for s, b in enumerate(d["pflags"]))
        word = cell["hb"] | cell["el"] << 14 | (1 << 31 if cell["stopped"] else 0)
        ts = t if t < P else 0
        head = [P, cap, int(has_ins), int(clock), int(led), t, d["cfg"], pf, d["term_hi"], d["dummy_index"], d["cur_term"], cell["tag"], word, max_entries, flags, esz_w, len(sizes)]
        lines.append("T " + " ".join(str(v) for v in head + sizes + [d["match"][ts], d["next"][ts], d["pend_rs"][ts], len(windows[ts])]))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    got = out.stdout.split("\n")[:-1]
    assert len(got) == len(cases)
    seen = {"status": set(), "events": 0, "peer": set(), "kinds": set(), "unarmed": 0, "reset": 0}
    for k, (line, (d, windows, P, cap, t, clock, led, cell, max_entries, flags, esz_w, sizes, has_ins)) in enumerate(zip(got, cases)):
        w = [int(x) for x in line.split()[1:]]
        m, win = copy.deepcopy(d), ([list(x) for x in windows] if has_ins else None)
        c = {"tag": cell["tag"], "hb": cell["hb"], "el": cell["el"]}
        limits = {"max_bytes": max_entries, "sizes": dict(enumerate(sizes)), "esz_w": esz_w} if flags & 2 else {"max_entries": max_entries}
        a, items = M.transfer_leader(m, win, P, cap, t, clock=clock, led=led, cell=c if clock else None, **limits)
        ts = t if t < P else 0
        word = c["hb"] | c["el"] << 14 | (1 << 31 if cell["stopped"] else 0)
        kind, prev, last = ([(i[1], i[2], i[3]) for i in items] + [(0, 0, 0)])[0]
        want = [a["status"], a["cfg"], sum(b << (8 * s) for s, b in enumerate(m["pflags"])), a["events"], a["previous"], a["matched"], word, m["next"][ts],
                len(win[ts]) if has_ins else len(windows[ts]), kind, prev, last]
        assert w == want, (k, line, want, d, t)
        seen["status"].add(a["status"])
        seen["events"] |= a["events"]
        seen["kinds"].add(kind)
        if a["status"] == M.STARTED and clock:
            seen["unarmed" if cell["tag"] != d["cur_term"] else "reset"] += 1
        if a["status"] == M.STARTED and a["events"] & M.EV_APPEND and has_ins:
            pb, nxt = d["pflags"][t], d["next"][t]
            st = pb & 3
            seen["peer"].add("probe" if st == CM.PROBE and not pb & CM.PF_PAUSED else "paused" if st == CM.PROBE else
                             "full" if st == CM.REPLICATE and len(windows[t]) == cap else "replicate" if st == CM.REPLICATE else "snapshot")
            if pb & CM.PF_PEND_RS:
                seen["peer"].add("pend_rs")
            if nxt <= d["term_hi"] and nxt < d["dummy_index"] + 1:
                seen["peer"].add("compacted")
    return seen


def test_host_twin_matches_the_model(tmp_path):
    """The edge cases and a seeded sweep: every answer field, the flag row, the clock cell, the transferee's next cell and window
    count and the item the kernels would store -- and what the sweep reached: every status, every event, an armed and an unarmed
    clock cell, and a transferee in each of Probe, paused Probe, Replicate, Replicate with a full window, Snapshot, pend_rs != 0 and
    compacted."""
    exe = build_twin(tmp_path, "transfer_twin", [])
    seen = run_twin(exe, edge_twin_cases())
    assert seen["status"] == ALL_STATUSES
    seen = run_twin(exe, sweep_cases(41, 6000))
    assert seen["status"] == ALL_STATUSES
    assert seen["events"] == M.EV_TIMEOUT_NOW | M.EV_APPEND | M.EV_ABORTED_PREVIOUS and seen["unarmed"] and seen["reset"]
    assert seen["peer"] == {"probe", "paused", "replicate", "full", "snapshot", "pend_rs", "compacted"}
    assert seen["kinds"] == {0, CM.SEND_APPEND, CM.SEND_SNAPSHOT, CM.SEND_HOST}


def test_host_twin_is_clean_under_asan_and_ubsan(tmp_path):
    """The same program, -fsanitize=address,undefined -fno-sanitize-recover=all, run directly (a stand-alone executable)."""
    exe = build_twin(tmp_path, "transfer_twin_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    run_twin(exe, edge_twin_cases() + sweep_cases(42, 1500))


# ---------------------------------------------------------------------------------------------------------------------
# 4. declared, exported, bound; refusals are host checks; kernel resources
# ---------------------------------------------------------------------------------------------------------------------
def test_every_new_name_is_declared_exported_and_bound(rg):
    """include/raftgroups_transfer.h: every function it declares is exported (as rgm_*, nothing else with that prefix) and bound, in
    Python and in the generated bindings/raftgroups_transfer.rs with the header's arity; the six older headers, their export sets and
    their generated bindings are what they were."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_bindings
    from raft_rs_amd import engine as E
    hdr = open(os.path.join(ROOT, "include", "raftgroups_transfer.h"), encoding="utf-8").read()
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(rgm_\w+)\s*\([^()]*\)\s*;", plain))
    assert declared == set(NEW_NAMES)
    assert not re.findall(r"\b(rg[xtvhc]?_\w+)\s*\([^()]*\)\s*;", plain)  # ... and it declares no function of an older prefix
    assert re.findall(r'#include "(\w+\.h)"', plain) == ["raftgroups.h"]
    for needle in ("raft.rs:1821-1889", "election_elapsed is NOT reset", "RG_SEND_BYTES only", "COST.", "profiles/transfer.txt"):
        assert needle in hdr, needle
    older = {k: open(os.path.join(ROOT, "include", k), encoding="utf-8").read() for k in ("raftgroups.h", "raftgroups_lead.h", "raftgroups_term.h", "raftgroups_vote.h",
                                                                                       "raftgroups_handoff.h", "raftgroups_conf.h")}
    assert all("rgm_" not in v and "RGM_" not in v for v in older.values())
    nm = subprocess.run(["nm", "-D", "--defined-only", rg.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split() and " T " in l}
    assert {s for s in exported if s.startswith("rgm_")} == declared
    for prefix, n in {"rg_": 129, "rgx_": 8, "rgt_": 6, "rgv_": 4, "rgh_": 3, "rgc_": 3}.items():  # nothing new under the older prefixes
        assert len({s for s in exported if s.startswith(prefix)}) == n, prefix
    assert len(exported) == 129 + 8 + 6 + 4 + 3 + 3 + 3
    lib = ctypes.CDLL(rg.LIB_PATH)
    for name in NEW_NAMES:
        assert hasattr(lib, name) and name in E.SYMBOLS, name
    rs = open(os.path.join(ROOT, "bindings", "raftgroups_transfer.rs")).read()
    assert rs == gen_rust_bindings.generate_transfer()
    for path, gen in (("raftgroups.rs", gen_rust_bindings.generate), ("raftgroups_lead.rs", gen_rust_bindings.generate_lead), ("raftgroups_term.rs", gen_rust_bindings.generate_term),
                      ("raftgroups_vote.rs", gen_rust_bindings.generate_vote), ("raftgroups_handoff.rs", gen_rust_bindings.generate_handoff),
                      ("raftgroups_conf.rs", gen_rust_bindings.generate_conf)):
        assert open(os.path.join(ROOT, "bindings", path)).read() == gen(), path
    rust = {m.group(1): m.group(2) for m in re.finditer(r"pub fn (rgm_\w+)\((.*?)\)(?: -> [^;]+)?;", rs)}
    assert set(rust) == declared
    for name in declared:
        c_args = [x for x in re.search(r"\b" + name + r"\s*\(([^()]*)\)\s*;", plain, flags=re.S).group(1).split(",") if x.strip() and x.strip() != "void"]
        assert len(c_args) == len([x for x in rust[name].split(",") if x.strip()]) == len(E.SYMBOLS[name][1]), name
    for needle in ("pub struct RgmTransferRec", "pub struct RgmTransferResp", "pub struct RgmTransferOut", "pub items: *mut RgSendItem", "pub count: *mut u32",
                   "pub const RGM_TRANSFER_VERSION: u32 = 1;", "pub const RGM_XFER_FAULT: u32 = 7;", "host_recs: *const RgmTransferRec", "dev_out: *const RgmTransferOut",
                   "use super::raftgroups::*;"):
        assert needle in rs, needle
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_bindings.py"), "--check"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lib.rgm_transfer_version.restype = ctypes.c_uint32
    assert lib.rgm_transfer_version() == int(re.search(r"#define RGM_TRANSFER_VERSION (\d+)u", hdr).group(1)) == E.TRANSFER_VERSION
    assert [f for f, _ in E.TransferOut._fields_] == list(E.TRANSFER_OUT_FIELDS) and ctypes.sizeof(E.TransferOut) == 40
    assert E.TRANSFER_REC_DTYPE.itemsize == 16 and E.TRANSFER_RESP_DTYPE.itemsize == 32 and E.TRANSFER_RESP_DTYPE.itemsize % 8 == 0
    assert [E.TRANSFER_RESP_DTYPE.fields[k][1] for k in ("last_index", "matched", "cfg", "n_items", "status", "events", "previous", "reserved")] == [0, 8, 16, 20, 24, 25, 26, 27]
    for k in ("NONE", "STARTED", "SELF", "IN_PROGRESS", "LEARNER", "NO_PROGRESS", "NOT_LED", "FAULT"):
        assert getattr(E, "XFER_" + k) == getattr(M, k) == int(re.search(r"#define RGM_XFER_%s (\d+)u" % k, hdr).group(1))
    for k in ("TIMEOUT_NOW", "APPEND", "ABORTED_PREVIOUS"):
        assert getattr(E, "XFER_EV_" + k) == getattr(M, "EV_" + k) == int(re.search(r"#define RGM_XFER_EV_%s (0x[0-9a-f]+)u" % k, hdr).group(1), 16)
    for method in ("transfer_leader", "transfer_leader_device"):
        assert callable(getattr(E.Engine, method)), method
    assert (E.ABI_VERSION, E.LEAD_VERSION, E.TERM_VERSION, E.VOTE_VERSION, E.HANDOFF_EXT_VERSION, E.CONF_VERSION) == (12, 1, 1, 1, 1, 1)


def test_api_refusals_are_host_checks(rg):
    """What the two calls refuse is decided on the host, before anything is staged or launched: a NULL engine comes back as
    RG_ERR_INVALID_ARG without a device; the state checks and the record walk stand in front of RG_ENTER_STEP (which refuses
    unresolved host hints where every next step does); every int entry point is a function-try-block that ends in RG_ABI_GUARD; the
    arithmetic's header needs no device header; the unit touches none of the engine's send-stage bookkeeping and not the commit
    publication."""
    lib = rg.load_library()
    n = ctypes.c_uint64(7)
    assert lib.rgm_transfer_leader(None, None, 0, None, 0, 0, None, 0, ctypes.byref(n)) == -1 and b"rgm_transfer_leader" in lib.rg_last_error()
    assert lib.rgm_transfer_leader_device(None, None, 0, 0, None) == -1 and b"rgm_transfer_leader_device" in lib.rg_last_error()
    csrc = os.path.join(ROOT, "raft_rs_amd", "csrc")
    src = open(os.path.join(csrc, "ext_transfer.hip")).read()
    for fn, needles in (("rgm_transfer_leader", ("rgm_transfer_state", "q.group >= h->G", "q.reserved", "q.slot >= h->P", "rg_named_once", "item_cap && !host_items", "!n_items")),
                        ("rgm_transfer_leader_device", ("rgm_transfer_state", "!dev_out->status", "dev_out->item_cap && !dev_out->items", "!dev_to", "!dev_out->count"))):
        body = src[src.index('extern "C" int %s(' % fn):]
        body = body[:body.index("} RG_ABI_GUARD")]
        assert ") try {" in body[:700], fn
        enter = body.index("RG_ENTER_STEP(h")
        assert "RG_ENTER(h)" not in body
        for needle in needles:
            assert 0 <= body.find(needle) < enter, (fn, needle)
        for later in ("rg_stage_reserve", "hipMemsetAsync", "RGM_LAUNCH", "rg_follow_round_trip", "host_cfg_valid = false", "h->host_cfg["):
            assert body.find(later) == -1 or body.find(later) > enter, (fn, later)
    state = src[src.index("static int rgm_transfer_state"):src.index("// One launch of kernel")]
    for needle in ("unknown flags", "flags & ~RG_SEND_BYTES", "h->host_mirror", "!h->esz", "h->send_ready", "h->ingested_upper", "RG_ERR_STATE", "RG_ERR_INVALID_ARG", "!h->ins_arena"):
        assert needle in state, needle
    dense = src[src.index('extern "C" int rgm_transfer_leader_device('):]
    assert "h->host_cfg_valid = false" in dense
    for unit in ("send_items", "send_cols", "send_last_dense", "stage_max_entries", "stage_flags", "send_counter", "rg_list_stage_ran", "send_bound", "local_lost", "cls_stale"):
        assert unit not in src, unit  # the engine's send-stage bookkeeping, the commit publication and the size classes are not this unit's
    assert "h->send_ready = " not in src
    assert src.count("#pragma GCC visibility push(default)") == 1 and src.index("visibility push") < src.index('#include "../../include/raftgroups_transfer.h"') < src.index("visibility pop")
    kernels = open(os.path.join(csrc, "rg_kernels_transfer.h")).read()
    code = re.sub(r"//.*", "", kernels)
    assert "__restrict__" not in code and code.count("atomicAdd(") == 1 and "__syncthreads_or(" in code and "rg_wld<" in code and "rg_wst<" in code
    assert code.count("template <int P, typename IX>") == 3 and "rg_conf_send_peer(" in code and "__launch_bounds__(256)" in code
    assert "for (int s" not in code  # a lane loads the transferee's slot, never the row
    header = open(os.path.join(csrc, "rg_transfer.h")).read()
    assert '#include "rg_conf.h"' in header and "hip" not in re.sub(r"//.*", "", header).lower()
    assert "rg_conf_send_peer" not in re.sub(r"//.*", "", header)  # reused, not restated
    build = open(os.path.join(ROOT, "raft_rs_amd", "build.py")).read()
    assert '"ext_transfer.hip"' in build and '"rg_transfer.h"' in build and '"rg_kernels_transfer.h"' in build and "raftgroups_transfer.h" in build
    old = open(os.path.join(csrc, "abi_state.hip")).read()
    assert 'extern "C" int rg_set_config(rg_engine *h, uint64_t group, uint32_t cfg_word) try {' in old  # (the old road stays)


def test_no_instantiation_carries_scratch():
    """tools/kernel_resources.py over ext_transfer.hip: exactly k_transfer_list and k_transfer_dense, every slot count x both index
    widths, no scratch (the resource metadata of the code objects; the instruction text is not searched)."""
    if not os.path.exists(shutil.which("hipcc") or "/opt/rocm/bin/hipcc"):
        pytest.fail("hipcc is needed (the engine is built with it)")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--src=raft_rs_amd/csrc/ext_transfer.hip"], cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines()[1:]:
        m = re.match(r"(\S.*?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)$", line)
        if m:
            rows[m.group(1)] = (int(m.group(2)), int(m.group(5)), int(m.group(6)))
    want = sorted("%s<%d, %s>" % (k, p, ix) for k in ("k_transfer_list", "k_transfer_dense") for p in range(1, 9) for ix in ("unsigned int", "unsigned long"))
    assert sorted(rows) == want, (sorted(rows), out.stderr[-1000:])
    for k, (vgpr, scratch, lds) in rows.items():
        print(k, vgpr, scratch, lds)
        assert scratch == 0 and lds <= 512, (k, vgpr, scratch, lds)
