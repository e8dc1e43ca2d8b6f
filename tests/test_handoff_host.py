"""CPU only: the hand-off between the follower arena and the leader columns. (1) The arithmetic of csrc/rg_handoff.h -- what the
hand-off kernels run -- is compiled for the HOST with g++ (tests/host_check/handoff_twin.cpp, a stand-alone program) and diffed
against tests/handoff_model.py on the edge list and over a seeded random sweep, (2) once more under AddressSanitizer + UBSan, run
directly; (3) what the sweep contains is asserted from the model alone; (4) the dense kernels carry no scratch
(tools/kernel_resources.py); (5) every new name is declared, exported and bound, and the refusals are host checks; (6) on the
cases the GPU tests promote, the model agrees with the oracle's tick over the existing route, cell for cell.

Citations: pingcap/raft-rs v0.6.0."""
import ctypes
import os
import random
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import gate_model as G
import handoff_model as H

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_NAMES = ("rg_follow_promote", "rg_follow_promote_device", "rg_follow_demote", "rg_follow_demote_device")
SWEEP = 6000


def build_twin(tmp_path, name, extra):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build the host twin")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, os.path.join(HERE, "host_check", "handoff_twin.cpp"), "-o", exe])
    return exe


def conf_of(f):
    return H.mask(f.incoming) | H.mask(f.outgoing) << 8 | f.self_slot << 16


def promote_line(f, lead, P, persisted):
    c = f.canonical()
    row = sum(b << (8 * s) for s, b in enumerate(lead["pflags"]))
    return "P %d %d %d %d %d %d%s %d %d %d %d %d %d %d %d %d" % (
        P, c["committed"], c["last_index"], c["dummy_index"], c["dummy_term"], len(c["runs"]), "".join(" %d %d" % r for r in c["runs"]), f.term, f.lead,
        f.self_id, f.role, conf_of(f), lead["cfg"], row, persisted is not None, persisted or 0)


def demote_line(lead):
    return "D %d %d %d %d %d %d %d %s %s" % (lead["commit"], lead["term_lo"], lead["term_hi"], lead["cur_term"], lead["dummy_index"], lead["dummy_term"],
                                           lead["run_count"], " ".join("%d" % x for x in lead["run_first"]), " ".join("%d" % x for x in lead["run_term"]))


def apply_twin(lead, P, persisted, last, words):
    """The stores of rg_handoff_promote_one, from the twin's " L ..." words, on a copy of the lead group."""
    w = [int(x) for x in words]
    d = H.copy_lead(lead)
    d["commit"], d["term_lo"], d["term_hi"], d["cur_term"], d["dummy_index"], d["dummy_term"], d["run_count"] = w[:7]
    d["run_first"], d["run_term"] = w[7:15], w[15:23]
    pf, cfg, present, self_slot, clear_snap, clear_rs, next_all = w[23:30]
    for s in range(8):
        if not present >> s & 1:
            continue
        assert s < P
        own = s == self_slot
        d["match"][s] = persisted if own else 0
        d["next"][s] = persisted + 1 if own else next_all
        if own:
            d["pr_commit"][s] = d["commit"]
        if clear_snap >> s & 1:
            d["pend_snap"][s] = 0
        if clear_rs >> s & 1:
            d["pend_rs"][s] = 0
    d["pflags"] = [pf >> (8 * s) & 0xFF for s in range(P)]
    assert pf >> (8 * P) == sum(b << (8 * s) for s, b in enumerate(lead["pflags"])) >> (8 * P)
    d["cfg"] = cfg
    return d


def edge_cases():
    """(name, Follower, lead, P, persisted): the log shapes x the configurations of the issue's list."""
    out = []
    for name, (c, term) in H.LOG_EDGES.items():
        f = H.Follower(c, term, 7, (0, 1, 2), (), 1)
        lead = H.fresh_lead(3, H.mask((0, 1, 2)) | 1 << 16 | 7 << 24, sentinel=0xEEEE)
        out.append((name, f, lead, 3, None))
    c, term = H.LOG_EDGES["one_run"]
    # self slot 7 of P = 8; joint; learners in PRESENT; TRANSFEREE set; PENDING_CONF (and every other flag) on the own slot; gids
    f = H.Follower(c, term, 9, (5, 6, 7), (4, 5, 7), 7)
    lead = H.fresh_lead(8, H.mask((5, 6, 7)) | H.mask((4, 5, 7)) << 8 | 7 << 16 | 0x80000 | 5 << 20 | H.mask((1, 4, 5, 6, 7)) << 24, sentinel=0xEEEE)
    lead["pflags"] = [0xFF, 0xFF, 0x0F, 0xFF, 0xC2, 0x41, 0x86, 0xFF]
    lead["gid"] = [1, 2, 3, 1, 2, 3, 1, 2]
    out.append(("config", f, lead, 8, c["last_index"]))
    for k, (role, lead_id, self_id) in enumerate(((G.CANDIDATE, 0, 7), (G.FOLLOWER, 8, 7), (G.FOLLOWER, 0, 0))):
        out.append(("not_won%d" % k, H.Follower(c, term, self_id, (0, 1, 2), (), 1, role, lead_id), H.fresh_lead(3, 7 | 1 << 16 | 7 << 24), 3, None))
    for k, cfg in enumerate((7 | 0 << 16 | 7 << 24, 3 | 1 << 16 | 7 << 24, 7 | 4 << 8 | 1 << 16 | 7 << 24, 7 | 1 << 16 | 5 << 24, 7 | 5 << 16 | 0xFF << 24)):
        fc = H.Follower(c, term, 7, (0, 1, 2), (), 5 if k == 4 else 1)
        out.append(("conf%d" % k, fc, H.fresh_lead(3, cfg), 3, None))
    out.append(("not_persisted", H.Follower(c, term, 7, (0, 1, 2), (), 1), H.fresh_lead(3, 7 | 1 << 16 | 7 << 24), 3, c["last_index"] - 1))
    out.append(("term_not_above", H.Follower(c, 3, 7, (0, 1, 2), (), 1), H.fresh_lead(3, 7 | 1 << 16 | 7 << 24), 3, None))
    return out


EXPECT = {"last_2_63_minus_1": H.FAULT, "not_won0": H.NOT_WON, "not_won1": H.NOT_WON, "not_won2": H.NOT_WON, "conf0": H.CONF, "conf1": H.CONF, "conf2": H.CONF,
          "conf3": H.CONF, "conf4": H.CONF, "not_persisted": H.NOT_PERSISTED, "term_not_above": H.FAULT}


def run_cases(exe, cases):
    """Promote every case in the twin and in the model, then demote what the model's lead group holds in both. -> statuses"""
    lines, expect, after = [], [], []
    for name, f, lead, P, persisted in cases:
        lines.append(promote_line(f, lead, P, persisted))
        m = H.copy_lead(lead)
        a = H.promote(f, m, P, persisted)
        if a[0] != H.DONE:
            assert m == lead, name  # the model itself is all-or-nothing
        expect.append(("P", name, a, lead, m, P, f.canonical()["last_index"] if persisted is None else persisted))
        src = m if a[0] == H.DONE else lead
        lines.append(demote_line(src))
        expect.append(("D", name) + H.demote(src))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    got = out.stdout.split("\n")[:-1]
    assert len(got) == len(expect), (len(got), len(expect))
    statuses = []
    for line, e in zip(got, expect):
        w = line.split()
        if e[0] == "P":
            _, name, a, lead, m, P, persisted = e
            assert w[0] == "P" and tuple(int(x) for x in w[1:6]) == a, (name, line, a)
            if a[0] == H.DONE:
                assert w[6] == "L" and apply_twin(lead, P, persisted, 0, w[7:]) == m, (name, line, m)
            else:
                assert len(w) == 6, (name, line)
            statuses.append(("P", a[0]))
        else:
            _, name, a, c = e
            assert w[0] == "D" and tuple(int(x) for x in w[1:5]) == a, (name, line, a)
            if a[0] == H.DONE:
                runs = [int(x) for x in w[11:]]
                got_c = {"committed": int(w[6]), "last_index": int(w[7]), "dummy_index": int(w[8]), "dummy_term": int(w[9]),
                         "runs": list(zip(runs[0::2], runs[1::2]))}
                assert w[5] == "S" and int(w[10]) == len(c["runs"]) and got_c == c, (name, line, c)
            statuses.append(("D", a[0]))
    return statuses


def sweep_cases(seed, n):
    rng = random.Random(seed)
    cases = []
    for k in range(n):
        P = rng.choice((1, 3, 3, 5, 7, 8))
        f, lead, persisted = H.random_case(rng, P)
        if k % 4 == 3:  # ... and a lead group whose own table is what gets demoted when the promotion is refused
            H.random_lead_log(rng, lead)
        cases.append(("sweep%d" % k, f, lead, P, persisted))
    return cases


def test_model_edges():
    """The model alone on the edge list: each refusal is the one the issue names; eight older runs plus the tail drop the oldest
    run, and the demotion reads back a declared gap; promote then demote is the old log plus one entry of term T."""
    for name, f, lead, P, persisted in edge_cases():
        m = H.copy_lead(lead)
        a = H.promote(f, m, P, persisted)
        assert a[0] == EXPECT.get(name, H.DONE), (name, a)
        if a[0] != H.DONE:
            continue
        c = f.canonical()
        (st, term, last, commit), back = H.demote(m)
        assert (st, term, last, commit) == (H.DONE, f.term, c["last_index"] + 1, c["committed"]), name
        want = (list(c["runs"]) + [(c["last_index"] + 1, f.term)])[-H.FOLLOW_RUNS:]
        assert back["runs"] == want and back["dummy_index"] == c["dummy_index"] and back["last_index"] == c["last_index"] + 1, (name, back)
        if name == "eight_older_plus_tail":
            assert back["runs"][0][0] > back["dummy_index"] + 1 and m["run_count"] == H.TERM_RUNS  # the declared gap
        if name == "config":
            assert m["cfg"] >> 20 & 0xF == 0 and m["pflags"] == [0xFF, 0, 0x0F, 0xFF, 0, 0, 0, 0x21] and m["gid"] == lead["gid"]
            assert m["match"][7] == persisted and m["next"][1] == persisted + 1 and m["match"][0] == 0xEEEE and m["pend_snap"][2] == 0xEEEE
            assert m["pend_snap"][5] == 0 and m["pend_rs"][5] == 0xEEEE and m["pend_rs"][6] == 0 and m["pr_commit"][7] == c["committed"]
    assert set(EXPECT) <= {c[0] for c in edge_cases()}


def test_sweep_coverage_from_the_model_alone():
    """The sweep contains every promotion status, demotions of both outcomes, full tables, declared gaps and empty logs."""
    seen, shapes = set(), set()
    for name, f, lead, P, persisted in sweep_cases(11, SWEEP):
        m = H.copy_lead(lead)
        a = H.promote(f, m, P, persisted)
        seen.add(("P", a[0]))
        seen.add(("D", H.demote(m if a[0] == H.DONE else lead)[0][0]))
        c = f.canonical()
        if a[0] == H.DONE:
            shapes.add(("runs", len(c["runs"])))
            shapes.add(("gap", bool(c["runs"]) and c["runs"][0][0] > c["dummy_index"] + 1))
            shapes.add(("joint", bool(f.outgoing)))
            shapes.add(("transferee", bool(lead["cfg"] >> 20 & 0xF)))
    assert seen == {("P", s) for s in (H.DONE, H.NOT_WON, H.CONF, H.NOT_PERSISTED, H.FAULT)} | {("D", H.DONE), ("D", H.FAULT)}, seen
    assert {("runs", 0), ("runs", 1), ("runs", H.TERM_RUNS), ("runs", H.FOLLOW_RUNS), ("gap", True), ("gap", False), ("joint", True), ("joint", False),
            ("transferee", True), ("transferee", False)} <= shapes, shapes


def test_host_twin_matches_the_model(tmp_path):
    """The edge list and a seeded sweep: every answer field, every cell the kernel would store, the canonical log after a demotion."""
    exe = build_twin(tmp_path, "handoff_twin", [])
    st = run_cases(exe, edge_cases())
    assert len(st) == 2 * len(edge_cases())
    for seed in (11, 12):
        st = run_cases(exe, sweep_cases(seed, SWEEP))
        assert len(st) == 2 * SWEEP and {s for k, s in st if k == "P"} == {H.DONE, H.NOT_WON, H.CONF, H.NOT_PERSISTED, H.FAULT}
    out = subprocess.run([exe], input="P 3 5 4 0 0 1 1 1 2 7 7 0 66055 0 0 0 0\n", stdout=subprocess.PIPE, text=True, check=True).stdout
    assert out == "W 3\n"  # (a log that is not canonical never reaches the arithmetic)


def test_host_twin_is_clean_under_asan_and_ubsan(tmp_path):
    """The same program, -fsanitize=address,undefined -fno-sanitize-recover=all, run directly (a stand-alone executable)."""
    exe = build_twin(tmp_path, "handoff_twin_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    run_cases(exe, edge_cases())
    assert len(run_cases(exe, sweep_cases(13, 1500))) == 3000


def test_dense_kernels_carry_no_scratch():
    """tools/kernel_resources.py over abi_handoff.hip: the dense kernels (and the sparse ones) of both index widths use no scratch
    and no LDS."""
    if not os.path.exists(shutil.which("hipcc") or "/opt/rocm/bin/hipcc"):
        pytest.fail("hipcc is needed (the engine is built with it)")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--src=raft_rs_amd/csrc/abi_handoff.hip"], cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines()[1:]:
        m = re.match(r"(\S.*?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)$", line)
        if m:
            rows[m.group(1)] = (int(m.group(5)), int(m.group(6)))
    for name in ("k_handoff_promote_dense", "k_handoff_demote_dense", "k_handoff_promote_list", "k_handoff_demote_list"):
        mine = {k: v for k, v in rows.items() if k.startswith(name + "<")}
        assert sorted(mine) == [name + "<unsigned int>", name + "<unsigned long>"], (name, sorted(rows), out.stderr[-1000:])
        for k, (scratch, lds) in mine.items():
            print(k, scratch, lds)
            assert scratch == 0 and lds == 0, (k, scratch, lds)


def test_every_new_name_is_declared_exported_and_bound(rg):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_bindings
    from raft_rs_amd import engine as E
    hdr = open(os.path.join(ROOT, "include", "raftgroups.h"), encoding="utf-8").read()
    declared = {name for name, _, _ in gen_rust_bindings.parse(hdr)[3]}
    lib = ctypes.CDLL(rg.LIB_PATH)
    for name in NEW_NAMES:
        assert name in declared and hasattr(lib, name) and name in E.SYMBOLS, name
    assert len(declared) == 129 and "129 entry points" in open(os.path.join(ROOT, "README.md")).read()
    for k, v in (("NONE", E.HANDOFF_NONE), ("DONE", E.HANDOFF_DONE), ("NOT_WON", E.HANDOFF_NOT_WON), ("CONF", E.HANDOFF_CONF),
                 ("NOT_PERSISTED", E.HANDOFF_NOT_PERSISTED), ("FAULT", E.HANDOFF_FAULT)):
        assert int(re.search(r"#define RG_HANDOFF_%s (\d+)u" % k, hdr).group(1)) == v == getattr(H, k), k
    assert (E.HANDOFF_REC_DTYPE.names, E.HANDOFF_RESP_DTYPE.names) == (("follow_group", "lead_group", "persisted"), ("term", "last_index", "commit", "status", "out"))
    assert [f for f, _ in E.HandoffOut._fields_] == list(E.HANDOFF_OUT_COLUMNS) and E.ABI_VERSION == 12
    assert E.TERM_RUNS == H.TERM_RUNS and (H.OUT_BECAME_LEADER, H.OUT_APPENDED) == (0x10, 0x8)


def test_api_refusals_are_host_checks():
    """What the four calls refuse is decided on the host, before anything is staged or launched: the state checks, the group
    bounds and the duplicate rules (the record walk the sparse calls of four units share) stand in front of RG_ENTER."""
    csrc = os.path.join(ROOT, "raft_rs_amd", "csrc")
    src = open(os.path.join(csrc, "abi_handoff.hip")).read()
    for fn, needles in (("rg_follow_promote", ("rg_handoff_promote_state", "rg_walk_pairs", "RG_ERR_SLOT_BUSY")),
                        ("rg_follow_promote_device", ("rg_handoff_promote_state", "h->host_mirror", "rg_handoff_out_complete")),
                        ("rg_follow_demote", ("!h->fo", "rg_walk_pairs")),
                        ("rg_follow_demote_device", ("!h->fo", "h->host_mirror", "rg_handoff_out_complete"))):
        body = src[src.index('extern "C" int %s(' % fn):]
        body = body[:body.index("} RG_ABI_GUARD")]
        enter = body.index("RG_ENTER(h)")
        for needle in needles:
            assert 0 <= body.find(needle) < enter, (fn, needle)
    state = src[src.index("static int rg_handoff_promote_state"):src.index("// ... and what a promotion leaves behind")]
    assert "rg_elect_enabled" in state and "h->ins_arena" in state
    shared = open(os.path.join(csrc, "rg_handoff_host.h")).read()
    check = shared[shared.index("static inline int rg_walk_pairs"):shared.index("// The round trip of a sparse call")]
    assert "seen_f.emplace" in check and "seen_l.emplace" in check and "follow_group >= h->fo->cols.n" in check and "lead_group >= h->G" in check
    assert check.index("lead_group >= h->G") < check.index("rule(q, i)") < check.index("seen_f.emplace") < check.index("seen_l.emplace")
    assert "RG_ENTER" not in shared  # (nothing of the shared host half enters the engine: its callers do, behind their checks)
    elect = shared[shared.index("static inline int rg_elect_enabled"):shared.index("static inline bool rg_handoff_out_complete")]
    assert "!h->fo" in elect and "RG_FL_ELECT" in elect and "RG_ERR_STATE" in elect


@pytest.mark.parametrize("P", [3, 8])
def test_model_agrees_with_the_oracle_on_the_existing_route(oracle, P):
    """The cases the GPU tests promote: the reference's own tick -- the log columns loaded as a host loads them today, then
    RG_MF_BECOME_LEADER with m_hint = T -- leaves every column of every group as the model's promotion does, and reports
    RG_OUT_BECAME_LEADER | RG_OUT_APPENDED for exactly the promoted groups."""
    import handoff_rig as R
    cases = H.gpu_cases(P)
    st = R.state_with(H.SHAPES[P], P, 512 if P == 3 else 256, cases)
    want, answers = R.model_state(st, cases)
    after, gout = R.oracle_tick(*R.route_state(st, cases))
    assert not R.diff(want, after), R.diff(want, after)
    for c, a in zip(cases, answers):
        assert int(gout[c.L]) == a[4] == (0x18 if c.expect == H.DONE else 0), (c.name, hex(int(gout[c.L])))
        if a[0] == H.DONE:
            assert (int(after["cur_term"][c.L]), int(after["term_hi"][c.L]), int(after["commit"][c.L])) == a[1:4], c.name
    assert int(np.count_nonzero(gout)) == sum(c.expect == H.DONE for c in cases)
