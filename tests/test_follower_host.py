"""CPU only: the follower half. (1) tests/follower_model.py is pinned with the reference's own tables, committed as data
(tests/golden/follower_log.json from tests/golden/make_follower_golden.py, COMMIT_TO of reference_tables.json and the follower
columns of fast_log_rejection.json); (2) csrc/rg_follow.h -- the arithmetic the kernels run -- is compiled for the HOST with g++
(tests/host_check/follow_twin.cpp, a stand-alone program) and diffed against the model over seeded random streams, (3) once more
under AddressSanitizer + UBSan; (4) what the streams contain is asserted from the model alone; (5) the two step kernels use no
scratch.

Citations: pingcap/raft-rs v0.6.0."""
import json
import os
import re
import shutil
import subprocess
from concurrent.futures import ProcessPoolExecutor

import pytest

import follower_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = json.load(open(os.path.join(HERE, "golden", "follower_log.json")))
TABLES = json.load(open(os.path.join(HERE, "golden", "reference_tables.json")))
FAST = json.load(open(os.path.join(HERE, "golden", "fast_log_rejection.json")))


def log_of(index_term_pairs, committed=0):
    """A log from [(index, term)] with consecutive indices from 1."""
    assert [i for i, _ in index_term_pairs] == list(range(1, len(index_term_pairs) + 1))
    return M.Log(0, 0, [t for _, t in index_term_pairs], committed)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the model, pinned by the reference's rows
# ---------------------------------------------------------------------------------------------------------------------
def test_model_log_maybe_append_rows():
    """src/raft_log.rs test_log_maybe_append: rows (log_term, index, committed, ents, wlasti, wcommit, wpersist, wpanic) against
    previous_ents with raft_log.committed = commit; new_entry(index, term). `persisted` stays on the host: wpersist is what the
    host derives from the conflict index (min(persisted, conflict - 1), src/raft_log.rs:270-272), checked here the same way.
    The row that panics is a FAULT."""
    t = GOLD["LOG_MAYBE_APPEND"]
    c = t["constants"]
    assert len(t["rows"]) == 16 and sum(r[7] for r in t["rows"]) == 1
    for k, (log_term, index, committed, ents, wlasti, wcommit, wpersist, wpanic) in enumerate(t["rows"]):
        log = log_of(t["previous_ents"], c["commit"])
        assert [i for i, _ in ents] == list(range(index + 1, index + 1 + len(ents))), k
        got = log.maybe_append(index, log_term, committed, [term for _, term in ents])
        assert (got == "panic") == wpanic, (k, got)
        if wpanic:
            assert log.committed == c["commit"] and log.last_index == c["last_index"]  # nothing applied
            continue
        assert (None if got is None else got[1]) == wlasti, (k, got)
        assert log.committed == wcommit, k
        persisted = c["persist"]
        if got is not None and got[0] != 0:
            persisted = min(persisted, got[0] - 1)
        assert persisted == wpersist, k
        if got is not None and ents:
            assert log.terms[log.last_index - len(ents):] == [term for _, term in ents], k


def test_model_find_conflict_rows():
    """src/raft_log.rs test_find_conflict: rows (ents, wconflict)."""
    t = GOLD["FIND_CONFLICT"]
    assert len(t["rows"]) == 12
    for k, (ents, wconflict) in enumerate(t["rows"]):
        assert log_of(t["previous_ents"]).find_conflict(ents) == wconflict, k


def test_model_term_rows():
    """src/raft_log.rs test_term: a snapshot at (offset, 1), then entries (offset + i, term i) for i in 1..num."""
    t = GOLD["TERM"]
    c = t["constants"]
    assert len(t["rows"]) == 5 and t["snapshot"] == ["offset", 1] and t["appended"]["entry"] == ["offset + i", "i"]
    log = M.Log(c["offset"], t["snapshot"][1], list(range(t["appended"]["i_from"], c[t["appended"]["i_below"]])), c["offset"])
    for k, (index, w) in enumerate(t["rows"]):
        assert log.term(index) == (w, w), k
    # ... and the bounded view of that log (99 terms: all but the last 9 runs are gone) hands back exactly the gap
    b = log.copy(bounded=True)
    assert b.known == c["offset"] + c["num"] - 1 - M.TERM_RUNS
    assert b.term(b.known - 1) == (1, c["num"] - 1 - M.TERM_RUNS) and b.term(b.known) == (c["num"] - 1 - M.TERM_RUNS,) * 2


def test_model_handle_msg_append_rows():
    """harness/tests/integration_cases/test_raft.rs test_handle_msg_append: rows (m, w_index, w_commit, w_reject) on the log
    [(1, 1), (2, 2)] (empty_entry(term, index)) with nothing committed."""
    t = GOLD["HANDLE_MSG_APPEND"]
    assert len(t["rows"]) == 11
    for k, (m, w_index, w_commit, w_reject) in enumerate(t["rows"]):
        log = log_of([(i, term) for term, i in t["log"]])
        ents = m["entries"] or []
        assert [i for i, _ in ents] == list(range(m["index"] + 1, m["index"] + 1 + len(ents)))
        r = log.append(m["index"], m["log_term"], m["commit"], [term for _, term in ents])
        assert r[0] in (M.ACCEPT, M.REJECT) and (r[0] == M.REJECT) == w_reject, (k, r)
        assert (log.last_index, log.committed) == (w_index, w_commit), k
        assert r[2] == w_commit, k


def test_model_handle_heartbeat_rows():
    """test_raft.rs test_handle_heartbeat: rows (m, w_commit) on a log of three entries, commit_to(commit) first."""
    t = GOLD["HANDLE_HEARTBEAT"]
    assert len(t["rows"]) == 2
    for k, (m, w_commit) in enumerate(t["rows"]):
        log = log_of([(i, term) for term, i in t["log"]], t["constants"]["commit"])
        r = log.heartbeat(m["commit"])
        assert r == (M.HEARTBEAT, 0, w_commit, 0, 0, 0) and log.committed == w_commit, k


def test_model_commit_to_rows():
    """src/raft_log.rs test_commit_to (reference_tables.json COMMIT_TO): rows (commit, wcommit, wpanic) on previous_ents
    [(1, 1), (2, 2), (3, 3)] with previous_commit = 2 (raft_log.rs:1500-1501), through a heartbeat; the panic is a FAULT."""
    rows = TABLES["COMMIT_TO"]["rows"]
    assert len(rows) == 3
    for k, (commit, wcommit, wpanic) in enumerate(rows):
        log = M.Log(0, 0, [1, 2, 3], 2)
        r = log.heartbeat(commit)
        assert (r[0] == M.FAULT) == wpanic, k
        assert log.committed == (2 if wpanic else wcommit), k


def fast_rejection_probe(row):
    """test_raft.rs test_fast_log_rejection from the follower's side. n1 (leader_log) wins its election and appends its noop;
    the first MsgAppend it sends n2 after the heartbeat response is the probe at next - 1: index = the leader's last index BEFORE
    the noop, log_term = that entry's term, one entry (the noop, in a term above every term of either log). n2 (follower_log,
    nothing committed) answers with reject_hint_index / reject_hint_term."""
    leader = row["leader_log"]
    term, index = leader[-1]
    noop_term = max(t for t, _ in leader + row["follower_log"]) + 1
    return index, term, [noop_term]


def test_model_fast_log_rejection_follower_columns():
    assert len(FAST["rows"]) == 8
    for k, row in enumerate(FAST["rows"]):
        log = log_of([(i, t) for t, i in row["follower_log"]])
        index, log_term, ents = fast_rejection_probe(row)
        r = log.append(index, log_term, 0, ents)
        assert r == (M.REJECT, index, 0, 0, row["reject_hint_index"], row["reject_hint_term"]), (k, r)


# ---------------------------------------------------------------------------------------------------------------------
# 2.-4. the host twin of csrc/rg_follow.h against the model
# ---------------------------------------------------------------------------------------------------------------------
N_FOLLOW = 300  # (stride 512: groups on both sides of a 256 boundary)
GROUPS = [0, 1, 7, 100, 254, 255, 256, 257, 298, 299] + list(range(20, 74))
SEEDS = list(range(1, 11))       # 10 x 20 000 = 200 000 operations, deep histories (tables overflow)
OPS_PER_SEED = 20000
SHALLOW_SEEDS = [101, 102]       # logs of <= 4 runs that (almost) never open a term: at most 8 older runs, so never HOST


def build_twin(tmp_path, name, extra):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build the host twin")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, os.path.join(HERE, "host_check", "follow_twin.cpp"), "-o", exe])
    return exe


def state_text(c):
    return "%d %d %d %d %d%s" % (c["committed"], c["last_index"], c["dummy_index"], c["dummy_term"], len(c["runs"]),
                                 "".join(" %d %d" % r for r in c["runs"]))


def twin_io(events):
    """(stdin of the twin, the stdout the model expects)."""
    lines, expect = ["N %d" % N_FOLLOW], []
    for ev in events:
        if ev[0] == "W":
            lines.append("W %d %s" % (ev[1], state_text(ev[2])))
            expect.append("W 0")
            continue
        _, g, op, r, c = ev
        if op[0] == "H":
            lines.append("H %d %d" % (g, op[1]))
        else:
            rs = M.entry_runs(op[4])
            lines.append("A %d %d %d %d %d%s" % (g, op[1], op[2], op[3], len(rs), "".join(" %d %d" % x for x in rs)))
        expect.append("R %d %d %d %d %d %d" % r)
        lines.append("S %d" % g)
        expect.append("S " + state_text(c))
    return "\n".join(lines) + "\n", expect


def run_stream(args):
    exe, seed, n_ops, max_changes, new_terms = args
    events, kinds, max_runs = M.make_stream(seed, GROUPS, n_ops, max_changes, new_terms)
    text, expect = twin_io(events)
    out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, (seed, out.returncode, out.stderr[-2000:])
    got = out.stdout.split("\n")[:-1]
    assert len(got) == len(expect), (seed, len(got), len(expect))
    for k, (a, b) in enumerate(zip(got, expect)):
        assert a == b, (seed, k, text.split("\n")[k + 1], a, b)
    return n_ops, kinds, max_runs


def check_coverage(kinds, host):
    missing = [k for k in M.KINDS + (("host",) if host else ()) if not kinds.get(k)]
    assert not missing, (missing, kinds)
    if not host:
        assert not kinds.get("host"), kinds


def test_stream_coverage_from_the_model_alone():
    """Every seed the twin and the GPU tests use contains: ACCEPT without a conflict, with a cut log, extending the tail and filing
    a new run, REJECT, STALE, HEARTBEAT, every FAULT kind a step can reach, and HOST; the shallow streams (at most 8 older runs at
    any time) never contain HOST."""
    with ProcessPoolExecutor(max_workers=4) as ex:
        deep = list(ex.map(_kinds_of, [(s, 4000, 12, True) for s in SEEDS]))
        shallow = list(ex.map(_kinds_of, [(s, 4000, 3, False) for s in SHALLOW_SEEDS]))
    for kinds, max_runs in deep:
        check_coverage(kinds, True)
        assert max_runs > M.TERM_RUNS + 1
    for kinds, max_runs in shallow:
        assert max_runs <= M.TERM_RUNS + 1
        check_coverage(kinds, False)


def _kinds_of(args):
    return M.make_stream(args[0], GROUPS, *args[1:])[1:]


def test_host_twin_matches_the_model(tmp_path):
    """>= 200 000 operations: every response and every canonical state, in deep histories (bounded view, HOST included) and in
    shallow ones."""
    exe = build_twin(tmp_path, "follow_twin", [])
    jobs = [(exe, s, OPS_PER_SEED, 12, True) for s in SEEDS] + [(exe, s, 4000, 3, False) for s in SHALLOW_SEEDS]
    with ProcessPoolExecutor(max_workers=4) as ex:
        res = list(ex.map(run_stream, jobs))
    assert sum(n for n, _, _ in res[:len(SEEDS)]) >= 200000
    for _, kinds, _ in res[:len(SEEDS)]:
        check_coverage(kinds, True)
    for _, kinds, max_runs in res[len(SEEDS):]:
        assert max_runs <= M.TERM_RUNS + 1
        check_coverage(kinds, False)


def test_host_twin_refuses_states_that_are_not_canonical(tmp_path):
    exe = build_twin(tmp_path, "follow_twin", [])
    good = {"committed": 3, "last_index": 6, "dummy_index": 2, "dummy_term": 1, "runs": [(3, 1), (5, 4)]}
    bad = [dict(good, runs=[(5, 4), (3, 1)]), dict(good, runs=[(3, 4), (5, 1)]), dict(good, runs=[(3, 4), (5, 4)]), dict(good, committed=7),
           dict(good, runs=[(2, 1), (5, 4)]), dict(good, runs=[(3, 0), (5, 4)]), dict(good, runs=[(3, 1), (7, 4)]), dict(good, runs=[]),
           dict(good, committed=1), dict(good, dummy_index=0, runs=[(1, 1)]), dict(good, last_index=2, committed=2), dict(good, last_index=1 << 63)]
    text = "N 4\n" + "".join("W 1 %s\nS 1\n" % state_text(c) for c in [good] + bad + [dict(good, runs=[(4, 1), (5, 4)])])
    out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")[:-1]
    assert out[0] == "W 0" and out[1] == "S " + state_text(good)
    for k in range(len(bad)):
        assert out[2 + 2 * k] != "W 0" and out[3 + 2 * k] == "S " + state_text(good), (k, bad[k], out[2 + 2 * k])  # refused, nothing written
    assert out[-2] == "W 0"  # (run_first[0] > dummy_index + 1 declares a gap: canonical)


def test_host_twin_is_clean_under_asan_and_ubsan(tmp_path):
    """The same program, -fsanitize=address,undefined -fno-sanitize-recover=all, run directly (a stand-alone executable)."""
    exe = build_twin(tmp_path, "follow_twin_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    n, kinds, _ = run_stream((exe, SEEDS[0], 6000, 12, True))
    assert n == 6000
    check_coverage(kinds, True)


# ---------------------------------------------------------------------------------------------------------------------
# 5. resources
# ---------------------------------------------------------------------------------------------------------------------
def test_step_kernels_use_no_scratch():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc is needed (the engine is built with it)")
    cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-c", os.path.join(ROOT, "raft_rs_amd", "csrc", "abi_follow.hip"),
           "-o", os.devnull, "-Wno-pass-failed", "-Rpass-analysis=kernel-resource-usage"]
    err = subprocess.run(cmd, stderr=subprocess.PIPE, stdout=subprocess.PIPE, text=True).stderr
    rows, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
        if not m:
            continue
        txt = m.group(1).strip()
        if txt.startswith("Function Name:"):
            cur = rows.setdefault(txt.split(":", 1)[1].strip(), {})
        elif cur is not None and ":" in txt:
            k, v = txt.split(":", 1)
            cur[k.strip()] = v.strip()
    for name in ("k_follow_dense", "k_follow_list"):
        row = [v for k, v in rows.items() if name in k]
        assert len(row) == 1, (name, sorted(rows), err[-2000:])
        print(name, row[0])
        assert int(row[0]["ScratchSize [bytes/lane]"]) == 0, (name, row[0])
