"""GPU: the follower half on the device (rg_follow_step / rg_follow_step_device / rg_follow_write / rg_follow_read) against
tests/follower_model.py, word for word: every response field and, after every round, the canonical state of every group.
The leader side of the engine has another size (300 groups x 3 slots) than any follower arena here, so an index or stride taken
from the wrong side cannot pass. No test provokes a device fault: every bad argument is refused on the host."""
import json
import os
import random

import numpy as np
import pytest

import follower_model as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = 0xA5A5A5A5A5A5A5A5


def states_array(rg, groups, canon):
    a = np.zeros(len(groups), dtype=rg.engine.FOLLOW_STATE_DTYPE)
    for k, (g, c) in enumerate(zip(groups, canon)):
        a[k]["group"], a[k]["committed"], a[k]["last_index"] = g, c["committed"], c["last_index"]
        a[k]["dummy_index"], a[k]["dummy_term"], a[k]["n_runs"] = c["dummy_index"], c["dummy_term"], len(c["runs"])
        for j, (first, term) in enumerate(c["runs"]):
            a[k]["run_first"][j], a[k]["run_term"][j] = first, term
    return a


def canon_of(row):
    n = int(row["n_runs"])
    assert not row["run_first"][n:].any() and not row["run_term"][n:].any() and int(row["reserved"]) == 0
    return {"committed": int(row["committed"]), "last_index": int(row["last_index"]), "dummy_index": int(row["dummy_index"]),
            "dummy_term": int(row["dummy_term"]), "runs": [(int(row["run_first"][j]), int(row["run_term"][j])) for j in range(n)]}


def records_arrays(rg, recs):
    """[(g, op)] -> (FOLLOW_MSG_DTYPE array, FOLLOW_ENT_RUN_DTYPE array of the further entry runs)"""
    E = rg.engine
    msgs = np.zeros(len(recs), dtype=E.FOLLOW_MSG_DTYPE)
    ext = []
    for k, (g, op) in enumerate(recs):
        m = msgs[k]
        m["group"] = g
        if op[0] == "H":
            m["flags"], m["commit"] = E.FOLLOW_MSG_HEARTBEAT, op[1]
            continue
        rs = M.entry_runs(op[4])
        m["flags"], m["index"], m["log_term"], m["commit"] = E.FOLLOW_MSG_APPEND, op[1], op[2], op[3]
        m["ent_term"], m["n_entries"] = rs[0]
        if len(rs) > 1:
            m["ext"] = (len(ext) << 8) | (len(rs) - 1)
            ext += rs[1:]
    e = np.zeros(len(ext), dtype=E.FOLLOW_ENT_RUN_DTYPE)
    for k, (t, c) in enumerate(ext):
        e[k]["term"], e[k]["count"] = t, c
    return msgs, e


def resp_tuple(r):
    return tuple(int(r[k]) for k in ("status", "index", "commit", "conflict", "reject_hint", "log_term"))


class Follower:
    """An engine whose leader side is 300 x 3, with a follower arena of n groups."""

    def __init__(self, rg, n, eng=None):
        self.rg, self.n = rg, n
        self.eng = eng or rg.Engine(300, 3)
        self.eng.follow_enable(n)
        self.stride = self.eng.follow_stride()
        assert self.stride == (n + 255) // 256 * 256

    def close(self):
        self.eng.sync()
        self.eng.close()

    def write(self, groups, canon):
        self.eng.follow_write(states_array(self.rg, groups, canon))

    def read_all(self):
        return [canon_of(r) for r in self.eng.follow_read(np.arange(self.n, dtype=np.uint64))]

    def sparse(self, recs):
        """recs: [(g, op)] -> response tuples, positional"""
        msgs, ext = records_arrays(self.rg, recs)
        return [resp_tuple(r) for r in self.eng.follow_step(msgs, ext)]

    def dense(self, recs, with_ext=True, zero_ext=False):
        """recs: [(g, op)], at most one per group -> {g: response tuple}; every column cell the call must leave alone is
        checked against a sentinel."""
        import torch
        E, F = self.rg.engine, self.stride
        msgs, ext = records_arrays(self.rg, recs)
        cols = {k: np.zeros(F, dtype=np.uint64) for k in ("index", "log_term", "commit", "ent_term", "ext")}
        flags, n_entries = np.zeros(F, dtype=np.uint8), np.zeros(F, dtype=np.uint32)
        for m in msgs:
            g = int(m["group"])
            assert flags[g] == 0
            flags[g], n_entries[g] = m["flags"], m["n_entries"]
            for k in cols:
                cols[k][g] = m[k]
        dev = {k: torch.from_numpy(v.view(np.int64)).cuda() for k, v in cols.items()}
        dev["flags"], dev["n_entries"] = torch.from_numpy(flags).cuda(), torch.from_numpy(n_entries.view(np.int32)).cuda()
        if with_ext:
            dev["ext_runs"] = torch.from_numpy(np.frombuffer(ext.tobytes() + bytes(16), dtype=np.int64).copy()).cuda()
            dev["n_ext"] = len(ext)
        else:
            assert len(ext) == 0
            dev.pop("ext")
        if zero_ext:
            assert len(ext) == 0
        out = {k: torch.full((F,), SENTINEL - (1 << 64), dtype=torch.int64, device="cuda") for k in ("index", "commit", "conflict", "reject_hint", "log_term")}
        out["status"] = torch.full((F,), 0x7f, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.eng.follow_step_device(dev, out)
        self.eng.sync()
        status = out["status"].cpu().numpy()
        o = {k: v.cpu().numpy().view(np.uint64) for k, v in out.items() if k != "status"}
        assert (status[self.n:] == 0x7f).all() and not status[:self.n][flags[:self.n] == 0].any()
        idle = status != 0
        idle[self.n:] = False
        for k in ("index", "commit", "conflict"):
            assert (o[k][~idle] == SENTINEL).all(), k
        rej = status == E.FOLLOW_REJECT
        rej[self.n:] = False
        for k in ("reject_hint", "log_term"):
            assert (o[k][~rej] == SENTINEL).all(), k
        res = {}
        for g, _ in recs:
            r = status[g] == E.FOLLOW_REJECT
            res[g] = (int(status[g]), int(o["index"][g]), int(o["commit"][g]), int(o["conflict"][g]),
                      int(o["reject_hint"][g]) if r else 0, int(o["log_term"][g]) if r else 0)
        return res


def dense_list(f, recs):
    """the dense form's answers in the order of recs"""
    res = f.dense(recs)
    return [res[g] for g, _ in recs]


def log_of(term_index_pairs, committed=0):
    return M.Log(0, 0, [t for t, _ in term_index_pairs], committed)


# ---------------------------------------------------------------------------------------------------------------------
# A. the reference's rows, each as its own group, through both forms
# ---------------------------------------------------------------------------------------------------------------------
def golden_cases():
    gold = json.load(open(os.path.join(HERE, "golden", "follower_log.json")))
    fast = json.load(open(os.path.join(HERE, "golden", "fast_log_rejection.json")))
    tables = json.load(open(os.path.join(HERE, "golden", "reference_tables.json")))
    cases = []  # (log, op)
    t = gold["LOG_MAYBE_APPEND"]
    for log_term, index, committed, ents, *_ in t["rows"]:  # (behind handle_append_entries: index < committed is STALE)
        cases.append((M.Log(0, 0, [term for _, term in t["previous_ents"]], t["constants"]["commit"]), ("A", index, log_term, committed, [term for _, term in ents])))
    t = gold["FIND_CONFLICT"]
    for ents, _ in t["rows"]:
        if ents:
            i0 = ents[0][0]
            cases.append((M.Log(0, 0, [term for _, term in t["previous_ents"]]), ("A", i0 - 1, [0, 1, 2, 3, 0][min(i0 - 1, 4)], 0, [term for _, term in ents])))
    t = gold["HANDLE_MSG_APPEND"]
    for m, *_ in t["rows"]:
        cases.append((log_of(t["log"]), ("A", m["index"], m["log_term"], m["commit"], [term for _, term in (m["entries"] or [])])))
    t = gold["HANDLE_HEARTBEAT"]
    for m, _ in t["rows"]:
        cases.append((log_of(t["log"], t["constants"]["commit"]), ("H", m["commit"])))
    for commit, _, _ in tables["COMMIT_TO"]["rows"]:
        cases.append((M.Log(0, 0, [1, 2, 3], 2), ("H", commit)))
    for row in fast["rows"]:  # (the probe of the new leader: tests/test_follower_host.py fast_rejection_probe)
        term, index = row["leader_log"][-1]
        noop = max(t_ for t_, _ in row["leader_log"] + row["follower_log"]) + 1
        cases.append((log_of(row["follower_log"]), ("A", index, term, 0, [noop])))
    t = gold["TERM"]  # a deep log: the reference's 99 terms behind a snapshot, probed at the table's indices
    c = t["constants"]
    for index, w in t["rows"]:
        cases.append((M.Log(c["offset"], 1, list(range(1, c["num"])), c["offset"], bounded=True), ("A", max(index, c["offset"]), w, 0, [])))
    return cases, fast["rows"]


def test_golden_rows_on_the_device(rg):
    cases, fast = golden_cases()
    assert len(cases) == 16 + 10 + 11 + 2 + 3 + 8 + 5
    f = Follower(rg, len(cases))
    groups = list(range(len(cases)))
    for form in ("sparse", "dense"):
        logs = [log.copy(bounded=True) for log, _ in cases]
        f.write(groups, [l.canonical() for l in logs])
        want = [M.step(l, op) for l, (_, op) in zip(logs, cases)]
        recs = [(g, op) for g, (_, op) in zip(groups, cases)]
        got = f.sparse(recs) if form == "sparse" else dense_list(f, recs)
        assert got == want, [(k, cases[k][1], a, b) for k, (a, b) in enumerate(zip(got, want)) if a != b][:5]
        assert f.read_all() == [l.canonical() for l in logs]
        k0 = len(cases) - 5 - 8
        for k, row in enumerate(fast):
            assert got[k0 + k][0] == M.REJECT and got[k0 + k][4:] == (row["reject_hint_index"], row["reject_hint_term"])
        assert sorted({r[0] for r in got}) == [M.ACCEPT, M.REJECT, M.STALE, M.HEARTBEAT, M.FAULT, M.HOST]
    f.close()


# ---------------------------------------------------------------------------------------------------------------------
# B. random rounds against the model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed", [(1, 11), (255, 12), (256, 13), (257, 14), (4101, 15)])
def test_random_rounds(rg, n, seed):
    init, rounds, kinds = M.plan_rounds(n, seed)
    if n >= 255:  # (12 records of one group cannot hold every kind)
        missing = [k for k in M.KINDS + ("host",) if not kinds.get(k)]
        assert not missing, missing
    f = Follower(rg, n)
    f.write(list(range(n)), init)
    assert f.read_all() == init
    assert len(rounds) == 12
    for k, rnd in enumerate(rounds):
        recs = [(g, op) for g, op, _ in rnd["records"]]
        want = [r for _, _, r in rnd["records"]]
        if rnd["form"] == "dense":
            got = dense_list(f, recs)
        else:
            got = f.sparse(recs)
        bad = [(i, recs[i], got[i], want[i]) for i in range(len(recs)) if got[i] != want[i]]
        assert not bad, (k, rnd["form"], bad[:5])
        assert f.read_all() == rnd["states"], (k, rnd["form"])
    f.close()


# ---------------------------------------------------------------------------------------------------------------------
# C. sparse order
# ---------------------------------------------------------------------------------------------------------------------
def test_sparse_records_apply_in_array_order_per_group(rg):
    n = 700
    rng = random.Random(21)
    logs = [M.random_log(rng, 6, bounded=True) for _ in range(n)]
    init = [l.canonical() for l in logs]
    recs = []
    for g in range(n - 1, n - 1 - 600, -1):  # descending group order: every workgroup of the list kernel holds run boundaries
        chain = rng.randint(2, 5) if g % 3 == 0 else 1
        for j in range(chain):
            log = logs[g]
            if chain == 1:
                op = M.random_op(rng, log)
            elif j < chain - 1:  # an append on the tail, then an append on top of it ...
                t = log.term(log.last_index)[1] + (j % 2)
                op = ("A", log.last_index, log.term(log.last_index)[0], log.committed, [t] * rng.randint(1, 3))
            else:                # ... then a heartbeat that commits what they brought
                op = ("H", log.last_index)
            recs.append((g, op, M.step(log, op)))
    assert len({g for g, _, _ in recs}) > 257
    dep = [r for g, op, r in recs if g % 3 == 0]
    assert all(r[0] in (M.ACCEPT, M.HEARTBEAT) for r in dep) and sum(r[0] == M.HEARTBEAT and r[2] > 0 for r in dep) >= 150
    f = Follower(rg, n)
    f.write(list(range(n)), init)
    got = f.sparse([(g, op) for g, op, _ in recs])
    assert got == [r for _, _, r in recs]
    final = f.read_all()
    assert final == [l.canonical() for l in logs]
    f.write(list(range(n)), init)  # ... and the same records, one call each
    one = [f.sparse([(g, op)])[0] for g, op, _ in recs]
    assert one == got and f.read_all() == final
    f.close()


# ---------------------------------------------------------------------------------------------------------------------
# D. entry runs
# ---------------------------------------------------------------------------------------------------------------------
def test_entry_runs_through_the_side_array(rg):
    n = 300
    rng = random.Random(31)
    f = Follower(rg, n)
    for form in ("sparse", "dense"):
        logs = [M.random_log(rng, 5, bounded=True) for _ in range(n)]
        f.write(list(range(n)), [l.canonical() for l in logs])
        recs, seen = [], set()
        for g in range(n):
            log = logs[g]
            index = rng.randint(log.committed, log.last_index)
            ents, t = [], log.term(index)[1]
            for i in range(index + 1, index + 1 + rng.randint(1, 9)):
                t = log.term(i)[0] if (i <= log.last_index and rng.random() < 0.7) else t + rng.choice((0, 0, 1, 1, 2)) - (rng.random() < 0.03)
                ents.append(max(t, 0))
            op = ("A", index, log.term(index)[0], rng.randint(0, index + len(ents)), ents)
            seen.add(min(len(M.entry_runs(ents)), 4))
            recs.append((g, op, M.step(log, op)))
        assert seen == {1, 2, 3, 4}
        got = f.sparse([(g, op) for g, op, _ in recs]) if form == "sparse" else dense_list(f, [(g, op) for g, op, _ in recs])
        assert got == [r for _, _, r in recs]
        assert f.read_all() == [l.canonical() for l in logs]
    # a single-term stream: ext = NULL and an all-zero ext column give the same
    logs = [M.random_log(rng, 5, bounded=True) for _ in range(n)]
    init = [l.canonical() for l in logs]
    recs = []
    for g in range(n):
        log = logs[g]
        op = ("A", log.last_index, log.term(log.last_index)[0], log.last_index, [log.term(log.last_index)[1] + (g % 5 == 0)] * rng.randint(0, 8))
        recs.append((g, op, M.step(log, op)))
    res = []
    for with_ext in (False, True):
        f.write(list(range(n)), init)
        r = f.dense([(g, op) for g, op, _ in recs], with_ext=with_ext, zero_ext=True)
        res.append(([r[g] for g in range(n)], f.read_all()))
    assert res[0] == res[1] and res[0][0] == [r for _, _, r in recs] and res[0][1] == [l.canonical() for l in logs]
    f.close()


# ---------------------------------------------------------------------------------------------------------------------
# E. deep histories
# ---------------------------------------------------------------------------------------------------------------------
def deep_log(rng, dummy_index=5, dummy_term=3):
    """12 term changes: 13 runs of 1..3 entries, terms dummy_term + 1, + 2, ..."""
    terms = []
    for k in range(13):
        terms += [dummy_term + 1 + k] * rng.randint(1, 3)
    return M.Log(dummy_index, dummy_term, terms, dummy_index)


def test_deep_histories_hand_back_exactly_the_gap(rg):
    rng = random.Random(41)
    cases = []  # (exact log, op)
    lg = deep_log(rng)
    b = lg.copy(bounded=True)
    assert b.known > lg.dummy_index + 3 and len(b.canonical()["runs"]) == 9
    known_term, last = b.term(b.known)[0], lg.last_index
    special = {
        "stops above the gap": ("A", last, known_term + 2, 0, [99]),
        "through the gap to the dummy entry": ("A", last, lg.dummy_term - 1, 0, [99]),
        "stops inside the gap": ("A", last, lg.dummy_term + 1, 0, [99]),
        "stops at the first gap index it tries": ("A", b.known - 1, known_term + 5, 0, [99]),
        "matches in the gap or not: open": ("A", b.known - 1, lg.dummy_term + 2, 0, []),
        "below the gap's terms: a sure mismatch": ("A", b.known - 2, lg.dummy_term - 2, 0, []),
    }
    for op in special.values():
        cases.append((lg, op))
    for _ in range(250):
        lg = deep_log(rng, rng.choice((0, 5, 50)), rng.choice((1, 3)))
        if lg.dummy_index == 0:
            lg.dummy_term = 0
        lg.committed = lg.dummy_index + rng.randint(0, 6)
        cases.append((lg, M.random_op(rng, lg)))
    n = len(cases)
    f = Follower(rg, n)
    exact = [lg.copy() for lg, _ in cases]
    bound = [lg.copy(bounded=True) for lg, _ in cases]
    f.write(list(range(n)), [l.canonical() for l in bound])
    want_b = [M.step(l, op) for l, (_, op) in zip(bound, cases)]
    want_e = [M.step(l, op) for l, (_, op) in zip(exact, cases)]
    got = f.sparse([(g, op) for g, (_, op) in enumerate(cases)])
    host = {g for g in range(n) if got[g][0] == M.HOST}
    assert host == {g for g in range(n) if want_b[g][0] == M.HOST} and len(host) >= 10
    assert all(got[g] == want_e[g] for g in range(n) if g not in host)
    assert got == want_b and f.read_all() == [l.canonical() for l in bound]
    names = list(special)
    assert [got[k][0] for k in range(len(names))] == [M.REJECT, M.REJECT, M.HOST, M.HOST, M.HOST, M.REJECT], [(names[k], got[k]) for k in range(len(names))]
    assert got[0][4] > b.known and got[1][4:] == (cases[1][0].dummy_index - 1, 0) and got[5][4:] == (cases[5][0].dummy_index - 1, 0)
    # the host compacts its log so that the table is contiguous again: the same messages are all answered
    comp = [lg.copy(bounded=True).compacted().copy(bounded=True) for lg, _ in cases]
    canon = [l.canonical() for l in comp]
    assert all(c["runs"][0][0] == c["dummy_index"] + 1 and len(c["runs"]) <= 9 for c in canon)
    f.write(list(range(n)), canon)
    want = [M.step(l, op) for l, (_, op) in zip(comp, cases)]
    got = dense_list(f, [(g, op) for g, (_, op) in enumerate(cases)])
    assert got == want and not any(r[0] == M.HOST for r in want)
    assert f.read_all() == [l.canonical() for l in comp]
    f.close()


# ---------------------------------------------------------------------------------------------------------------------
# F. faults leave no trace
# ---------------------------------------------------------------------------------------------------------------------
def test_faults_and_hand_backs_leave_no_trace(rg):
    n = 257
    rng = random.Random(51)
    want_kinds = [k for k in M.KINDS if k.startswith("fault_")] + ["host"]
    logs = [M.random_log(rng, 12, bounded=True) for _ in range(n)]
    init = [l.canonical() for l in logs]
    picked = {}  # kind -> [(g, op)]
    for g in [n - 1] * 200 + list(range(n - 2, -1, -1)) * 40:  # (the group behind the 256 boundary first, until it has one)
        if g in {h for v in picked.values() for h, _ in v}:
            continue
        trial = logs[g].copy()
        op = M.random_op(rng, trial)
        M.step(trial, op)
        if trial.kind in want_kinds and len(picked.setdefault(trial.kind, [])) < 4:
            picked[trial.kind].append((g, op))
    assert sorted(picked) == sorted(want_kinds) and any(g == 256 for v in picked.values() for g, _ in v)
    recs = [x for v in picked.values() for x in v]
    f = Follower(rg, n)
    f.write(list(range(n)), init)
    before = f.eng.follow_read(np.arange(n, dtype=np.uint64)).tobytes()
    for form in ("sparse", "dense"):
        got = f.sparse(recs) if form == "sparse" else dense_list(f, recs)
        for (g, op), r in zip(recs, got):
            assert r == M.step(logs[g], op) and r[0] in (M.FAULT, M.HOST)
        assert f.eng.follow_read(np.arange(n, dtype=np.uint64)).tobytes() == before
    # bad arguments: refused on the host, nothing applied
    E = rg.engine
    good = ("A", logs[3].last_index, logs[3].term(logs[3].last_index)[0], 0, [20, 21])
    msgs, ext = records_arrays(rg, [(3, good), (4, ("H", 0))])
    for field, value in (("group", n), ("flags", 3), ("flags", 0), ("ext", (1 << 8) | 1), ("ext", (2 << 8) | 1)):
        bad = msgs.copy()
        bad[1 if field != "ext" else 0][field] = value
        with pytest.raises(rg.EngineError) as ei:
            f.eng.follow_step(bad, ext)
        assert ei.value.code == -1, (field, value)
    with pytest.raises(rg.EngineError) as ei:
        f.eng.follow_write(states_array(rg, [0, n], [init[0], init[0]]))
    assert ei.value.code == -1
    with pytest.raises(rg.EngineError) as ei:
        f.eng.follow_write(states_array(rg, [0], [dict(init[0], committed=init[0]["last_index"] + 1)]))
    assert ei.value.code == -1
    with pytest.raises(rg.EngineError) as ei:
        f.eng.follow_read(np.array([n], dtype=np.uint64))
    assert ei.value.code == -1
    assert f.eng.follow_read(np.arange(n, dtype=np.uint64)).tobytes() == before
    # ... and in one batch the record BEHIND a refused one is applied
    chain = []
    for g, op in recs:
        log = logs[g]
        nxt = ("A", log.last_index, log.term(log.last_index)[0], log.last_index + 1, [log.term(log.last_index)[1] + 1])
        chain += [(g, op, M.step(log, op)), (g, nxt, M.step(log, nxt))]
    got = f.sparse([(g, op) for g, op, _ in chain])
    assert got == [r for _, _, r in chain] and all(r[0] == M.ACCEPT for r in got[1::2])
    assert f.read_all() == [l.canonical() for l in logs]
    f.close()


# ---------------------------------------------------------------------------------------------------------------------
# G. lifetime
# ---------------------------------------------------------------------------------------------------------------------
def test_calls_before_enable_and_a_second_enable_are_state_errors(rg):
    import ctypes as C
    eng = rg.Engine(300, 3)
    L, E = eng.L, rg.engine
    buf = np.zeros(4096, dtype=np.uint64)
    st = np.zeros(1, dtype=E.FOLLOW_STATE_DTYPE)
    msg = np.zeros(1, dtype=E.FOLLOW_MSG_DTYPE)
    msg[0]["flags"] = E.FOLLOW_MSG_HEARTBEAT
    fm, fo = E.FollowMsgs(), E.FollowOut()
    assert L.rg_follow_stride(eng.h) == 0
    calls = {
        "rg_follow_write": lambda: L.rg_follow_write(eng.h, st.ctypes.data, 1),
        "rg_follow_read": lambda: L.rg_follow_read(eng.h, buf.ctypes.data, 1, st.ctypes.data),
        "rg_follow_step": lambda: L.rg_follow_step(eng.h, msg.ctypes.data, 1, None, 0, buf.ctypes.data),
        "rg_follow_step_device": lambda: L.rg_follow_step_device(eng.h, C.byref(fm), C.byref(fo)),  # (refused before a pointer is looked at)
    }
    for name, call in calls.items():
        assert call() == -8, name  # RG_ERR_STATE
        assert name in L.rg_last_error().decode() and "rg_follow_enable" in L.rg_last_error().decode()
    bytes0 = eng.device_info()["engine_bytes"]
    with pytest.raises(rg.EngineError) as ei:
        eng.follow_enable(0)
    assert ei.value.code == -1
    eng.follow_enable(257)
    assert eng.follow_stride() == 512 and eng.device_info()["engine_bytes"] == bytes0 + 512 * 177
    with pytest.raises(rg.EngineError) as ei:
        eng.follow_enable(257)
    assert ei.value.code == -8
    with pytest.raises(rg.EngineError) as ei:  # the dense call's columns: only ext / ext_runs may be NULL
        eng.follow_step_device({}, {})
    assert ei.value.code == -1
    # a fresh arena: empty logs at index 0
    s = eng.follow_read(np.arange(257, dtype=np.uint64))
    assert not any(s[k].any() for k in ("committed", "last_index", "dummy_index", "dummy_term", "n_runs", "run_first", "run_term"))
    eng.close()


def test_checkpoint_restore_round_trip(rg):
    n = 257
    init, rounds, _ = M.plan_rounds(n, 61, rounds=4)
    f = Follower(rg, n)
    f.write(list(range(n)), init)
    for rnd in rounds[:2]:
        f.dense([(g, op) for g, op, _ in rnd["records"]]) if rnd["form"] == "dense" else f.sparse([(g, op) for g, op, _ in rnd["records"]])
    assert f.read_all() == rounds[1]["states"]
    f.eng.checkpoint()
    image = f.eng.follow_read(np.arange(n, dtype=np.uint64)).tobytes()
    for rnd in rounds[2:]:
        f.dense([(g, op) for g, op, _ in rnd["records"]]) if rnd["form"] == "dense" else f.sparse([(g, op) for g, op, _ in rnd["records"]])
    assert f.read_all() == rounds[3]["states"] != rounds[1]["states"]
    f.eng.restore()
    assert f.eng.follow_read(np.arange(n, dtype=np.uint64)).tobytes() == image
    for rnd in rounds[2:]:  # ... and the rounds run again from the image, with the same answers
        recs = [(g, op) for g, op, _ in rnd["records"]]
        got = dense_list(f, recs) if rnd["form"] == "dense" else f.sparse(recs)
        assert got == [r for _, _, r in rnd["records"]]
    assert f.read_all() == rounds[3]["states"]
    f.close()


def test_leader_side_does_not_see_the_arena(rg):
    """300 x 3: dense ticks (four: more than three) with the arena enabled and stepped between them leave every leader-side column bit-identical
    to an engine that never had one."""
    import test_read_index_gpu as RI
    init, rounds, _ = M.plan_rounds(257, 71, rounds=3)
    cols = []
    for with_arena in (False, True):
        r = RI.Rig(rg, 3, depth=1, seed=7, n=300, enable=False)
        f = None
        if with_arena:
            f = Follower(rg, 257, eng=r.eng)
            f.write(list(range(257)), init)
        for k in range(2):
            if f:
                rnd = rounds[k]
                f.dense([(g, op) for g, op, _ in rnd["records"]]) if rnd["form"] == "dense" else f.sparse([(g, op) for g, op, _ in rnd["records"]])
            r.tick_advance(list(range(0, 300, 2 + k)))  # two dense ticks each: the leaders append, their peers ack
        if f:
            assert f.read_all() == rounds[1]["states"]
        cols.append([r.eng.read_column(c).tobytes() for c in range(19)])
        r.close()
    assert cols[0] == cols[1]
