"""GPU: the follower's term gate, vote step and election clock on the device (rg_follow_step_gated / rg_follow_step_gated_device
/ rg_follow_clock / rg_follow_soft_write / rg_follow_soft_read) against tests/gate_model.py, word for word: every gate answer,
events word, response term and log response, and after every step the canonical log and the soft state of every group.
No test provokes a device fault: every bad argument is refused on the host."""
import json
import os
import random

import numpy as np
import pytest

import follower_model as F
import gate_model as G

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "vote_gate.json")))
SENTINEL = 0xA5A5A5A5A5A5A5A5
SIZES = (1, 63, 64, 65, 255, 256, 257, 513)


def states_array(E, groups, canon):
    a = np.zeros(len(groups), dtype=E.FOLLOW_STATE_DTYPE)
    for k, (g, c) in enumerate(zip(groups, canon)):
        a[k]["group"], a[k]["committed"], a[k]["last_index"] = g, c["committed"], c["last_index"]
        a[k]["dummy_index"], a[k]["dummy_term"], a[k]["n_runs"] = c["dummy_index"], c["dummy_term"], len(c["runs"])
        for j, (first, term) in enumerate(c["runs"]):
            a[k]["run_first"][j], a[k]["run_term"][j] = first, term
    return a


def canon_of(row):
    n = int(row["n_runs"])
    return {"committed": int(row["committed"]), "last_index": int(row["last_index"]), "dummy_index": int(row["dummy_index"]),
            "dummy_term": int(row["dummy_term"]), "runs": [(int(row["run_first"][j]), int(row["run_term"][j])) for j in range(n)]}


def soft_array(E, groups, softs):
    a = np.zeros(len(groups), dtype=E.FOLLOW_SOFT_DTYPE)
    for k, (g, s) in enumerate(zip(groups, softs)):
        a[k]["group"] = g
        (a[k]["term"], a[k]["vote"], a[k]["leader_id"], a[k]["priority"], a[k]["role"], a[k]["election_elapsed"], a[k]["randomized_timeout"],
         a[k]["promotable"]) = s
    return a


def soft_of(row):
    assert not row["reserved"].any()
    return tuple(int(row[k]) for k in ("term", "vote", "leader_id", "priority", "role", "election_elapsed", "randomized_timeout", "promotable"))


def records_arrays(E, recs):
    """[(g, Msg)] -> (FOLLOW_MSG_DTYPE array, FOLLOW_HDR_DTYPE array, FOLLOW_ENT_RUN_DTYPE array)"""
    msgs, hdrs, ext = np.zeros(len(recs), dtype=E.FOLLOW_MSG_DTYPE), np.zeros(len(recs), dtype=E.FOLLOW_HDR_DTYPE), []
    for k, (g, m) in enumerate(recs):
        r, h = msgs[k], hdrs[k]
        r["group"], r["flags"], r["index"], r["log_term"], r["commit"] = g, m.kind, m.index, m.log_term, m.commit
        h["term"], h["from"], h["priority"], h["flags"] = m.term, m.frm, m.priority, E.GATE_FORCE if m.force else 0
        if m.kind == G.APPEND:
            rs = F.entry_runs(m.ents)
            r["ent_term"], r["n_entries"] = rs[0]
            if len(rs) > 1:
                r["ext"] = (len(ext) << 8) | (len(rs) - 1)
                ext += rs[1:]
        else:
            r["ent_term"] = m.commit_term
    e = np.zeros(len(ext), dtype=E.FOLLOW_ENT_RUN_DTYPE)
    for k, (t, c) in enumerate(ext):
        e[k]["term"], e[k]["count"] = t, c
    return msgs, hdrs, e


def device_u64(ptr, n):
    """n u64 words of device memory at an address the library handed out (through the HIP runtime the process has loaded)."""
    import ctypes
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64.so" in line)
    buf = (ctypes.c_uint64 * n)()
    assert ctypes.CDLL(path).hipMemcpy(buf, ctypes.c_void_p(ptr), 8 * n, 2) == 0  # hipMemcpyDeviceToHost
    return list(buf)


def answer(resp, gate):
    return (int(gate["gate"]), int(gate["events"]), int(gate["term"]),
            tuple(int(resp[k]) for k in ("status", "index", "commit", "conflict", "reject_hint", "log_term")))


class Gated:
    """An engine whose leader side is 300 x 3, with a gated follower arena of n groups, and the model of it."""

    def __init__(self, rg, n, cfg, gate=True):
        self.rg, self.E, self.n, self.cfg = rg, rg.engine, n, cfg
        self.eng = rg.Engine(300, 3)
        self.eng.follow_enable(n)
        self.stride = self.eng.follow_stride()
        if gate:
            self.eng.follow_gate_enable(cfg.election_tick, cfg.min_timeout, cfg.max_timeout, cfg.flags, cfg.seed)
        self.nodes = [G.Node(cfg, g) for g in range(n)]

    def close(self):
        self.eng.sync()
        self.eng.close()

    def load(self, g, log=None, soft=None):
        """the model's node g, and the device's group g, from a log and / or a soft tuple"""
        if log is not None:
            self.nodes[g].log = log
            self.eng.follow_write(states_array(self.E, [g], [log.canonical()]))
        if soft is not None:
            self.nodes[g].load(*soft)
            self.eng.follow_soft_write(soft_array(self.E, [g], [soft]))

    def load_many(self, groups, logs, softs):
        for g, log, s in zip(groups, logs, softs):
            self.nodes[g].log = log
            self.nodes[g].load(*s)
        self.eng.follow_write(states_array(self.E, groups, [l.canonical() for l in logs]))
        self.eng.follow_soft_write(soft_array(self.E, groups, softs))

    def read_soft(self):
        return [soft_of(r) for r in self.eng.follow_soft_read(np.arange(self.n, dtype=np.uint64))]

    def read_logs(self):
        return [canon_of(r) for r in self.eng.follow_read(np.arange(self.n, dtype=np.uint64))]

    def check_state(self, what=""):
        soft, logs = self.read_soft(), self.read_logs()
        bad = [(g, soft[g], self.nodes[g].soft()) for g in range(self.n) if soft[g] != self.nodes[g].soft()]
        assert not bad, (what, bad[:4])
        bad = [(g, logs[g], self.nodes[g].log.canonical()) for g in range(self.n) if logs[g] != self.nodes[g].log.canonical()]
        assert not bad, (what, bad[:4])

    def sparse(self, recs):
        msgs, hdrs, ext = records_arrays(self.E, recs)
        resp, gate = self.eng.follow_step_gated(msgs, hdrs, ext)
        return [answer(r, g) for r, g in zip(resp, gate)]

    def model(self, recs):
        return [self.nodes[g].step(m) for g, m in recs]

    def dense(self, recs):
        """recs: [(g, Msg)], at most one per group, no vote kinds -> answers in the order of recs; every output cell the call
        must leave alone is checked against a sentinel."""
        import torch
        E, S = self.E, self.stride
        msgs, hdrs, ext = records_arrays(E, recs)
        cols = {k: np.zeros(S, dtype=np.uint64) for k in ("index", "log_term", "commit", "ent_term", "ext")}
        term, frm = np.zeros(S, dtype=np.uint64), np.zeros(S, dtype=np.uint64)
        flags, n_entries = np.zeros(S, dtype=np.uint8), np.zeros(S, dtype=np.uint32)
        for m, h in zip(msgs, hdrs):
            g = int(m["group"])
            assert flags[g] == 0
            flags[g], n_entries[g], term[g], frm[g] = m["flags"], m["n_entries"], h["term"], h["from"]
            for k in cols:
                cols[k][g] = m[k]
        dev = {k: torch.from_numpy(v.view(np.int64)).cuda() for k, v in cols.items()}
        dev["flags"], dev["n_entries"] = torch.from_numpy(flags).cuda(), torch.from_numpy(n_entries.view(np.int32)).cuda()
        dev["ext_runs"] = torch.from_numpy(np.frombuffer(ext.tobytes() + bytes(16), dtype=np.int64).copy()).cuda()
        dev["n_ext"] = len(ext)
        d_term, d_from = torch.from_numpy(term.view(np.int64)).cuda(), torch.from_numpy(frm.view(np.int64)).cuda()
        out = {k: torch.full((S,), SENTINEL - (1 << 64), dtype=torch.int64, device="cuda")
               for k in ("index", "commit", "conflict", "reject_hint", "log_term", "resp_term")}
        for k in ("status", "gate", "events"):
            out[k] = torch.full((S,), 0x7f, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.eng.follow_step_gated_device(dev, d_term, d_from, out, out["gate"], out["events"], out["resp_term"])
        self.eng.sync()
        o = {k: v.cpu().numpy() for k, v in out.items()}
        o = {k: v.view(np.uint64) if v.dtype == np.int64 else v for k, v in o.items()}
        has = flags != 0
        for k in ("status", "gate", "events"):
            assert (o[k][self.n:] == 0x7f).all() and not o[k][:self.n][~has[:self.n]].any(), k
        for k in ("index", "commit", "conflict", "resp_term"):
            assert (o[k][~has] == SENTINEL).all(), k
        rej = has & (o["status"] == E.FOLLOW_REJECT)
        for k in ("reject_hint", "log_term"):
            assert (o[k][~rej] == SENTINEL).all(), k
        res = []
        for g, _ in recs:
            r = bool(rej[g])
            res.append((int(o["gate"][g]), int(o["events"][g]), int(o["resp_term"][g]),
                        (int(o["status"][g]), int(o["index"][g]), int(o["commit"][g]), int(o["conflict"][g]),
                         int(o["reject_hint"][g]) if r else 0, int(o["log_term"][g]) if r else 0)))
        return res

    def clock(self, cap, sync=True):
        """-> (n appended, the sorted list)"""
        import torch
        hup = torch.full((cap + 2,), SENTINEL - (1 << 64), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        n = self.eng.follow_clock(hup, cap, sync=sync)
        self.eng.sync()
        counts = device_u64(self.eng.follow_clock_counts(), 2)  # the two device words: appended, due
        if sync:
            assert counts[0] == n
        else:
            assert n is None
            n = counts[0]
        assert counts[0] == min(cap, counts[1])
        h = hup.cpu().numpy().view(np.uint64)
        return n, h


def run_cases(rg, cfg, cases):
    """cases: [(log, soft tuple, [Msg ...])], one group each, all records in ONE sparse call (a group's in array order).
    -> per case: (answers, soft after, node). Device == model is asserted for every answer and every cell."""
    f = Gated(rg, len(cases), cfg)
    groups = list(range(len(cases)))
    f.load_many(groups, [c[0].copy(bounded=True) for c in cases], [c[1] for c in cases])
    f.check_state("load")
    recs = [(g, m) for g, c in zip(groups, cases) for m in c[2]]
    # any interleaving of the groups: round-robin over the groups in a shuffled group order, a group's records in their order
    by_group = {}
    for i, (g, _) in enumerate(recs):
        by_group.setdefault(g, []).append(i)
    gs = list(by_group)
    random.Random(7).shuffle(gs)
    seq = []
    while any(by_group.values()):
        for g in gs:
            if by_group[g]:
                seq.append(by_group[g].pop(0))
    sent = [recs[i] for i in seq]
    got = f.sparse(sent)
    want = f.model(sent)
    bad = [(sent[i][0], sent[i][1].key(), got[i], want[i]) for i in range(len(sent)) if got[i] != want[i]]
    assert not bad, bad[:4]
    f.check_state("after")
    soft = f.read_soft()
    f.close()
    out = []
    for g in groups:
        out.append(([got[k] for k in range(len(sent)) if sent[k][0] == g], soft[g], f.nodes[g]))
    return out


def soft(term=1, vote=0, lead=0, priority=0, role=0, elapsed=0, timeout=15, promotable=1):
    return (term, vote, lead, priority, role, elapsed, timeout, promotable)


# ---------------------------------------------------------------------------------------------------------------------
# A. the reference's rows
# ---------------------------------------------------------------------------------------------------------------------
def test_golden_rows_on_the_device(rg):
    cases, want = [], []
    t = GOLD["RECV_MSG_REQUEST_VOTE"]
    c = t["constants"]
    for k, (state, index, log_term, vote_for, w_reject) in enumerate(t["rows"]):
        if k in t["skipped_leader_rows"]:
            continue
        term = max(t["log"][-1][0], log_term)
        cases.append((F.Log(0, 0, [x for x, _ in t["log"]]), soft(term, vote_for, role=state), [G.Msg(G.VOTE, term, c["from"], index=index, log_term=log_term)]))
        want.append((w_reject, term))
    t = GOLD["FOLLOWER_VOTE"]
    for vote, nvote, wreject in t["rows"]:
        cases.append((F.Log(), soft(t["constants"]["hard_state_term"], vote), [G.Msg(G.VOTE, t["constants"]["m_term"], nvote)]))
        want.append((wreject, t["constants"]["m_term"]))
    t = GOLD["VOTER"]
    c = t["constants"]
    unloadable = 0
    for ents, log_term, index, wreject in t["rows"]:
        terms = [x for x, _ in ents]
        if terms != sorted(terms):  # a log whose terms decrease is not canonical: rg_follow_write refuses it (checked below)
            unloadable += 1
            continue
        cases.append((F.Log(0, 0, terms), soft(0), [G.Msg(G.VOTE, c["m_term"], c["from"], index=index, log_term=log_term)]))
        want.append((wreject, c["m_term"]))
    assert unloadable == 1 and len(cases) == 20 + 6 + 8
    t = GOLD["ADVANCE_COMMIT_BY_VOTE"]
    for use_prevote in t["use_prevote"]:  # (PRE_VOTE itself does not change what the recipient of a request does)
        cases.append((F.Log(0, 0, [1, 1, 1], 1), soft(1, 1, 1, promotable=0),
                      [G.Msg(G.PREVOTE if use_prevote else G.VOTE, 2, t["candidate"], index=2, log_term=1, commit=2, commit_term=1)]))
        want.append((True, 1 if use_prevote else 2))
    res = run_cases(rg, G.Config(10), cases)
    for k, ((answers, s, node), (w_reject, w_term)) in enumerate(zip(res, want)):
        gate, ev, resp_term, resp = answers[0]
        assert gate == (G.G_VOTE_REJECT if w_reject else G.G_VOTE_GRANT) and resp_term == w_term, (k, answers)
    for answers, s, node in res[-2:]:
        assert node.log.committed == 2 and answers[0][3][2] == 1 and answers[0][3][5] == 1
    # test_vote_request, the recipient: the append builds the log, then the clock makes the group due within 2 * election_tick - 1
    t = GOLD["VOTE_REQUEST"]
    c = t["constants"]
    f = Gated(rg, len(t["rows"]), G.Config(c["election_tick"], seed=5))
    for g, (ents, wterm) in enumerate(t["rows"]):
        f.load(g, soft=soft(0))
    recs = [(g, G.Msg(G.APPEND, wterm - 1, c["from"], index=c["m_index"], log_term=c["m_log_term"], ents=[x for x, _ in ents])) for g, (ents, wterm) in enumerate(t["rows"])]
    assert f.sparse(recs) == f.model(recs)
    fired = []
    for _ in range(2 * c["election_tick"] - 1):
        n, h = f.clock(4)
        fired += [int(x) for x in h[:n]]
        for node in f.nodes:
            node.tick()
    assert sorted(fired) == [0, 1]
    f.check_state()
    logs = f.read_logs()
    for g, (ents, wterm) in enumerate(t["rows"]):
        assert (f.nodes[g].term + 1, logs[g]["last_index"], logs[g]["runs"][-1][1]) == (wterm, ents[-1][1], ents[-1][0])
    bad = states_array(f.E, [0], [{"committed": 0, "last_index": 2, "dummy_index": 0, "dummy_term": 0, "runs": [(1, 2), (2, 1)]}])
    with pytest.raises(rg.EngineError):
        f.eng.follow_write(bad)
    f.close()


# ---------------------------------------------------------------------------------------------------------------------
# B. dense vs sparse vs model on one random stream
# ---------------------------------------------------------------------------------------------------------------------
def test_dense_sparse_and_model_agree_on_a_random_stream(rg):
    n, rounds = 513, 40
    cfg = G.Config(3, flags=G.CHECK_QUORUM | G.PRE_VOTE, seed=77)
    rng = random.Random(31)
    d, s = Gated(rg, n, cfg), Gated(rg, n, cfg)
    quiet = {g for g in range(n) if g % 17 == 3}  # groups that never get a message
    groups = list(range(n))
    logs = [F.random_log(rng, 12, bounded=True) for _ in groups]
    softs = [G.random_soft(rng, cfg, l) for l in logs]
    for f in (d, s):
        f.load_many(groups, [l.copy() for l in logs], softs)
    cov, hups, gates = {}, 0, set()
    for r in range(rounds):
        todo = [g for g in groups if g not in quiet and rng.random() < 0.6 and not (r % 2 and 256 <= g < 512)]  # odd rounds: a workgroup without a message
        recs = [(g, G.random_msg(rng, d.nodes[g])) for g in todo]
        steps = [x for x in recs if x[1].kind in (G.APPEND, G.HEARTBEAT, G.TOUCH)]
        votes = [x for x in recs if x[1].kind in (G.VOTE, G.PREVOTE)]
        rng.shuffle(recs)
        want = dict(zip([g for g, _ in recs], d.model(recs)))
        assert dict(zip([g for g, _ in recs], s.model(recs))) == want
        got_s = dict(zip([g for g, _ in recs], s.sparse(recs)))
        got_d = dict(zip([g for g, _ in steps], d.dense(steps)))
        got_d.update(zip([g for g, _ in votes], d.sparse(votes)))
        bad = [(g, got_s[g], got_d[g], want[g]) for g in want if not got_s[g] == got_d[g] == want[g]]
        assert not bad, (r, bad[:4])
        for a in want.values():
            gates.add(a[0])
            cov[a[3][0]] = cov.get(a[3][0], 0) + 1
        # the clock, and the hup round trip: the host campaigns and writes role, term and vote back
        due = sorted(g for g in groups if d.nodes[g].tick())
        assert sorted(g for g in groups if s.nodes[g].tick()) == due
        for f in (d, s):
            k, h = f.clock(n)
            assert k == len(due) and sorted(int(x) for x in h[:k]) == due and (h[k:] == SENTINEL).all(), r
        hups += len(due)
        if due:
            w = [(d.nodes[g].term + 1, g + 1000, 0, d.nodes[g].priority, G.CANDIDATE, 0, 0, 1) for g in due]
            for f in (d, s):
                for g, x in zip(due, w):
                    f.nodes[g].load(*x)
                f.eng.follow_soft_write(soft_array(f.E, due, w))
        d.check_state(("dense", r))
        s.check_state(("sparse", r))
    assert gates == {G.G_PASS, G.G_IGNORED, G.G_STALE_LEADER, G.G_PREVOTE_LOW, G.G_VOTE_GRANT, G.G_VOTE_REJECT}
    assert all(cov.get(k) for k in (F.NONE, F.ACCEPT, F.REJECT, F.STALE, F.HEARTBEAT, F.FAULT, F.HOST)) and hups > 100
    final = d.read_logs()
    for g in quiet:  # never stepped: the log they were loaded with; the clock and the hup round trip alone moved their soft cells
        assert final[g] == logs[g].canonical() and d.nodes[g].priority == softs[g][3]
    d.close()
    s.close()


# ---------------------------------------------------------------------------------------------------------------------
# C. the term gate's corners
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, G.CHECK_QUORUM, G.PRE_VOTE, G.CHECK_QUORUM | G.PRE_VOTE])
def test_term_gate_corners(rg, flags):
    cfg = G.Config(10, flags=flags, seed=3)
    cases, meta = [], []
    log = F.Log(0, 0, [1, 2, 2], 1)
    for kind in (G.APPEND, G.HEARTBEAT, G.VOTE, G.PREVOTE, G.TOUCH):
        for rel in (-1, 0, 1):
            for role in (G.FOLLOWER, G.PRE_CANDIDATE, G.CANDIDATE):
                for lead in ((0, 3) if role == G.FOLLOWER else (0,)):
                    m = G.Msg(kind, 5 + rel, 2, index=3, log_term=2, commit=2 if kind in (G.APPEND, G.HEARTBEAT) else 0, ents=[2] if kind == G.APPEND else [])
                    cases.append((log, soft(5, 0, lead, role=role, elapsed=4, timeout=15), [m]))
                    meta.append((kind, rel, role, lead))
    res = run_cases(rg, cfg, cases)
    for g, ((answers, s, node), (kind, rel, role, lead)) in enumerate(zip(res, meta)):
        gate, ev, resp_term, resp = answers[0]
        key = (kind, rel, role, lead, answers[0])
        step_kind = kind in (G.APPEND, G.HEARTBEAT, G.TOUCH)
        if rel < 0:  # a lower term: nothing changes, whatever the answer
            assert s == soft(5, 0, lead, role=role, elapsed=4, timeout=15) and ev == 0 and resp_term == 5, key
            w = G.G_STALE_LEADER if (flags and kind in (G.APPEND, G.HEARTBEAT)) else G.G_PREVOTE_LOW if kind == G.PREVOTE else G.G_IGNORED
            assert gate == w and node.log.committed == 1, key
            continue
        if rel > 0 and not step_kind and (flags & G.CHECK_QUORUM) and lead:  # inside the lease (elapsed 4 < 10)
            assert (gate, ev, resp_term) == (G.G_IGNORED, 0, 5) and s == soft(5, 0, lead, role=role, elapsed=4, timeout=15), key
            continue
        if step_kind:
            assert gate == G.G_PASS and resp_term == 5 + rel and s[:3] == (5 + rel, 0, 2) and s[4:6] == (0, 0), key  # lead = from, Follower, elapsed 0
            assert bool(ev & G.EV_BECAME_FOLLOWER) == (role != 0) and bool(ev & G.EV_LEADER_CHANGED) == (lead != 2), key
            assert bool(ev & G.EV_HARD_STATE) == (rel > 0 or kind != G.TOUCH), key  # (APPEND / HEARTBEAT commit index 2)
            assert s[6] == (G.draw(cfg.seed, g, 5 + rel, 15, 10, 20) if rel > 0 or role != 0 else 15), key  # reset draws a new timeout
            assert resp[0] == {G.APPEND: F.ACCEPT, G.HEARTBEAT: F.HEARTBEAT, G.TOUCH: F.NONE}[kind], key
        elif kind == G.PREVOTE:  # never changes the term, the vote, the clock
            assert s == soft(5, 0, lead, role=role, elapsed=4, timeout=15) and ev == 0, key
            grant = rel > 0 or lead == 0
            assert (gate, resp_term) == ((G.G_VOTE_GRANT, 5 + rel) if grant else (G.G_VOTE_REJECT, 5)), key
        else:
            grant = rel > 0 or lead == 0
            assert gate == (G.G_VOTE_GRANT if grant else G.G_VOTE_REJECT) and resp_term == 5 + rel, key
            assert s[:3] == (5 + rel, 2 if grant else 0, 0 if rel > 0 else lead), key
            assert s[4] == (0 if rel > 0 else role) and bool(ev & G.EV_BECAME_FOLLOWER) == (rel > 0 and role != 0), key
            assert bool(ev & G.EV_HARD_STATE) == grant and bool(ev & G.EV_LEADER_CHANGED) == (rel > 0 and lead != 0), key


def test_lease_edges_and_force(rg):
    """in_lease = CHECK_QUORUM && lead != 0 && election_elapsed < election_tick; FORCE (a leader transfer) overrides it."""
    cfg = G.Config(10, flags=G.CHECK_QUORUM)
    log = F.Log(0, 0, [1, 1], 1)
    cases = []
    for elapsed in (9, 10):
        for kind in (G.VOTE, G.PREVOTE):
            for force in (False, True):
                cases.append((log, soft(3, 0, 7, elapsed=elapsed, timeout=15), [G.Msg(kind, 4, 2, index=2, log_term=1, force=force)]))
    cases.append((log, soft(3, 0, 0, elapsed=0, timeout=15), [G.Msg(G.VOTE, 4, 2, index=2, log_term=1)]))  # no leader: no lease
    res = run_cases(rg, cfg, cases)
    k = 0
    for elapsed in (9, 10):
        for kind in (G.VOTE, G.PREVOTE):
            for force in (False, True):
                (gate, ev, resp_term, resp), = res[k][0]
                if elapsed == 9 and not force:
                    assert (gate, ev, resp_term) == (G.G_IGNORED, 0, 3) and res[k][1] == soft(3, 0, 7, elapsed=9, timeout=15), k
                else:
                    assert (gate, resp_term) == (G.G_VOTE_GRANT, 4), (k, gate)
                    if kind == G.VOTE:
                        assert res[k][1][:3] == (4, 2, 0) and ev == G.EV_HARD_STATE | G.EV_LEADER_CHANGED, k
                    else:
                        assert res[k][1] == soft(3, 0, 7, elapsed=elapsed, timeout=15) and ev == 0, k
                k += 1
    assert res[k][0][0][0] == G.G_VOTE_GRANT


# ---------------------------------------------------------------------------------------------------------------------
# D. votes
# ---------------------------------------------------------------------------------------------------------------------
def test_vote_step(rg):
    cfg = G.Config(10)
    log = F.Log(0, 0, [1, 2, 2, 3], 2)  # last (4, term 3), committed (2, term 2)
    V = lambda **kw: G.Msg(kw.pop("kind", G.VOTE), kw.pop("term", 5), kw.pop("frm", 2), **kw)  # noqa: E731
    up = dict(index=4, log_term=3)
    cases = [
        # can_vote's three arms, and none of them
        (log, soft(5, 2, 0), [V(**up)]),                                # 0: a repeat of the vote already cast
        (log, soft(5, 0, 0), [V(**up)]),                                # 1: no vote, no leader
        (log, soft(5, 7, 9), [V(kind=G.PREVOTE, term=6, **up)]),        # 2: a pre-vote for a future term
        (log, soft(5, 7, 0), [V(**up)]),                                # 3: voted for another
        (log, soft(5, 0, 9), [V(**up)]),                                # 4: there is a leader
        (log, soft(5, 7, 9), [V(kind=G.PREVOTE, **up)]),                # 5: a pre-vote of this term
        # is_up_to_date at equal, lower and higher term / index
        (log, soft(5), [V(index=3, log_term=3)]),                       # 6: equal term, shorter: reject
        (log, soft(5), [V(index=5, log_term=3)]),                       # 7: equal term, longer
        (log, soft(5), [V(index=9, log_term=2)]),                       # 8: lower term, longer: reject
        (log, soft(5), [V(index=1, log_term=4)]),                       # 9: higher term, shorter
        # the priority tie: only at m.index <= last_index
        (log, soft(5, priority=2), [V(priority=1, **up)]),              # 10: m.index == last_index, lower priority: reject
        (log, soft(5, priority=2), [V(priority=1, index=5, log_term=3)]),  # 11: m.index > last_index
        (log, soft(5, priority=2), [V(priority=2, **up)]),              # 12: equal priority
        (log, soft(5, priority=-1), [V(priority=-1, **up)]),            # 13: negative priorities
        # a repeat vote for the same candidate: granted again, nothing new to persist
        (log, soft(5), [V(**up), V(**up), V(frm=3, **up)]),             # 14
        # a pre-vote grant leaves term, vote and clock untouched
        (log, soft(5, 0, 0, elapsed=7, timeout=15), [V(kind=G.PREVOTE, term=6, **up)]),  # 15
        # commit_info before maybe_commit_by_vote; commit-by-vote at committed, committed + 1, last_index, last_index + 1, a wrong term
        (log, soft(5), [V(index=0, log_term=0, commit=2, commit_term=2)]),   # 16
        (log, soft(5), [V(index=0, log_term=0, commit=3, commit_term=2)]),   # 17
        (log, soft(5), [V(index=0, log_term=0, commit=4, commit_term=3)]),   # 18
        (log, soft(5), [V(index=0, log_term=0, commit=5, commit_term=3)]),   # 19
        (log, soft(5), [V(index=0, log_term=0, commit=4, commit_term=2)]),   # 20
        (log, soft(5), [V(index=0, log_term=0, commit=3, commit_term=0)]),   # 21: commit_term 0: not a commit hint
        (log, soft(5, role=G.CANDIDATE), [V(index=0, log_term=0, commit=3, commit_term=2)]),      # 22: a candidate: CONF_CHECK
        (log, soft(5, role=G.PRE_CANDIDATE), [V(kind=G.PREVOTE, index=0, log_term=0, commit=3, commit_term=2)]),  # 23
        (log, soft(5, role=G.CANDIDATE), [V(term=6, index=0, log_term=0, commit=3, commit_term=2)]),  # 24: a follower by then: no CONF_CHECK
        (log, soft(5), [V(commit=4, commit_term=3, **up)]),             # 25: a grant does not commit
        # an empty log: last_term = dummy_term
        (F.Log(7, 4, [], 7), soft(5), [V(index=7, log_term=4)]),        # 26
        (F.Log(7, 4, [], 7), soft(5), [V(index=9, log_term=3)]),        # 27: reject; commit_info = (7, 4)
        (F.Log(), soft(5), [V(index=0, log_term=0)]),                   # 28
    ]
    res = run_cases(rg, cfg, cases)
    gate = [[a[0] for a in r[0]] for r in res]
    GR, RJ = G.G_VOTE_GRANT, G.G_VOTE_REJECT
    assert gate[:6] == [[GR], [GR], [GR], [RJ], [RJ], [RJ]]
    assert gate[6:10] == [[RJ], [GR], [RJ], [GR]]
    assert gate[10:14] == [[RJ], [GR], [GR], [GR]]
    assert gate[14] == [GR, GR, RJ] and [a[1] for a in res[14][0]] == [G.EV_HARD_STATE, 0, 0] and res[14][1][1] == 2
    assert res[0][0][0][1] == 0 and res[0][1][5] == 0  # the repeat: no HARD_STATE, election_elapsed = 0
    assert res[2][1] == soft(5, 7, 9) and res[2][0][0][2] == 6
    assert gate[15] == [GR] and res[15][0][0][1:3] == (0, 6) and res[15][1] == soft(5, 0, 0, elapsed=7, timeout=15)
    for k, committed, ev in ((16, 2, 0), (17, 3, 1), (18, 4, 1), (19, 2, 0), (20, 2, 0), (21, 2, 0), (22, 3, 9), (23, 3, 9), (24, 3, 1 | 2), (25, 2, 1)):
        a = res[k][0][0]
        assert a[0] == (GR if k == 25 else RJ) and res[k][2].log.committed == committed and a[1] == ev, (k, a)
        if k != 25:
            assert a[3] == (F.NONE, 0, 2, 0, 0, 2), (k, a)  # commit_info of BEFORE: (2, term 2)
    assert gate[26:] == [[GR], [RJ], [GR]] and res[27][0][0][3] == (F.NONE, 9, 7, 0, 0, 4)


# ---------------------------------------------------------------------------------------------------------------------
# E. several records of one group in one sparse call
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_records_of_one_group_apply_in_array_order(rg, n):
    """A higher-term vote, then an append from the new leader, then a stale append -- per group, all groups in one call."""
    cfg = G.Config(10, flags=G.PRE_VOTE, seed=n)
    log = F.Log(0, 0, [1, 1], 1)
    chain = [G.Msg(G.VOTE, 3, 2, index=2, log_term=1), G.Msg(G.APPEND, 3, 2, index=2, log_term=1, commit=3, ents=[3]),
             G.Msg(G.APPEND, 2, 9, index=2, log_term=1, commit=3, ents=[2, 2])]
    res = run_cases(rg, cfg, [(log, soft(2, 9, 9, elapsed=5, timeout=15), chain)] * n)
    for answers, s, node in res:
        assert [a[0] for a in answers] == [G.G_VOTE_GRANT, G.G_PASS, G.G_STALE_LEADER]
        assert [a[1] for a in answers] == [G.EV_HARD_STATE | G.EV_LEADER_CHANGED, G.EV_HARD_STATE | G.EV_LEADER_CHANGED, 0]
        assert [a[2] for a in answers] == [3, 3, 3] and answers[1][3] == (F.ACCEPT, 3, 3, 3, 0, 0)
        assert s[:6] == (3, 2, 2, 0, 0, 0) and node.log.canonical()["runs"] == [(1, 1), (3, 3)]
    if n >= 64:
        assert len({s[6] for _, s, _ in res}) > 3  # the timeouts drawn by the reset differ by group


# ---------------------------------------------------------------------------------------------------------------------
# F. gap logs
# ---------------------------------------------------------------------------------------------------------------------
def test_gap_logs_hand_back_and_leave_the_soft_state(rg):
    """A log of 14 terms behind a snapshot at term 1: the bounded view keeps 9 runs; (dummy, known) is the gap. commit_info
    needs term(committed), maybe_commit term(m.commit), an append's match_term term(m.index): inside the gap they hand back
    where the interval [dummy_term, first known term] does not settle them."""
    cfg = G.Config(10)
    deep = F.Log(10, 1, [t for t in range(1, 15) for _ in range(2)], 13, bounded=True)  # entries 11..38, terms 1..14
    assert deep.known == 21 and deep.term(15) == (1, 6)
    before = soft(20, 0, 0, role=G.CANDIDATE, elapsed=5, timeout=15)
    cases = [
        (deep, before, [G.Msg(G.VOTE, 21, 2, index=0, log_term=0)]),                                   # 0: reject needs term(13): HOST
        (deep, before, [G.Msg(G.VOTE, 21, 2, index=38, log_term=14)]),                                 # 1: a grant needs none
        (deep.copy(), before, [G.Msg(G.APPEND, 21, 2, index=15, log_term=3, ents=[3])]),               # 2: match_term in the gap: HOST
        (deep.copy(), before, [G.Msg(G.APPEND, 21, 2, index=22, log_term=7, ents=[9]),                 # 3: decided on known entries: REJECT
                               G.Msg(G.APPEND, 21, 2, index=15, log_term=3, ents=[3]),                 #    HOST, then the group goes on
                               G.Msg(G.HEARTBEAT, 21, 2, commit=30)]),
        (deep.copy(), before, [G.Msg(G.APPEND, 21, 2, index=38, log_term=14, commit=50, ents=[])]),    # 4: FAULT-free accept (commit capped)
        (deep.copy(), before, [G.Msg(G.HEARTBEAT, 21, 2, commit=50), G.Msg(G.TOUCH, 21, 2)]),          # 5: FAULT: undone; then a TOUCH
    ]
    committed_known = F.Log(10, 1, [t for t in range(1, 15) for _ in range(2)], 25, bounded=True)
    cases += [
        (committed_known, before, [G.Msg(G.VOTE, 20, 2, index=0, log_term=0, commit=26, commit_term=8)]),   # 6: all known: commits
        (deep, before, [G.Msg(G.VOTE, 20, 2, index=0, log_term=0, commit=26, commit_term=8)]),              # 7: commit_info in the gap: HOST
    ]
    res = run_cases(rg, cfg, cases)
    st = [[(a[0], a[1], a[2], a[3][0]) for a in r[0]] for r in res]
    assert st[0] == [(G.G_PASS, 0, 20, F.HOST)] and res[0][1] == before
    assert st[1] == [(G.G_VOTE_GRANT, G.EV_HARD_STATE | G.EV_BECAME_FOLLOWER, 21, F.NONE)]
    assert st[2] == [(G.G_PASS, 0, 20, F.HOST)] and res[2][1] == before
    assert [x[3] for x in st[3]] == [F.REJECT, F.HOST, F.HEARTBEAT] and st[3][1][:3] == (G.G_PASS, 0, 21) and res[3][2].log.committed == 30
    assert st[4][0][3] == F.ACCEPT
    assert st[5] == [(G.G_PASS, 0, 20, F.FAULT), (G.G_PASS, G.EV_HARD_STATE | G.EV_BECAME_FOLLOWER | G.EV_LEADER_CHANGED, 21, F.NONE)]
    assert st[6] == [(G.G_VOTE_REJECT, G.EV_HARD_STATE | G.EV_CONF_CHECK, 20, F.NONE)] and res[6][2].log.committed == 26
    assert st[7] == [(G.G_PASS, 0, 20, F.HOST)] and res[7][1] == before


# ---------------------------------------------------------------------------------------------------------------------
# G. the clock
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_clock_against_the_model(rg, n):
    cfg = G.Config(3, seed=n)
    f = Gated(rg, n, cfg)
    rng = random.Random(n)
    groups = list(range(n))
    softs = [soft(1, 0, 0, elapsed=rng.randint(0, 2), timeout=0, promotable=int(g % 5 != 1 or n == 1)) for g in groups]
    f.load_many(groups, [F.Log() for _ in groups], softs)
    assert all(3 <= x.timeout < 6 for x in f.nodes)
    fired_ever = set()
    for call in range(12):
        due = [g for g in groups if f.nodes[g].tick(deliver=False)]
        cap = (n, 0, 1, len(due) - 1, len(due), len(due) + 1)[call % 6] if due else n
        cap = max(cap, 0)
        k, h = f.clock(cap, sync=call % 4 != 3)
        want = min(cap, len(due))
        assert k == int((h != SENTINEL).sum())
        got = [int(x) for x in h[:k]]
        assert k == want and len(set(got)) == k and set(got) <= set(due) and (h[k:] == SENTINEL).all(), (call, cap, k, want)
        for g in got:
            f.nodes[g].elapsed = 0
        fired_ever |= set(got)
        f.check_state(call)  # the due groups that did not fit are still due: not restarted
        if call == 5 and n > 1:  # a step between two clock calls restarts exactly its own group
            g = n // 2
            rec = [(g, G.Msg(G.HEARTBEAT, 1, 2, commit=0))]
            assert f.sparse(rec) == f.model(rec) and f.nodes[g].elapsed == 0
            f.check_state("step")
    assert fired_ever == {g for g in groups if softs[g][7]}  # non-promotable groups never fire, every other did
    f.close()


def test_clock_saturates(rg):
    f = Gated(rg, 65, G.Config(16383, 32000, 32767))
    f.load(0, soft=soft(1, elapsed=32766, timeout=32766, promotable=0))
    f.load(64, soft=soft(1, elapsed=32766, timeout=32000, promotable=1))
    for want in (32767, 32767):
        k, h = f.clock(0)
        assert k == 0
        for node in f.nodes:
            node.tick(deliver=False)
        f.check_state()
        s = f.read_soft()
        assert s[0][5] == want and s[64][5] == want
    k, h = f.clock(8)
    assert k == 1 and int(h[0]) == 64 and f.read_soft()[64][5] == 0 and f.read_soft()[0][5] == 32767
    f.close()


# ---------------------------------------------------------------------------------------------------------------------
# H. draws
# ---------------------------------------------------------------------------------------------------------------------
def test_timeout_draws(rg):
    n = 65536
    cfg = G.Config(10, seed=0xC0FFEE)
    f = Gated(rg, n, cfg)
    E = f.E
    t0 = f.eng.follow_soft_read(np.arange(n, dtype=np.uint64))["randomized_timeout"].astype(np.int64)
    assert t0.tolist() == [G.draw(cfg.seed, g, 0, 0, 10, 20) for g in range(n)]
    assert sorted(set(t0.tolist())) == list(range(10, 20))
    # a reset: a heartbeat of a higher term through the dense form; then a second reset in the SAME term (a candidate steps down)
    import torch
    S = f.stride
    z64 = torch.zeros(S, dtype=torch.int64, device="cuda")
    ones = torch.ones(S, dtype=torch.int64, device="cuda")
    msgs = {"flags": torch.full((S,), E.FOLLOW_MSG_HEARTBEAT, dtype=torch.uint8, device="cuda"), "index": z64, "log_term": z64, "commit": z64,
            "ent_term": z64, "n_entries": torch.zeros(S, dtype=torch.int32, device="cuda")}
    out = {k: torch.zeros(S, dtype=torch.int64, device="cuda") for k in ("index", "commit", "conflict", "reject_hint", "log_term")}
    out["status"] = torch.zeros(S, dtype=torch.uint8, device="cuda")
    gate, events, rterm = torch.zeros(S, dtype=torch.uint8, device="cuda"), torch.zeros(S, dtype=torch.uint8, device="cuda"), torch.zeros(S, dtype=torch.int64, device="cuda")
    m_term, m_from = ones * 4, ones * 2
    torch.cuda.synchronize()
    f.eng.follow_step_gated_device(msgs, m_term, m_from, out, gate, events, rterm)
    f.eng.sync()
    assert (gate.cpu().numpy() == E.GATE_PASS).all() and (rterm.cpu().numpy() == 4).all()
    assert (events.cpu().numpy() == E.GATE_EV_HARD_STATE | E.GATE_EV_LEADER_CHANGED).all()
    s1 = f.eng.follow_soft_read(np.arange(n, dtype=np.uint64))
    t1 = s1["randomized_timeout"].astype(np.int64)
    assert t1.tolist() == [G.draw(cfg.seed, g, 4, int(t0[g]), 10, 20) for g in range(n)]
    assert sorted(set(t1.tolist())) == list(range(10, 20)) and (s1["term"] == 4).all() and (s1["leader_id"] == 2).all()
    w = s1.copy()
    w["role"], w["leader_id"] = E.ROLE_CANDIDATE, 0
    f.eng.follow_soft_write(w)
    f.eng.follow_step_gated_device(msgs, m_term, m_from, out, gate, events, rterm)
    f.eng.sync()
    s2 = f.eng.follow_soft_read(np.arange(n, dtype=np.uint64))
    t2 = s2["randomized_timeout"].astype(np.int64)
    assert t2.tolist() == [G.draw(cfg.seed, g, 4, int(t1[g]), 10, 20) for g in range(n)]
    assert (t2 != t1).sum() > n // 2 and sorted(set(t2.tolist())) == list(range(10, 20)) and (s2["role"] == 0).all()
    assert (events.cpu().numpy() == E.GATE_EV_BECAME_FOLLOWER | E.GATE_EV_LEADER_CHANGED).all()
    f.close()


# ---------------------------------------------------------------------------------------------------------------------
# I. lifecycle
# ---------------------------------------------------------------------------------------------------------------------
def test_lifecycle(rg):
    import torch
    E = rg.engine
    cfg = G.Config(10, seed=1)
    f = Gated(rg, 300, cfg, gate=False)
    eng = f.eng
    one = soft_array(E, [0], [soft(1)])
    rec = records_arrays(E, [(0, G.Msg(G.HEARTBEAT, 1, 2))])
    buf = torch.zeros(f.stride, dtype=torch.int64, device="cuda")
    b8 = torch.zeros(f.stride, dtype=torch.uint8, device="cuda")
    msgs = {"flags": b8, "index": buf, "log_term": buf, "commit": buf, "ent_term": buf, "n_entries": torch.zeros(f.stride, dtype=torch.int32, device="cuda")}
    out = {k: buf.clone() for k in ("index", "commit", "conflict", "reject_hint", "log_term")}
    out["status"] = b8.clone()
    d_gate, d_events, d_term, d_hup = b8.clone(), b8.clone(), buf.clone(), buf.clone()
    calls = [lambda: eng.follow_soft_write(one), lambda: eng.follow_soft_read([0]), lambda: eng.follow_step_gated(*rec),
             lambda: eng.follow_step_gated_device(msgs, buf, buf, out, d_gate, d_events, d_term), lambda: eng.follow_clock(d_hup, 4)]
    for k, call in enumerate(calls):  # before the enable: RG_ERR_STATE
        with pytest.raises(rg.EngineError) as e:
            call()
        assert "rg_follow_gate_enable first" in str(e.value), k
    assert eng.follow_clock_counts() is None
    fresh = rg.Engine(300, 3)
    with pytest.raises(rg.EngineError):  # ... and before rg_follow_enable
        fresh.follow_gate_enable(10)
    fresh.close()
    bytes0 = eng.device_info()["engine_bytes"]
    eng.follow_gate_enable(10, seed=1)
    assert eng.device_info()["engine_bytes"] - bytes0 >= 37 * f.stride
    with pytest.raises(rg.EngineError) as e:
        eng.follow_gate_enable(10, seed=1)
    assert "already enabled" in str(e.value)
    for c in calls:
        c()
    f.nodes[0].load(*soft(1))  # (what the first of them wrote: a later draw chains on the cell's timeout)
    # soft_write's refusals write nothing, not even the good records of the call
    rng = random.Random(5)
    groups = list(range(300))
    logs = [F.random_log(rng, 6, bounded=True) for _ in groups]
    f.load_many(groups, logs, [G.random_soft(rng, cfg, l) for l in logs])
    good = soft(9, 1, 0, elapsed=3, timeout=12)
    for bad_g, bad in ((300, good), (5, soft(9, role=3)), (5, soft(9, lead=2, role=1)), (5, soft(9, timeout=9)), (5, soft(9, timeout=20)),
                       (5, soft(9, elapsed=32768)), (4, good), (5, soft(9, promotable=2))):
        with pytest.raises(rg.EngineError):
            eng.follow_soft_write(soft_array(E, [4, bad_g], [good, bad]))
        f.check_state(bad)
    for bad_rec in ((300, G.Msg(G.HEARTBEAT, 1, 2)), (0, G.Msg(G.HEARTBEAT, 0, 2)), (0, G.Msg(G.HEARTBEAT, 1, 0)), (0, G.Msg(G.APPEND | G.VOTE, 1, 2)),
                    (0, G.Msg(32, 1, 2))):
        with pytest.raises(rg.EngineError):
            eng.follow_step_gated(*records_arrays(E, [(1, G.Msg(G.HEARTBEAT, 50, 2)), bad_rec]))
        f.check_state(bad_rec)
    # the dense form answers FAULT to what the sparse form refuses, and touches nothing
    recs = [(0, G.Msg(G.VOTE, 50, 2)), (1, G.Msg(G.HEARTBEAT, 50, 0)), (2, G.Msg(G.APPEND | G.TOUCH, 50, 2))]
    got = f.dense(recs)
    assert [(a[0], a[1], a[3][0]) for a in got] == [(E.GATE_NONE, 0, F.FAULT)] * 3 and [a[2] for a in got] == [f.nodes[g].term for g in range(3)]
    f.check_state("dense faults")
    # checkpoint -> mutate -> restore
    eng.checkpoint()
    saved = ([x.soft() for x in f.nodes], [x.log.canonical() for x in f.nodes])
    recs = [(g, G.random_msg(rng, f.nodes[g])) for g in groups]
    assert f.sparse(recs) == f.model(recs)
    f.clock(300)
    assert f.read_soft() != saved[0]
    eng.restore()
    assert f.read_soft() == saved[0] and f.read_logs() == saved[1]
    # the ungated step on a gated engine leaves the soft cells bit-identical
    m = np.zeros(300, dtype=E.FOLLOW_MSG_DTYPE)
    m["group"], m["flags"] = groups, E.FOLLOW_MSG_HEARTBEAT
    eng.follow_step(m)
    assert f.read_soft() == saved[0]
    f.close()
