"""GPU: the candidate half on the device (rg_follow_elect_* / rg_follow_campaign / rg_follow_campaign_device /
rg_follow_vote_resps / rg_follow_vote_resps_device) against tests/elect_model.py, word for word: every field of every answer, and
after every call the canonical log, the soft state and the election cells of every group.
No test provokes a device fault: every bad argument is refused on the host, every malformed dense cell is an ANSWER."""
import json
import os

import numpy as np
import pytest

import elect_model as M
import follower_model as F
import gate_model as G
from test_follow_gate_gpu import SENTINEL, SIZES, canon_of, device_u64, records_arrays, soft, soft_array, soft_of, states_array

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "elect.json")))
U8_COLS = ("result", "events", "status", "req_kind", "targets", "flags")
U64_COLS = ("term", "req_term", "req_index", "req_log_term", "req_commit", "req_commit_term")
REQ_COLS = ("req_kind", "targets", "flags", "req_term", "req_index", "req_log_term", "req_commit", "req_commit_term")


def cells_array(E, groups, cells):
    a = np.zeros(len(groups), dtype=E.FOLLOW_ELECT_DTYPE)
    for k, (g, c) in enumerate(zip(groups, cells)):
        a[k]["group"], a[k]["self_id"], a[k]["conf"], a[k]["yes"], a[k]["no"] = (g,) + tuple(c)
    return a


def cells_of(row):
    assert not row["reserved"].any()
    return tuple(int(row[k]) for k in ("self_id", "conf", "yes", "no"))


def answer_of(row):
    return tuple(int(row[k]) for k in M.ANSWER_FIELDS)


class Arena:
    """An engine whose leader side is 300 x 3, with a follower arena of n groups with all three layers."""

    def __init__(self, rg, n, cfg):
        self.rg, self.E, self.n, self.cfg = rg, rg.engine, n, cfg
        self.eng = rg.Engine(300, 3)
        self.eng.follow_enable(n)
        self.stride = self.eng.follow_stride()
        self.eng.follow_gate_enable(cfg.election_tick, cfg.min_timeout, cfg.max_timeout, cfg.flags, cfg.seed)
        self.eng.follow_elect_enable()
        self.all = np.arange(n, dtype=np.uint64)

    def close(self):
        self.eng.sync()
        self.eng.close()

    def load(self, groups, canon=None, softs=None, cells=None):
        if canon is not None:
            self.eng.follow_write(states_array(self.E, groups, canon))
        if softs is not None:
            self.eng.follow_soft_write(soft_array(self.E, groups, softs))
        if cells is not None:
            self.eng.follow_elect_write(cells_array(self.E, groups, cells))

    def load_nodes(self, nodes):
        """the device's groups 0.. from model nodes"""
        gs = list(range(len(nodes)))
        self.load(gs, [nd.log.canonical() for nd in nodes], [nd.soft() for nd in nodes], [nd.cells() for nd in nodes])

    def states(self):
        """[(canonical, soft, cells)] of every group"""
        logs, softs, cells = self.eng.follow_read(self.all), self.eng.follow_soft_read(self.all), self.eng.follow_elect_read(self.all)
        return [(canon_of(a), soft_of(b), cells_of(c)) for a, b, c in zip(logs, softs, cells)]

    def check(self, want, what=""):
        got = self.states()
        bad = [(g, got[g], want[g]) for g in range(self.n) if got[g] != tuple(want[g])]
        assert not bad, (what, bad[:3])

    def check_nodes(self, nodes, what=""):
        self.check([(nd.log.canonical(), nd.soft(), nd.cells()) for nd in nodes], what)

    # ---- the sparse calls ----
    def campaign(self, recs):
        """[(g, Rec of kind HUP / TIMEOUT_NOW)] -> answers"""
        a = np.zeros(len(recs), dtype=self.E.FOLLOW_CAMPAIGN_REQ_DTYPE)
        for k, (g, m) in enumerate(recs):
            a[k]["group"], a[k]["term"], a[k]["from"] = g, m.term, m.frm
            a[k]["flags"] = (self.E.CAMPAIGN_TIMEOUT_NOW if m.kind == M.TIMEOUT_NOW else 0) | (self.E.CAMPAIGN_BLOCKED if m.blocked else 0)
        return [answer_of(r) for r in self.eng.follow_campaign(a)]

    def vote_recs(self, recs):
        a = np.zeros(len(recs), dtype=self.E.FOLLOW_VOTE_REC_DTYPE)
        for k, (g, m) in enumerate(recs):
            a[k]["group"], a[k]["term"], a[k]["commit"], a[k]["commit_term"] = g, m.term, m.commit, m.commit_term
            a[k]["from_slot"], a[k]["kind"], a[k]["reject"] = m.frm, m.kind, m.reject
        return a

    def responses(self, recs):
        """[(g, Rec of kind VOTE / PREVOTE)], several per group allowed -> answers"""
        return [answer_of(r) for r in self.eng.follow_vote_resps(self.vote_recs(recs))]

    # ---- the device forms ----
    def out_columns(self, size):
        import torch
        out = {k: torch.full((size,), 0x7f, dtype=torch.uint8, device="cuda") for k in U8_COLS}
        out.update({k: torch.full((size,), SENTINEL - (1 << 64), dtype=torch.int64, device="cuda") for k in U64_COLS})
        return out

    @staticmethod
    def host_columns(out):
        o = {k: v.cpu().numpy() for k, v in out.items()}
        return {k: v.view(np.uint64) if v.dtype == np.int64 else v for k, v in o.items()}

    @staticmethod
    def answer_at(o, i):
        """the answer at position i; a column the call must leave alone holds its sentinel"""
        req = int(o["result"][i]) == M.REQUESTS
        for k in REQ_COLS:
            assert req or int(o[k][i]) in (0x7f, SENTINEL), (k, i)
        return tuple(int(o[k][i]) if (req or k not in REQ_COLS) else 0 for k in M.ANSWER_FIELDS)

    def dense(self, recs, raw=None):
        """recs: [(g, Rec)], at most one per group -> answers in the order of recs. raw: {g: (kind, slot, reject, term)} cells
        written as they are (malformed ones)."""
        import torch
        S = self.stride
        cols = {k: np.zeros(S, dtype=np.uint8) for k in ("kind", "slot", "reject")}
        cols.update({k: np.zeros(S, dtype=np.uint64) for k in ("term", "commit", "commit_term")})
        for g, m in recs:
            assert cols["kind"][g] == 0
            cols["kind"][g], cols["slot"][g], cols["reject"][g] = m.kind, m.frm, m.reject
            cols["term"][g], cols["commit"][g], cols["commit_term"][g] = m.term, m.commit, m.commit_term
        for g, (kind, slot, reject, term) in (raw or {}).items():
            cols["kind"][g], cols["slot"][g], cols["reject"][g], cols["term"][g] = kind, slot, reject, term
        dev = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).cuda() for k, v in cols.items()}
        out = self.out_columns(S)
        torch.cuda.synchronize()
        self.eng.follow_vote_resps_device(dev, out)
        self.eng.sync()
        o = self.host_columns(out)
        has = cols["kind"] != 0
        for k in ("result", "events", "status"):  # written for every group: 0 where there was no message; nothing beyond n
            assert (o[k][self.n:] == 0x7f).all() and not o[k][:self.n][~has[:self.n]].any(), k
        assert (o["term"][~has] == SENTINEL).all()
        for k in REQ_COLS:
            assert (o[k][~has] == (0x7f if k in U8_COLS else SENTINEL)).all(), k
        self.last_dense = o
        return [self.answer_at(o, g) for g, _ in recs]

    def storm(self, cap, block=None):
        """clock -> campaign_device on the stream, no host sync in between -> (appended, due, the list, {g: answer})"""
        import torch
        hup = torch.full((cap + 2,), SENTINEL - (1 << 64), dtype=torch.int64, device="cuda")
        out = self.out_columns(cap + 2)
        d_block = None
        if block is not None:
            b = np.zeros(self.stride, dtype=np.uint8)
            for g, v in block.items():
                b[g] = 3 if v else 0
            d_block = torch.from_numpy(b).cuda()
        torch.cuda.synchronize()
        assert self.eng.follow_clock(hup, cap, sync=False) is None
        self.eng.follow_campaign_device(hup, self.eng.follow_clock_counts(), cap, out, d_block)
        self.eng.sync()
        appended, due = device_u64(self.eng.follow_clock_counts(), 2)
        assert appended == min(cap, due)
        h = hup.cpu().numpy().view(np.uint64)
        assert (h[appended:] == SENTINEL).all()
        o = self.host_columns(out)
        for k, v in o.items():  # nothing beyond min(*dev_n, cap) is touched
            assert (v[appended:] == (0x7f if k in U8_COLS else SENTINEL)).all(), k
        groups = [int(x) for x in h[:appended]]
        assert len(set(groups)) == len(groups)
        return appended, due, groups, {g: self.answer_at(o, i) for i, g in enumerate(groups)}


def cluster(cfg, size, group, self_id=1, log=None):
    n = M.Node(cfg, group, log, self_id=self_id, incoming=range(size), self_slot=self_id - 1)
    n.promotable = True
    return n


# ---------------------------------------------------------------------------------------------------------------------
# A. the reference's rows
# ---------------------------------------------------------------------------------------------------------------------
def test_golden_rows_on_the_device(rg):
    """test_leader_election_in_one_round_rpc's 13 rows, test_single_node_candidate, test_nonleader_start_election's follower and
    test_candidate_fallback's two messages: one MsgHup each in ONE rg_follow_campaign, then every row's responses in ONE
    rg_follow_vote_resps (a group's in array order), then the fallback appends through rg_follow_step_gated."""
    t = GOLD["LEADER_ELECTION_IN_ONE_ROUND_RPC"]
    cfg = G.Config(t["constants"]["election_tick"], seed=3)
    nodes = [cluster(cfg, size, g) for g, (size, _, _) in enumerate(t["rows"])]
    nodes.append(cluster(cfg, 1, len(nodes)))  # SINGLE_NODE_CANDIDATE
    fb = GOLD["CANDIDATE_FALLBACK"]
    first_fb = len(nodes)
    nodes += [cluster(cfg, len(fb["peers"]), first_fb + k) for k in range(len(fb["messages"]))]
    f = Arena(rg, len(nodes), cfg)
    f.load_nodes(nodes)
    f.check_nodes(nodes, "load")
    hups = [(g, M.Rec(M.HUP)) for g in range(len(nodes))]
    got = f.campaign(hups)
    assert got == [nodes[g].record(m) for g, m in hups]
    f.check_nodes(nodes, "hup")
    assert all(nd.term == 1 for nd in nodes) and got[13][0] == M.WON and got[0][0] == M.WON
    recs = [(g, M.Rec(M.VOTE, term=1, frm=peer - 1, reject=not granted)) for g, (_, votes, _) in enumerate(t["rows"]) for peer, granted in votes]
    got = f.responses(recs)
    assert got == [nodes[g].record(m) for g, m in recs]
    f.check_nodes(nodes, "votes")
    states = f.states()
    for g, (size, votes, state) in enumerate(t["rows"]):
        canon, s, cells = states[g]
        assert s[0] == t["w_term"], g
        if state == 3:
            assert (s[4], s[2]) == (G.FOLLOWER, cells[0]) and cells[2:] == (0, 0), (g, s)  # a Follower of itself: handed to the leader engine
        else:
            assert (s[4], s[2]) == (state, 0), (g, s)
    msgs, hdrs, ext = records_arrays(f.E, [(first_fb + k, G.Msg(G.APPEND, term, frm)) for k, (frm, term) in enumerate(fb["messages"])])
    resp, gate = f.eng.follow_step_gated(msgs, hdrs, ext)
    for k, (frm, term) in enumerate(fb["messages"]):
        nodes[first_fb + k].step(G.Msg(G.APPEND, term, frm))
        assert int(gate[k]["events"]) & f.E.GATE_EV_BECAME_FOLLOWER
    f.check_nodes(nodes, "fallback")
    assert [(nd.role, nd.term) for nd in nodes[first_fb:]] == [(fb["w_role"], term) for _, term in fb["messages"]]
    f.close()


@pytest.mark.parametrize("pre_vote", [False, True])
def test_golden_start_election_through_the_clock(rg, pre_vote):
    """test_nonleader_start_election (a follower and a candidate time out within 2 * election_tick - 1 ticks and campaign at
    term 2 towards the two others) and test_sinle_node_pre_candidate, driven by rg_follow_clock -> rg_follow_campaign_device."""
    t = GOLD["NONLEADER_START_ELECTION"]
    cfg = G.Config(t["election_tick"], flags=G.PRE_VOTE if pre_vote else 0, seed=11)
    nodes = [cluster(cfg, len(t["peers"]), 0), cluster(cfg, len(t["peers"]), 1), cluster(cfg, 1, 2)]
    for nd in nodes:
        nd._events = 0
    nodes[0].become_follower(t["follower_term"], t["follower_lead"])
    nodes[1].become_candidate()
    f = Arena(rg, 3, cfg)
    f.load_nodes(nodes)
    fired = {}
    for _ in range(2 * t["election_tick"] - 1):
        appended, due, groups, answers = f.storm(4)
        want = [g for g, nd in enumerate(nodes) if nd.tick()]
        assert sorted(groups) == want
        for g in want:
            a = nodes[g].record(M.Rec(M.HUP))
            assert answers[g] == a, (g, answers[g], a)
            fired.setdefault(g, []).append(dict(zip(M.ANSWER_FIELDS, a)))
        f.check_nodes(nodes, "tick")
    assert [len(fired[g]) for g in (0, 1)] == [1, 1] and fired[2][0]["result"] == M.WON
    for g in (0, 1):
        a = fired[g][0]
        assert a["result"] == M.REQUESTS and a["targets"] == sum(1 << (p - 1) for p in t["targets"])
        if pre_vote:
            assert (a["req_kind"], a["req_term"], nodes[g].role, nodes[g].term) == (M.PREVOTE, t["request_term"], G.PRE_CANDIDATE, 1)
        else:
            assert (a["req_kind"], a["req_term"], nodes[g].role, nodes[g].term) == (M.VOTE, t["request_term"], t["w_role"], t["w_term"])
    f.close()


# ---------------------------------------------------------------------------------------------------------------------
# B. dense vs sparse vs model on one random stream
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", [M.GPU_PLAN, M.GPU_PLAN_NO_PREVOTE], ids=["prevote", "plain"])
def test_dense_sparse_and_model_agree_on_a_random_stream(rg, plan):
    """Arena d takes the device forms (dense responses, clock -> campaign_device), arena s the sparse ones (rg_follow_vote_resps,
    clock -> rg_follow_campaign); every answer field and, after every round, all three layers of every group against the model's
    plan (whose coverage tests/test_follow_elect_host.py asserts)."""
    n, seed, cfg, n_rounds = plan
    rounds, cov = M.plan_rounds(n, seed, cfg, n_rounds)
    M.check_coverage(cov, cfg)
    d, s = Arena(rg, n, cfg), Arena(rg, n, cfg)
    for r, rd in enumerate(rounds):
        recs = [(g, m) for g, m, _ in rd["records"]]
        want = [a for _, _, a in rd["records"]]
        what = (r, rd["kind"])
        if rd["kind"] == "load":
            gs = [x[0] for x in rd["loads"]]
            for f in (d, s):
                f.load(gs, [x[1] for x in rd["loads"]], [x[2] for x in rd["loads"]], [x[3] for x in rd["loads"]])
        elif rd["kind"] == "responses":
            got_d, got_s = d.dense(recs), s.responses(recs[::-1])[::-1]
            bad = [(g, m.key(), a, b, w) for (g, m), a, b, w in zip(recs, got_d, got_s, want) if not a == b == w]
            assert not bad, (what, bad[:3])
        elif rd["kind"] == "multi":
            for f in (d, s):
                got = f.responses(recs)
                bad = [(g, m.key(), a, w) for (g, m), a, w in zip(recs, got, want) if a != w]
                assert not bad, (what, bad[:3])
        elif rd["kind"] == "campaign":
            for f in (d, s):
                got = f.campaign(recs)
                bad = [(g, m.key(), a, w) for (g, m), a, w in zip(recs, got, want) if a != w]
                assert not bad, (what, bad[:3])
        else:
            appended, due, groups, answers = d.storm(n + 5, rd["blocked"])
            assert (appended, due, sorted(groups)) == (len(rd["due"]), len(rd["due"]), rd["due"]), what
            bad = [(g, answers[g], w) for (g, _), w in zip(recs, want) if answers[g] != w]
            assert not bad, (what, bad[:3])
            assert s.eng.follow_clock(None, 0) == 0  # every group ticks, none is delivered: the hups go the sparse road
            assert s.campaign(recs) == want, what
        d.check(rd["states"], what)
        if rd["kind"] == "storm":  # (the sparse road's MsgHup does not restart the clock: election_elapsed of a due group differs)
            got = s.states()
            due = set(rd["due"])
            for g in range(n):
                w = rd["states"][g]
                if g in due and got[g][1] != w[1]:
                    nd_role = w[1][4]
                    assert got[g][0] == w[0] and got[g][2] == w[2] and got[g][1][:5] == w[1][:5] and got[g][1][6:] == w[1][6:], (what, g, got[g], w)
                    assert nd_role == G.PRE_CANDIDATE or answers[g][0] in (M.IGNORED, M.BLOCKED) or answers[g][11] == F.HOST, (what, g)
                    s.load([g], softs=[w[1]])
                else:
                    assert got[g] == tuple(w), (what, g, got[g], w)
        else:
            s.check(rd["states"], what)
    d.close()
    s.close()


# ---------------------------------------------------------------------------------------------------------------------
# C. the storm path at the kernel's edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_clock_chained_into_the_campaign(rg, n):
    """Nothing due; one group due; every group due with cap below the number due (the undelivered groups neither campaign nor
    restart); the rest with a dev_block column; sentinel-filled output columns untouched beyond min(*dev_n, cap)."""
    import random
    rng = random.Random(n)
    cfg = G.Config(10, 12, 13, flags=G.PRE_VOTE if n % 2 else 0, seed=n)  # every timeout is 12
    nodes = []
    for g in range(n):
        incoming, outgoing, self_slot, _ = M.CONFS[g % len(M.CONFS)]
        nd = M.Node(cfg, g, F.random_log(rng, 3, bounded=True), self_id=200 + g, incoming=incoming, outgoing=outgoing, self_slot=self_slot)
        nd.load(rng.randint(nd.log.terms[-1] if nd.log.terms else 1, 15), 0, rng.choice((0, 7)), 0, G.FOLLOWER, 0, 12, True)
        nodes.append(nd)
    f = Arena(rg, n, cfg)
    f.load_nodes(nodes)

    def tick(cap, block=None, deliver=None):
        appended, due, groups, answers = f.storm(cap, block)
        want_due = [g for g, nd in enumerate(nodes) if nd.tick(deliver=False)]
        assert due == len(want_due) and appended == min(cap, due) and set(groups) <= set(want_due)
        for g in groups:
            nodes[g].elapsed = 0  # delivered: the clock restarts it, then its MsgHup
            a = nodes[g].record(M.Rec(M.HUP, blocked=bool(block and block.get(g))))
            assert answers[g] == a, (g, answers[g], a)
        f.check_nodes(nodes, (cap, due))
        return groups, answers
    assert tick(n + 1) == ([], {})  # nothing due
    one = n // 2
    nodes[one].elapsed = 11
    f.load([one], softs=[nodes[one].soft()])
    groups, answers = tick(n + 1)  # one group due (elapsed 11 + 1 reaches its timeout)
    assert groups == [one] and answers[one][0] in (M.REQUESTS, M.WON)
    for g, nd in enumerate(nodes):
        if g != one:
            nd.elapsed = 11
    f.load(list(range(n)), softs=[nd.soft() for nd in nodes])
    if n > 1:
        cap = (n - 1) // 2
        groups, _ = tick(cap)  # cap below the number due (cap 0: the call launches nothing)
        assert len(groups) == cap
        rest = [g for g in range(n) if g != one and g not in groups]
        assert all(nodes[g].role == G.FOLLOWER and nodes[g].elapsed == 12 for g in rest)
        block = {g: g % 3 == 0 for g in rest}
        groups, answers = tick(n, block)
        assert sorted(groups) == rest
        assert all((answers[g][0] == M.BLOCKED) == (block[g] and nodes[g].lead != nodes[g].self_id) for g in rest)
    f.close()


# ---------------------------------------------------------------------------------------------------------------------
# D. order, hand-backs, the win, the lifecycle
# ---------------------------------------------------------------------------------------------------------------------
def test_several_responses_of_one_group_apply_in_array_order(rg):
    """One sparse call: a pre-vote win followed by the real votes (the first record's answer carries the real requests, the
    second wins); the same two records the other way round (the real vote's later term steps the pre-candidate down, the
    pre-vote grant then finds a follower); a repeated vote with the opposite answer (the first stays); the three groups'
    records interleaved."""
    cfg = G.Config(10, flags=G.PRE_VOTE, seed=5)
    nodes = [cluster(cfg, 3, g, log=F.Log(0, 0, [1, 1], 1)) for g in range(3)]
    f = Arena(rg, 3, cfg)
    for nd in nodes:
        nd.load(1, 0, 0, 0, G.FOLLOWER, 0, 0, True)
    f.load_nodes(nodes)
    hups = [(g, M.Rec(M.HUP)) for g in range(3)]
    assert f.campaign(hups) == [nodes[g].record(m) for g, m in hups]
    assert all(nd.role == G.PRE_CANDIDATE for nd in nodes)
    pre, real = M.Rec(M.PREVOTE, term=2, frm=1), M.Rec(M.VOTE, term=2, frm=1)
    recs = [(0, pre), (1, real), (2, M.Rec(M.PREVOTE, term=1, frm=2, reject=True)), (0, real), (1, pre), (2, M.Rec(M.PREVOTE, term=2, frm=2)),
            (2, M.Rec(M.PREVOTE, term=1, frm=1, reject=True))]
    got = f.responses(recs)
    want = [nodes[g].record(m) for g, m in recs]
    assert got == want
    a = [dict(zip(M.ANSWER_FIELDS, x)) for x in got]
    assert (a[0]["result"], a[0]["req_kind"], a[0]["req_term"], a[0]["term"], a[0]["req_commit"]) == (M.REQUESTS, M.VOTE, 2, 2, 1) and a[3]["result"] == M.WON
    assert (a[1]["result"], a[4]["result"], nodes[1].role, nodes[1].term) == (M.STEPPED_DOWN, M.IGNORED, G.FOLLOWER, 2)
    assert [a[k]["result"] for k in (2, 5, 6)] == [M.PENDING, M.PENDING, M.LOST]  # slot 2's grant came second: its denial stays
    f.check_nodes(nodes)
    f.close()


def test_gap_logs_hand_back_and_leave_all_three_layers_untouched(rg):
    """A log whose table dropped runs, with the commit index in the gap: commit_info needs a term that is not on the device --
    MsgHup is handed back; a reject whose commit info points into the gap is handed back AFTER its vote was recorded and poll
    ran: the vote is undone too. Dense and sparse."""
    cfg = G.Config(10, seed=9)
    terms = [t for t in range(1, 13) for _ in range(2)]
    nodes = []
    for g in range(4):
        log = F.Log(0, 0, terms, 3 if g < 2 else 23, bounded=True)
        assert log.known > 4
        nd = cluster(cfg, 5, g, log=log)
        nd.load(12, nd.self_id if g >= 2 else 0, 0, 0, G.CANDIDATE if g >= 2 else G.FOLLOWER, 0, 0, True)
        if g >= 2:
            nd.load_elect(nd.self_id, M.conf_word(range(5), (), 0), 1, 0)
        nodes.append(nd)
    f = Arena(rg, 4, cfg)
    f.load_nodes(nodes)
    before = f.states()
    hups = [(0, M.Rec(M.HUP)), (1, M.Rec(M.TIMEOUT_NOW, term=14, frm=3))]
    got = f.campaign(hups)
    assert got == [nodes[g].record(m) for g, m in hups] and [a[0] for a in got] == [M.NONE] * 2 and [a[11] for a in got] == [F.HOST] * 2
    assert f.states() == before
    rej = M.Rec(M.VOTE, term=12, frm=2, reject=True, commit=3, commit_term=1)  # commit 3 is in the gap, term(3) in [0, 4]
    assert nodes[2].log.committed == 23
    nodes[2].log.committed = nodes[3].log.committed = 2
    f.load([2, 3], [nodes[2].log.canonical(), nodes[3].log.canonical()])
    before = f.states()
    got = f.responses([(2, rej)]) + f.dense([(3, rej)])
    assert got == [nodes[2].record(rej), nodes[3].record(rej)] and [a[11] for a in got] == [F.HOST] * 2
    assert f.states() == before
    f.check_nodes(nodes)
    ok = M.Rec(M.VOTE, term=12, frm=2, reject=True)  # the same reject without commit info goes through
    assert f.responses([(2, ok)]) == [nodes[2].record(ok)] and nodes[2].votes == {0: True, 2: False}
    f.check_nodes(nodes)
    f.close()


def test_after_a_win_stragglers_are_ignored_and_a_later_leader_is_an_event(rg):
    cfg = G.Config(10, seed=4)
    nodes = [cluster(cfg, 3, 0)]
    f = Arena(rg, 1, cfg)
    f.load_nodes(nodes)
    assert f.campaign([(0, M.Rec(M.HUP))]) == [nodes[0].record(M.Rec(M.HUP))]
    grant = M.Rec(M.VOTE, term=1, frm=1)
    win = f.responses([(0, grant)])
    assert win == [nodes[0].record(grant)] and win[0][0] == M.WON and win[0][1] & G.EV_LEADER_CHANGED and not win[0][1] & G.EV_BECAME_FOLLOWER
    straggler = M.Rec(M.VOTE, term=1, frm=2)
    before = f.states()
    assert f.responses([(0, straggler)]) == [nodes[0].record(straggler)] == [(M.IGNORED, 0, 1) + (0,) * 9]
    assert f.dense([(0, straggler)]) == [(M.IGNORED, 0, 1) + (0,) * 9] and f.states() == before
    assert f.campaign([(0, M.Rec(M.HUP))]) == [(M.IGNORED, 0, 1) + (0,) * 9]  # the hup of a group this store leads
    msgs, hdrs, ext = records_arrays(f.E, [(0, G.Msg(G.APPEND, 2, 3))])
    resp, gate = f.eng.follow_step_gated(msgs, hdrs, ext)
    want = nodes[0].step(G.Msg(G.APPEND, 2, 3))
    assert (int(gate[0]["gate"]), int(gate[0]["events"]), int(gate[0]["term"])) == want[:3]
    assert want[1] & G.EV_LEADER_CHANGED and nodes[0].lead == 3
    f.check_nodes(nodes)
    f.close()


def test_malformed_dense_cells_are_answered_not_applied(rg):
    cfg = G.Config(10, seed=4)
    nodes = [cluster(cfg, 3, g) for g in range(70)]
    f = Arena(rg, 70, cfg)
    f.load_nodes(nodes)
    hups = [(g, M.Rec(M.HUP)) for g in range(70)]
    assert f.campaign(hups) == [nodes[g].record(m) for g, m in hups]
    before = f.states()
    raw = {3: (12, 1, 0, 1), 4: (16, 1, 0, 1), 5: (4, 8, 0, 1), 64: (4, 255, 1, 1), 65: (8, 1, 0, 0), 66: (1, 1, 0, 1)}
    good = [(7, M.Rec(M.VOTE, term=1, frm=1))]
    got = f.dense(good, raw)
    assert got == [nodes[7].record(good[0][1])] and got[0][0] == M.WON
    o = f.last_dense
    for g in raw:
        assert (int(o["result"][g]), int(o["events"][g]), int(o["status"][g]), int(o["term"][g])) == (M.NONE, 0, F.FAULT, 1), g
    after = f.states()
    assert [after[g] for g in range(70) if g != 7] == [before[g] for g in range(70) if g != 7]
    f.check_nodes(nodes)
    f.close()


def test_checkpoint_and_restore_carry_the_election_cells(rg):
    cfg = G.Config(10, flags=G.PRE_VOTE, seed=8)
    nodes = [cluster(cfg, 5, g) for g in range(65)]
    f = Arena(rg, 65, cfg)
    for nd in nodes:
        nd.load(1, 0, 0, 0, G.FOLLOWER, 0, 0, True)
    f.load_nodes(nodes)
    hups = [(g, M.Rec(M.HUP)) for g in range(65)]
    assert f.campaign(hups) == [nodes[g].record(m) for g, m in hups]
    recs = [(g, M.Rec(M.PREVOTE, term=1 if g % 2 == 0 else 2, frm=1 + g % 4, reject=g % 2 == 0)) for g in range(65)]  # (a grant carries term + 1)
    assert f.responses(recs) == [nodes[g].record(m) for g, m in recs]
    saved = f.states()
    assert any(c[2][3] for c in saved) and any(c[2][2] != 1 for c in saved)
    f.eng.checkpoint()
    more = [(g, M.Rec(M.PREVOTE, term=2, frm=(2 + g % 4) % 5 or 1)) for g in range(65)]
    f.responses(more)
    f.eng.follow_elect_write(cells_array(f.E, [0], [(9, M.conf_word((0,), (), 0), 0, 0)]))
    assert f.states() != saved
    f.eng.restore()
    assert f.states() == saved
    f.check_nodes(nodes)
    f.close()


def test_lifecycle_and_refusals(rg):
    """Every call before rg_follow_elect_enable, a second enable and an enable before the gate are RG_ERR_STATE; what the header
    lists as refused is refused on the host and nothing is written or applied."""
    import torch
    E = rg.engine
    cfg = G.Config(10, seed=1)
    eng = rg.Engine(300, 3)
    eng.follow_enable(5)
    one = torch.zeros(256, dtype=torch.int64, device="cuda")
    cols = {k: one for k in E.ELECT_OUT_COLUMNS}
    msgs = {k: one for k in E.VOTE_COLUMNS}
    calls = [lambda: eng.follow_elect_write(np.zeros(0, dtype=E.FOLLOW_ELECT_DTYPE)), lambda: eng.follow_elect_read([0]),
             lambda: eng.follow_campaign(np.zeros(1, dtype=E.FOLLOW_CAMPAIGN_REQ_DTYPE)), lambda: eng.follow_vote_resps(np.zeros(0, dtype=E.FOLLOW_VOTE_REC_DTYPE)),
             lambda: eng.follow_campaign_device(one, one, 1, cols), lambda: eng.follow_vote_resps_device(msgs, cols)]

    def all_state_errors():
        for c in calls:
            with pytest.raises(rg.EngineError) as ei:
                c()
            assert ei.value.code == -8 and "first" in str(ei.value), str(ei.value)  # RG_ERR_STATE
    with pytest.raises(rg.EngineError, match="rg_follow_gate_enable first"):
        eng.follow_elect_enable()
    all_state_errors()
    eng.follow_gate_enable(cfg.election_tick, 0, 0, 0, cfg.seed)
    all_state_errors()
    info = eng.device_info()["engine_bytes"]
    eng.follow_elect_enable()
    assert eng.device_info()["engine_bytes"] == info + 14 * eng.follow_stride()
    with pytest.raises(rg.EngineError, match="already enabled"):
        eng.follow_elect_enable()
    eng.sync()
    eng.close()

    nodes = [cluster(cfg, 3, g) for g in range(5)]
    f = Arena(rg, 5, cfg)
    f.load_nodes(nodes)
    hups = [(g, M.Rec(M.HUP)) for g in range(5)]
    assert f.campaign(hups) == [nodes[g].record(m) for g, m in hups]
    before = f.states()
    conf = M.conf_word((0, 1, 2), (), 0)
    good = (1, conf, 1, 0)
    for groups, cells in (([5], [good]), ([0], [(0, conf, 1, 0)]), ([0], [(1, conf, 3, 2)]), ([0, 1, 0], [good] * 3), ([0], [(1, conf | 1 << 19, 1, 0)])):
        with pytest.raises(rg.EngineError):
            f.eng.follow_elect_write(cells_array(f.E, [1] + groups, [good] + cells))
    with pytest.raises(rg.EngineError):
        f.eng.follow_elect_read([0, 5])
    tn = M.Rec(M.TIMEOUT_NOW, term=3, frm=2)
    for recs in ([(0, M.Rec(M.HUP)), (1, tn), (0, M.Rec(M.HUP))], [(1, tn), (5, M.Rec(M.HUP))], [(1, tn), (2, M.Rec(M.TIMEOUT_NOW, term=0, frm=2))],
                 [(1, tn), (2, M.Rec(M.TIMEOUT_NOW, term=3, frm=0))]):
        with pytest.raises(rg.EngineError):
            f.campaign(recs)
    a = np.zeros(2, dtype=f.E.FOLLOW_CAMPAIGN_REQ_DTYPE)
    a[1]["group"], a[1]["flags"] = 1, 4
    with pytest.raises(rg.EngineError):
        f.eng.follow_campaign(a)
    ok = M.Rec(M.VOTE, term=1, frm=1)
    for g, kind, term, slot in ((5, 4, 1, 1), (1, 4, 1, 8), (1, 12, 1, 1), (1, 0, 1, 1), (1, 16, 1, 1), (1, 4, 0, 1)):
        a = f.vote_recs([(0, ok), (g, ok)])
        a[1]["kind"], a[1]["term"], a[1]["from_slot"] = kind, term, slot
        with pytest.raises(rg.EngineError):
            f.eng.follow_vote_resps(a)
    for bad_cols in ({**cols, "term": None}, {**cols, "flags": None}):
        with pytest.raises(rg.EngineError):
            f.eng.follow_campaign_device(one, one, 1, bad_cols)
        with pytest.raises(rg.EngineError):
            f.eng.follow_vote_resps_device(msgs, bad_cols)
    with pytest.raises(rg.EngineError):
        f.eng.follow_vote_resps_device({**msgs, "slot": None}, cols)
    with pytest.raises(rg.EngineError):
        f.eng.follow_campaign_device(one, None, 1, cols)
    assert f.states() == before
    f.close()
