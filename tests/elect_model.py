"""The candidate half -- campaign, vote responses and poll -- restated literally from the reference on top of gate_model.Node.

    Raft::hup                        src/raft.rs:1472-1525
    Raft::campaign                   src/raft.rs:1217-1263
    Raft::become_candidate           src/raft.rs:1101-1117
    Raft::become_pre_candidate       src/raft.rs:1124-1143
    Raft::become_leader (its reset)  src/raft.rs:1151-1161
    Raft::poll                       src/raft.rs:2166-2201
    Raft::step_candidate (responses, MsgTimeoutNow)  src/raft.rs:2230-2251
    Raft::step_follower (MsgTimeoutNow)              src/raft.rs:2298-2318
    Raft::maybe_commit_by_vote       src/raft.rs:2126-2164
    ProgressTracker::record_vote / tally_votes / vote_result   src/tracker.rs:307-344
    MajorityConfig::vote_result      src/quorum/majority.rs:130-154
    JointConfig::vote_result         src/quorum/joint.rs:56-67

A Node is one followed group with the three layers of the arena: the log (follower_model.Log), the soft state (gate_model.Node)
and the election cells: self_id, the configuration as SETS of slots, the votes as a dict {slot: granted} -- no mask arithmetic
here, so this file shares nothing with raft_rs_amd/csrc/rg_elect.h, which it checks. Node.record takes one record and returns what
the engine answers, ANSWER_FIELDS; where a term of the dropped gap decides (follower_model.Host) nothing of the node has changed.

How the arena holds a group that WON: role Follower with leader_id == self_id (the group is the leader engine's from then on).
"""
import random

import follower_model as F
import gate_model as G
from gate_model import CANDIDATE, FOLLOWER, INVALID_ID, PRE_CANDIDATE

VOTE, PREVOTE, HUP, TIMEOUT_NOW = 4, 8, 0x20, 0x40  # a record's kind: a response to that request kind, or one of the two local ones
F_REJECT, F_BLOCKED = 1, 2
NONE, IGNORED, BLOCKED, REQUESTS, PENDING, LOST, WON, STEPPED_DOWN = range(8)
REQ_TRANSFER = 1
V_PENDING, V_LOST, V_WON = 0, 1, 2
CAMPAIGN_PRE_ELECTION, CAMPAIGN_ELECTION, CAMPAIGN_TRANSFER = "pre", "election", "transfer"
ANSWER_FIELDS = ("result", "events", "term", "req_kind", "targets", "flags", "req_term", "req_index", "req_log_term", "req_commit", "req_commit_term",
                 "status")


class Rec:
    """One record. kind VOTE / PREVOTE: a response, frm = the sender's SLOT; TIMEOUT_NOW: frm = Message.from; HUP: local."""

    def __init__(self, kind, term=0, frm=0, reject=False, blocked=False, commit=0, commit_term=0):
        self.kind, self.term, self.frm, self.reject, self.blocked, self.commit, self.commit_term = kind, term, frm, reject, blocked, commit, commit_term

    def key(self):
        return (self.kind, self.term, self.frm, self.reject, self.blocked, self.commit, self.commit_term)

    @property
    def flags(self):
        return (F_REJECT if self.reject else 0) | (F_BLOCKED if self.blocked else 0)


def conf_word(incoming, outgoing, self_slot):
    """RG_ELECT_CONF_MAKE from sets of slots"""
    return sum(1 << s for s in incoming) | (sum(1 << s for s in outgoing) << 8) | (self_slot << 16)


def majority_vote_result(voters, check):
    """MajorityConfig::vote_result (majority.rs:130-154); check(id) -> True / False / None"""
    if not voters:
        return V_WON  # by convention, the elections on an empty config win
    yes = missing = 0
    for v in voters:
        c = check(v)
        if c is None:
            missing += 1
        elif c:
            yes += 1
    q = len(voters) // 2 + 1
    if yes >= q:
        return V_WON
    if yes + missing >= q:
        return V_PENDING
    return V_LOST


class Node(G.Node):
    def __init__(self, cfg, group, log=None, self_id=0, incoming=(), outgoing=(), self_slot=0):
        super().__init__(cfg, group, log)
        self.self_id, self.incoming, self.outgoing, self.self_slot = self_id, set(incoming), set(outgoing), self_slot
        self.votes = {}

    # ---- the election cells, as rg_follow_elect_write takes and rg_follow_elect_read reports them ----
    def load_elect(self, self_id, conf, yes, no):
        self.self_id = self_id
        self.incoming = {s for s in range(8) if conf >> s & 1}
        self.outgoing = {s for s in range(8) if conf >> (8 + s) & 1}
        self.self_slot = conf >> 16 & 7
        self.votes = {s: bool(yes >> s & 1) for s in range(8) if (yes | no) >> s & 1}

    def cells(self):
        """(self_id, conf, yes, no); the votes of a Follower read as 0 (reset cleared them)"""
        votes = self.votes if self.role != FOLLOWER else {}
        return (self.self_id, conf_word(self.incoming, self.outgoing, self.self_slot),
                sum(1 << s for s, v in votes.items() if v), sum(1 << s for s, v in votes.items() if not v))

    # ---- reset (raft.rs:942-971): prs.reset_votes() on top of what the gate's model does ----
    def reset(self, term):
        super().reset(term)
        self.votes = {}

    def become_candidate(self):
        term = self.term + 1
        self.reset(term)
        self.vote = self.self_id
        self.role = CANDIDATE

    def become_pre_candidate(self):
        self.role = PRE_CANDIDATE
        self.votes = {}
        self.lead = INVALID_ID

    def become_leader(self):
        term = self.term
        self.reset(term)
        self.lead = self.self_id
        self.role = FOLLOWER  # the arena's form of "Leader": the group is handed to the leader engine
        self._leader = True
        self._result = WON

    # ---- ProgressTracker ----
    def record_vote(self, slot, vote):
        self.votes.setdefault(slot, vote)  # tracker.rs:307-309

    def vote_result(self):
        check = self.votes.get  # tracker.rs:339-344: a slot that has not voted is None
        i, o = majority_vote_result(self.incoming, check), majority_vote_result(self.outgoing, check)
        if i == V_WON and o == V_WON:  # joint.rs:56-67
            return V_WON
        if i == V_LOST or o == V_LOST:
            return V_LOST
        return V_PENDING

    # ---- hup / campaign / poll ----
    def hup(self, transfer_leader, blocked):
        if self.lead == self.self_id:  # state == Leader
            return
        if blocked:  # num_pending_conf(ents) != 0: the host's count
            self._result = BLOCKED
            return
        if transfer_leader:
            self.campaign(CAMPAIGN_TRANSFER)
        elif self.cfg.pre_vote:
            self.campaign(CAMPAIGN_PRE_ELECTION)
        else:
            self.campaign(CAMPAIGN_ELECTION)

    def campaign(self, campaign_type):
        if campaign_type == CAMPAIGN_PRE_ELECTION:
            self.become_pre_candidate()
            vote_msg, term = PREVOTE, self.term + 1
        else:
            self.become_candidate()
            vote_msg, term = VOTE, self.term
        if self.poll(self.self_slot, True) == V_WON:
            return
        commit, commit_term = self.log.committed, F._value(self.log.term(self.log.committed))  # commit_info
        targets = 0
        for slot in sorted(self.incoming | self.outgoing):
            if slot == self.self_slot:
                continue
            targets |= 1 << slot
        last_term = F._value(self.log.term(self.log.last_index))
        self._request = (vote_msg, targets, REQ_TRANSFER if campaign_type == CAMPAIGN_TRANSFER else 0, term, self.log.last_index, last_term, commit, commit_term)
        self._result = REQUESTS

    def poll(self, slot, vote):
        self.record_vote(slot, vote)
        res = self.vote_result()
        if res == V_WON:
            if self.role == PRE_CANDIDATE:
                self.campaign(CAMPAIGN_ELECTION)
            else:
                self.become_leader()
        elif res == V_LOST:
            term = self.term
            self.become_follower(term, INVALID_ID)
            self._result = LOST
        else:
            self._result = PENDING
        return res

    def maybe_commit_by_vote_response(self, m):
        log = self.log
        if m.commit == 0 or m.commit_term == 0:
            return
        last_commit = log.committed
        if m.commit <= last_commit or self._leader:
            return
        if not (m.commit > log.committed and F._eq(log.term(m.commit), m.commit_term)):  # RaftLog::maybe_commit
            return
        log.committed = m.commit
        if self.role not in (CANDIDATE, PRE_CANDIDATE):
            return
        self._events |= G.EV_CONF_CHECK

    # ---- Raft::step for the four record kinds ----
    def _gate(self, m):
        """-> False: the message goes no further"""
        if m.term > self.term:
            if m.kind == PREVOTE and not m.reject:
                pass  # a granted pre-vote response carries our future term
            else:
                self.become_follower(m.term, INVALID_ID)
                self._result = STEPPED_DOWN
        elif m.term < self.term:
            return False
        return True

    def step_response(self, m):
        if not self._gate(m):
            return
        if self.role == FOLLOWER:
            return  # step_follower: _ => {}
        if (self.role == PRE_CANDIDATE and m.kind != PREVOTE) or (self.role == CANDIDATE and m.kind != VOTE):
            return
        self.poll(m.frm, not m.reject)
        self.maybe_commit_by_vote_response(m)

    def timeout_now(self, m):
        if not self._gate(m):
            return
        if self.role != FOLLOWER:
            return  # step_candidate ignores it
        if self.promotable:
            self.hup(True, m.blocked)

    def record(self, m):
        saved = (self.soft(), self.log.copy(), (self.self_id, set(self.incoming), set(self.outgoing), self.self_slot, dict(self.votes)))
        before = (self.term, self.vote, self.lead, self.log.committed)
        self._events, self._result, self._request, self._leader = 0, IGNORED, None, False
        try:
            if m.kind == HUP:
                self.hup(False, m.blocked)
            elif m.kind == TIMEOUT_NOW:
                self.timeout_now(m)
            else:
                self.step_response(m)
        except F.Host:
            self.load(*saved[0])
            self.log = saved[1]
            self.self_id, self.incoming, self.outgoing, self.self_slot, self.votes = saved[2]
            return (NONE, 0, self.term, 0, 0, 0, 0, 0, 0, 0, 0, F.HOST)
        ev = self._events
        if (self.term, self.vote, self.log.committed) != (before[0], before[1], before[3]):
            ev |= G.EV_HARD_STATE
        if self.lead != before[2]:
            ev |= G.EV_LEADER_CHANGED
        req = self._request if self._result == REQUESTS else None
        return (self._result, ev, self.term) + (req if req else (0,) * 8) + (F.NONE,)


# ---- seeded streams (shared by the CPU and the GPU tests) ----
CONFS = [  # (incoming, outgoing, self_slot, coverage class)
    ((0, 1, 2), (), 0, "majority"), ((0, 1, 2), (), 2, "majority"), ((0, 1, 2, 3, 4), (), 1, "majority"), ((0, 1, 2, 3), (), 3, "majority"),
    ((0, 1, 2, 3, 4, 5, 6), (), 6, "majority"), ((0, 1, 2, 3, 4, 5, 6, 7), (), 7, "majority"),
    ((0, 1, 2), (0, 3, 4), 0, "joint"), ((1, 2, 3), (1, 2, 3, 4, 5), 2, "joint"), ((0, 1), (2, 3, 4), 0, "joint"),
    ((3,), (), 3, "singleton"), ((0,), (), 0, "singleton"), ((2,), (2,), 2, "singleton"),
    ((0, 1, 2), (), 5, "self_not_voter"), ((0, 1, 2), (3, 4, 6), 7, "self_not_voter"), ((), (), 0, "self_not_voter"),
]


def random_log(rng):
    """A bounded log; where its table has dropped runs, every other time the commit index lies in the gap (commit_info needs
    a term of the gap then: the record is handed back)."""
    log = F.random_log(rng, rng.choice((4, 12, 12)), bounded=True)
    if log.known > log.dummy_index + 1 and rng.random() < 0.5:
        log.committed = rng.randint(log.dummy_index + 1, log.known - 1)
    return log


def random_elect(rng, soft):
    """Election cells a host may write beside `soft`: (self_id, conf, yes, no, coverage class)."""
    incoming, outgoing, self_slot, cls = rng.choice(CONFS)
    role = soft[4]
    yes = no = 0
    if role != FOLLOWER:  # a candidate has voted for itself; some peers have answered
        yes = 1 << self_slot
        for s in set(incoming) | set(outgoing):
            x = rng.random()
            if s != self_slot and x < 0.3:
                if x < 0.12:
                    yes |= 1 << s
                else:
                    no |= 1 << s
    return (100 + self_slot, conf_word(incoming, outgoing, self_slot), yes, no, cls)


def random_soft(rng, cfg, log):
    """As gate_model.random_soft with more candidates; a candidate has voted for itself (the caller fixes `vote`)."""
    term, vote, lead, prio, role, elapsed, timeout, promotable = G.random_soft(rng, cfg, log)
    if rng.random() < 0.55:
        role, lead = rng.choice((PRE_CANDIDATE, PRE_CANDIDATE, CANDIDATE)), 0
    return (max(term, 1), vote, lead, prio, role, elapsed, timeout, promotable and rng.random() < 0.85)


def random_rec(rng, node):
    x = rng.random()
    if x < 0.12:
        return Rec(HUP, blocked=rng.random() < 0.15)
    y = rng.random()
    if node.role == PRE_CANDIDATE and x >= 0.26 and y < 0.3:
        rel = 1  # the usual granted pre-vote response carries term + 1
    else:
        rel = 0 if y < 0.65 else rng.randint(1, 2) if y < 0.82 else -rng.randint(1, 2)
    term = max(node.term + rel, 1)
    if x < 0.26:
        return Rec(TIMEOUT_NOW, term=term, frm=rng.choice(G.PEERS), blocked=rng.random() < 0.15)
    kind = (PREVOTE if node.role == PRE_CANDIDATE else VOTE) if rng.random() < 0.65 else rng.choice((VOTE, PREVOTE))
    voters = sorted(node.incoming | node.outgoing)
    slot = rng.choice(voters) if voters and rng.random() < 0.85 else rng.randint(0, 7)
    if node.votes and rng.random() < 0.15:
        slot = rng.choice(sorted(node.votes))  # a slot that has voted already
    reject = rng.random() < 0.45
    if kind == PREVOTE and rel > 0 and rng.random() < 0.8:
        reject = False
    log = node.log
    commit = commit_term = 0
    if reject and rng.random() < 0.6:
        last = log.last_index
        commit = rng.choice((log.committed, log.committed + 1, last, last + 1, rng.randint(0, last + 1)))
        true_term = 0 if commit < log.dummy_index or commit > last else log.dummy_term if commit == log.dummy_index else log.terms[commit - log.dummy_index - 1]
        commit_term = true_term if rng.random() < 0.8 else rng.randint(0, 14)
    return Rec(kind, term=term, frm=slot, reject=reject, commit=commit, commit_term=commit_term)


def cover(cov, node, m, cls, a, role, promotable, voted):
    def hit(key):
        cov[key] = cov.get(key, 0) + 1
    hit("records")
    hit(("result", a[0]))
    hit(("status", a[11]))
    hit(("conf", cls))
    for b in (1, 2, 4, 8):
        if a[1] & b:
            hit(("ev", b))
    if m.kind in (VOTE, PREVOTE):
        rel = "<" if m.term < node_term(a, m) else "=" if m.term == node_term(a, m) else ">"
        hit(("resp", m.kind, rel, role))
        if m.frm in voted and voted[m.frm] == m.reject and a[11] == F.NONE and a[0] in (PENDING, LOST, WON, REQUESTS):
            hit("repeat_opposite")
    elif m.kind == TIMEOUT_NOW:
        hit(("timeout_now", role, bool(promotable)))
        if a[5] & REQ_TRANSFER:
            hit("transfer")
    if m.blocked and a[0] == BLOCKED:
        hit("blocked")
    if m.kind == HUP and a[0] == IGNORED:
        hit("hup_of_a_leader")


def node_term(a, m):
    return m._term_before


def make_stream(seed, cfg, groups, n_ops):
    """A seeded stream the way a host drives the arena's three layers. Events:
        ("W", g, canonical)                                  rg_follow_write of the log
        ("G", g, soft tuple as written, soft tuple after)    rg_follow_soft_write
        ("E", g, cells as written, cells after)              rg_follow_elect_write
        ("R", g, Rec, answer, canonical after, soft after, cells after)   one record
        ("K", sorted due groups, {g: soft after the tick}, {g: blocked}, [the "R" events of the due groups' MsgHup, in that order])
                                                             one rg_follow_clock over the arena and the campaign of its list
    Returns (events, {coverage key: count})."""
    rng = random.Random(seed)
    nodes, cls_of, events, cov = {}, {}, [], {}

    def load(g):
        log = random_log(rng)
        if g not in nodes:
            nodes[g] = Node(cfg, g)
        n = nodes[g]
        n.log = log
        events.append(("W", g, log.canonical()))
        w = random_soft(rng, cfg, log)
        e = random_elect(rng, w)
        if w[4] == CANDIDATE:
            w = (w[0], e[0]) + w[2:]
        elif w[4] == FOLLOWER and w[2] == 0 and rng.random() < 0.06:
            w = w[:2] + (e[0],) + w[3:]  # a group this store leads
        n.load(*w)
        events.append(("G", g, w, n.soft()))
        n.load_elect(*e[:4])
        cls_of[g] = e[4]
        events.append(("E", g, e[:4], n.cells()))

    def one(g, m):
        n = nodes[g]
        role, promotable, voted = n.role, n.promotable, dict(n.votes)
        m._term_before = n.term
        a = n.record(m)
        cover(cov, n, m, cls_of[g], a, role, promotable, voted)
        return ("R", g, m, a, n.log.canonical(), n.soft(), n.cells())
    for g in groups:
        load(g)
    for _ in range(n_ops):
        x = rng.random()
        if x < 0.03:
            due = sorted(g for g in groups if nodes[g].tick())
            softs = {g: nodes[g].soft() for g in groups}
            blocked = {g: rng.random() < 0.1 for g in due}
            cov["tick"] = cov.get("tick", 0) + 1
            cov["storm_hup"] = cov.get("storm_hup", 0) + len(due)
            recs = [one(g, Rec(HUP, blocked=blocked[g])) for g in due]
            events.append(("K", due, softs, blocked, recs))
            for ev in recs:
                if ev[3][11] == F.HOST:
                    load(ev[1])
            continue
        g = rng.choice(groups)
        if x < 0.12:
            load(g)
            continue
        ev = one(g, random_rec(rng, nodes[g]))
        events.append(ev)
        if ev[3][11] == F.HOST:  # the host handles the record itself and re-loads the group
            load(g)
    return events, cov


def plan_rounds(n, seed, cfg, rounds):
    """What the GPU stream test runs, from the model alone: n groups and `rounds` rounds, each ONE call (or one chained pair) per
    arena. -> (rounds, coverage); a round is {"kind", "records": [(g, Rec, answer)], "states": [(canonical, soft, cells) of every
    group after it]} and
        "load"       "loads": [(g, canonical, soft as written, cells as written)] -- rg_follow_write / _soft_write / _elect_write
        "responses"  at most one vote response per group: the dense form, or one sparse call in any order
        "multi"      vote responses, several per group, array order per group: one sparse call
        "campaign"   MsgHup / MsgTimeoutNow records of distinct groups: one rg_follow_campaign
        "storm"      one clock tick, then MsgHup for the due groups ("due", sorted; "blocked": {g: bool}): clock + campaign_device
    A record that is handed back (HOST) leaves its group as it was, so the rounds simply go on."""
    rng = random.Random(seed)
    nodes, cls_of, cov, out = [Node(cfg, g) for g in range(n)], {}, {}, []

    def load(g):
        log = random_log(rng)
        w = random_soft(rng, cfg, log)
        e = random_elect(rng, w)
        if w[4] == CANDIDATE:
            w = (w[0], e[0]) + w[2:]
        elif w[4] == FOLLOWER and w[2] == 0 and rng.random() < 0.06:
            w = w[:2] + (e[0],) + w[3:]
        nodes[g].log = log
        nodes[g].load(*w)
        nodes[g].load_elect(*e[:4])
        cls_of[g] = e[4]
        return (g, log.canonical(), w, e[:4])

    def one(g, m):
        nd = nodes[g]
        role, promotable, voted = nd.role, nd.promotable, dict(nd.votes)
        m._term_before = nd.term
        a = nd.record(m)
        cover(cov, nd, m, cls_of[g], a, role, promotable, voted)
        return (g, m, a)

    def response(g):
        while True:
            m = random_rec(rng, nodes[g])
            if m.kind in (VOTE, PREVOTE):
                return m

    def local(g):
        while True:
            m = random_rec(rng, nodes[g])
            if m.kind in (HUP, TIMEOUT_NOW):
                return m
    for r in range(rounds):
        kind = "load" if r == 0 else ("responses", "storm", "multi", "responses", "campaign", "responses", "load")[r % 7]
        rd = {"kind": kind, "records": []}
        if kind == "load":
            rd["loads"] = [load(g) for g in range(n) if r == 0 or rng.random() < 0.3]
        elif kind == "responses":
            quiet = range(256, 512) if r % 2 else ()  # every other time: a workgroup without a message
            rd["records"] = [one(g, response(g)) for g in range(n) if g not in quiet and rng.random() < 0.6]
        elif kind == "multi":
            todo = [g for g in range(n) if rng.random() < 0.5]
            todo += [g for g in todo if rng.random() < 0.5] + [g for g in todo if rng.random() < 0.2]
            rng.shuffle(todo)
            rd["records"] = [one(g, response(g)) for g in todo]
        elif kind == "campaign":
            todo = [g for g in range(n) if rng.random() < 0.4]
            rng.shuffle(todo)
            rd["records"] = [one(g, local(g)) for g in todo]
        else:
            rd["due"] = sorted(g for g in range(n) if nodes[g].tick())
            rd["blocked"] = {g: rng.random() < 0.1 for g in rd["due"]}
            cov["tick"] = cov.get("tick", 0) + 1
            cov["storm_hup"] = cov.get("storm_hup", 0) + len(rd["due"])
            rd["records"] = [one(g, Rec(HUP, blocked=rd["blocked"][g])) for g in rd["due"]]
        rd["states"] = [(nd.log.canonical(), nd.soft(), nd.cells()) for nd in nodes]
        out.append(rd)
    return out, cov


GPU_PLAN = (513, 31, G.Config(3, flags=G.CHECK_QUORUM | G.PRE_VOTE, seed=77), 36)  # plan_rounds' arguments in tests/test_follow_elect_gpu.py
GPU_PLAN_NO_PREVOTE = (257, 32, G.Config(4, 4, 9, 0, seed=78), 22)


def check_coverage(cov, cfg):
    want = [("result", r) for r in (IGNORED, BLOCKED, REQUESTS, PENDING, LOST, WON, STEPPED_DOWN)] + [("result", NONE), ("status", F.HOST), ("status", F.NONE)]
    want += [("ev", b) for b in (1, 2, 4, 8)]
    want += [("resp", k, rel, role) for k in (VOTE, PREVOTE) for rel in "<=>" for role in (FOLLOWER, PRE_CANDIDATE, CANDIDATE)]
    want += [("conf", c) for c in ("majority", "joint", "singleton", "self_not_voter")]
    want += [("timeout_now", role, p) for role in (FOLLOWER, PRE_CANDIDATE, CANDIDATE) for p in (False, True)]
    want += ["repeat_opposite", "blocked", "transfer", "hup_of_a_leader", "tick", "storm_hup"]
    missing = [k for k in want if not cov.get(k)]
    assert not missing, (missing, cov)
    # a condition on the generator, not a measurement: at most one record in ten is handed back
    assert cov[("status", F.HOST)] * 10 <= cov["records"], (cov[("status", F.HOST)], cov["records"])
