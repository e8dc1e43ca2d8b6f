"""The follower's term gate, vote step and election clock, restated literally from the reference over follower_model's
entry-list log.

    Raft::step, the term gate        src/raft.rs:1282-1411
    Raft::step, the vote step        src/raft.rs:1418-1461
    Raft::reset                      src/raft.rs:942-971
    Raft::become_follower            src/raft.rs:1082-1087
    Raft::tick / tick_election       src/raft.rs:1024-1047
    Raft::maybe_commit_by_vote       src/raft.rs:2126-2164
    Raft::step_candidate             src/raft.rs:2215-2229
    Raft::step_follower              src/raft.rs:2271-2285
    reset_randomized_election_timeout src/raft.rs:2744-2756 (thread_rng there; the engine's counter draw is restated below)
    RaftLog::is_up_to_date           src/raft_log.rs:412
    RaftLog::maybe_commit            src/raft_log.rs:487
    RaftLog::commit_info             src/raft_log.rs:637

A Node is one followed group: the soft state of a non-leader Raft and a follower_model.Log. Node.step takes a message the way
Raft::step does and returns what the engine's record answers: (gate, events, resp_term, follower response tuple). Where the log
is the bounded view and a term of the dropped gap decides, follower_model's interval rule raises Host: the record is handed back
and NOTHING of the node has changed; the same holds for a FAULT of the log step.
"""
import copy
import random

import follower_model as F

APPEND, HEARTBEAT, VOTE, PREVOTE, TOUCH = 1, 2, 4, 8, 16
CHECK_QUORUM, PRE_VOTE = 1, 2
FORCE = 1
G_NONE, G_PASS, G_IGNORED, G_STALE_LEADER, G_PREVOTE_LOW, G_VOTE_GRANT, G_VOTE_REJECT = range(7)
EV_HARD_STATE, EV_BECAME_FOLLOWER, EV_LEADER_CHANGED, EV_CONF_CHECK = 1, 2, 4, 8
FOLLOWER, PRE_CANDIDATE, CANDIDATE = 0, 1, 2
INVALID_ID = 0
ELAPSED_MAX = 32767
M64 = (1 << 64) - 1


def _mix(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, group, term, prev, lo, hi):
    """rg_follow_draw: a value of [lo, hi)."""
    x = _mix(_mix(_mix(seed ^ group) ^ term) ^ prev)
    return lo + (x >> 32) % (hi - lo)


class Config:
    def __init__(self, election_tick, min_timeout=0, max_timeout=0, flags=0, seed=0):
        self.election_tick = election_tick
        if min_timeout == 0 and max_timeout == 0:
            min_timeout, max_timeout = election_tick, 2 * election_tick
        self.min_timeout, self.max_timeout, self.flags, self.seed = min_timeout, max_timeout, flags, seed

    @property
    def check_quorum(self):
        return bool(self.flags & CHECK_QUORUM)

    @property
    def pre_vote(self):
        return bool(self.flags & PRE_VOTE)


class Msg:
    """A Message as far as a non-leader's Raft::step reads it. kind: one of APPEND .. TOUCH; ents: the entries' terms."""

    def __init__(self, kind, term, frm, index=0, log_term=0, commit=0, commit_term=0, ents=(), priority=0, force=False):
        self.kind, self.term, self.frm, self.index, self.log_term = kind, term, frm, index, log_term
        self.commit, self.commit_term, self.ents, self.priority, self.force = commit, commit_term, list(ents), priority, force

    def key(self):
        return (self.kind, self.term, self.frm, self.index, self.log_term, self.commit, self.commit_term, tuple(self.ents), self.priority, self.force)


class Node:
    SOFT = ("term", "vote", "lead", "priority", "role", "elapsed", "timeout", "promotable")

    def __init__(self, cfg, group, log=None):
        """What rg_follow_gate_enable leaves: a Follower at term 0 that is not promotable, with a drawn timeout."""
        self.cfg, self.group = cfg, group
        self.log = log if log is not None else F.Log()
        self.term = self.vote = self.lead = self.priority = 0
        self.role, self.elapsed, self.promotable = FOLLOWER, 0, False
        self.timeout = draw(cfg.seed, group, 0, 0, cfg.min_timeout, cfg.max_timeout)

    def soft(self):
        return tuple(int(getattr(self, k)) for k in self.SOFT)

    def load(self, term, vote, lead, priority, role, elapsed, timeout, promotable):
        """rg_follow_soft_write of this group (timeout 0 = draw one, chained on the cell's)."""
        if timeout == 0:
            timeout = draw(self.cfg.seed, self.group, term, self.timeout, self.cfg.min_timeout, self.cfg.max_timeout)
        self.term, self.vote, self.lead, self.priority, self.role = term, vote, lead, priority, role
        self.elapsed, self.timeout, self.promotable = elapsed, timeout, bool(promotable)

    # ---- reset / become_follower ----
    def reset(self, term):
        if self.term != term:
            self.term = term
            self.vote = INVALID_ID
        self.lead = INVALID_ID
        self.timeout = draw(self.cfg.seed, self.group, self.term, self.timeout, self.cfg.min_timeout, self.cfg.max_timeout)
        self.elapsed = 0

    def become_follower(self, term, lead):
        self.reset(term)
        self.lead = lead
        if self.role != FOLLOWER:
            self._events |= EV_BECAME_FOLLOWER
        self.role = FOLLOWER

    # ---- tick_election: True = the group is due (the caller delivers the hup, or says it could not) ----
    def tick(self, deliver=True):
        self.elapsed = min(self.elapsed + 1, ELAPSED_MAX)
        if not (self.elapsed >= self.timeout) or not self.promotable:
            return False
        if deliver:
            self.elapsed = 0
        return True

    # ---- Raft::step ----
    def step(self, m):
        assert m.term != 0 and m.frm != 0
        saved = (self.soft(), self.log.copy())
        before = (self.term, self.vote, self.lead, self.log.committed)
        self._events = 0
        try:
            gate, resp_term, resp = self._step(m)
        except F.Host:
            resp = (F.HOST, m.index, saved[1].committed, 0, 0, 0)
            gate, resp_term = None, None
        if gate is None or resp[0] in (F.FAULT, F.HOST):
            kind = self.log.kind
            self.load(*saved[0])
            self.log = saved[1]
            self.log.kind = kind
            return (G_PASS, 0, self.term, resp)
        ev = self._events
        if (self.term, self.vote, self.log.committed) != (before[0], before[1], before[3]):
            ev |= EV_HARD_STATE
        if self.lead != before[2]:
            ev |= EV_LEADER_CHANGED
        return (gate, ev, resp_term, resp)

    def _none(self):
        return (F.NONE, 0, self.log.committed, 0, 0, 0)

    def _step(self, m):
        cfg, vote_kind = self.cfg, m.kind in (VOTE, PREVOTE)
        none = (F.NONE, m.index, self.log.committed, 0, 0, 0)
        if m.term > self.term:
            if vote_kind:
                in_lease = cfg.check_quorum and self.lead != INVALID_ID and self.elapsed < cfg.election_tick
                if not m.force and in_lease:
                    return (G_IGNORED, self.term, none)
            if m.kind == PREVOTE:
                pass  # never change our term in response to a pre-vote request
            elif m.kind in (APPEND, HEARTBEAT, TOUCH):
                self.become_follower(m.term, m.frm)
            else:
                self.become_follower(m.term, INVALID_ID)
        elif m.term < self.term:
            if (cfg.check_quorum or cfg.pre_vote) and m.kind in (APPEND, HEARTBEAT):
                return (G_STALE_LEADER, self.term, none)
            if m.kind == PREVOTE:
                return (G_PREVOTE_LOW, self.term, none)
            return (G_IGNORED, self.term, none)

        log = self.log
        if vote_kind:
            can_vote = self.vote == m.frm or (self.vote == INVALID_ID and self.lead == INVALID_ID) or (m.kind == PREVOTE and m.term > self.term)
            if can_vote and self._is_up_to_date(m.index, m.log_term) and (m.index > log.last_index or self.priority <= m.priority):
                if m.kind == VOTE:
                    self.elapsed = 0
                    self.vote = m.frm
                return (G_VOTE_GRANT, m.term, (F.NONE, m.index, log.committed, 0, 0, 0))
            commit, commit_term = log.committed, F._value(log.term(log.committed))  # commit_info
            resp = (F.NONE, m.index, commit, 0, 0, commit_term)
            self._maybe_commit_by_vote(m)
            return (G_VOTE_REJECT, self.term, resp)
        if self.role in (PRE_CANDIDATE, CANDIDATE):  # step_candidate
            self.become_follower(m.term, m.frm)
        self.elapsed = 0  # step_follower
        self.lead = m.frm
        if m.kind == TOUCH:
            return (G_PASS, self.term, (F.NONE, m.index, log.committed, 0, 0, 0))
        resp = log.heartbeat(m.commit, m.index) if m.kind == HEARTBEAT else log.append(m.index, m.log_term, m.commit, m.ents)
        return (G_PASS, self.term, resp)

    def _is_up_to_date(self, last_index, term):
        last_term = F._value(self.log.term(self.log.last_index))
        return term > last_term or (term == last_term and last_index >= self.log.last_index)

    def _maybe_commit_by_vote(self, m):
        log = self.log
        if m.commit == 0 or m.commit_term == 0:
            return
        last_commit = log.committed
        if m.commit <= last_commit:
            return
        # RaftLog::maybe_commit(m.commit, m.commit_term)
        if not (m.commit > log.committed and F._eq(log.term(m.commit), m.commit_term)):
            return
        log.committed = m.commit  # commit_to: m.commit <= last_index, for term(m.commit) != 0
        if self.role not in (CANDIDATE, PRE_CANDIDATE):
            return
        self._events |= EV_CONF_CHECK  # the host counts the pending conf entries and steps down


# ---- seeded streams (shared by the CPU and the GPU tests) ----
PEERS = (1, 2, 3, 5)


def random_soft(rng, cfg, log):
    """A soft state a host may write: role != Follower implies no leader."""
    last_term = max([log.dummy_term] + log.terms)
    term = last_term + rng.randint(0, 3)
    role = rng.choice((FOLLOWER, FOLLOWER, FOLLOWER, PRE_CANDIDATE, CANDIDATE))
    lead = 0 if role != FOLLOWER or rng.random() < 0.3 else rng.choice(PEERS)
    vote = rng.choice((0, 0) + PEERS)
    elapsed = rng.choice((0, 0, cfg.election_tick - 1, cfg.election_tick, rng.randint(0, cfg.max_timeout)))
    timeout = rng.choice((0, rng.randint(cfg.min_timeout, cfg.max_timeout - 1)))
    return (term, vote, lead, rng.choice((0, 0, 0, -1, 2)), role, elapsed, timeout, rng.random() < 0.8)


def random_msg(rng, node):
    """A message drawn against the node: all five kinds, the three term relations, logs ahead and behind."""
    log = node.log
    x = rng.random()
    kind = APPEND if x < 0.45 else HEARTBEAT if x < 0.6 else VOTE if x < 0.75 else PREVOTE if x < 0.9 else TOUCH
    x = rng.random()
    if x < 0.55:
        term = node.term
    elif x < 0.8:
        term = node.term + rng.randint(1, 2)
    else:
        term = node.term - rng.randint(1, 2)
    term = max(term, 1)
    frm = node.lead if (node.lead and rng.random() < 0.7) else rng.choice(PEERS)
    if kind in (APPEND, HEARTBEAT):
        op = F.random_op(rng, log)
        while (op[0] == "H") != (kind == HEARTBEAT):
            op = F.random_op(rng, log)
        if kind == HEARTBEAT:
            return Msg(kind, term, frm, commit=op[1])
        return Msg(kind, term, frm, index=op[1], log_term=op[2], commit=op[3], ents=op[4])
    if kind == TOUCH:
        return Msg(kind, term, frm)
    last = log.last_index
    last_term = log.terms[-1] if log.terms else log.dummy_term
    index = max(0, last + rng.choice((-1, 0, 0, 1)))
    log_term = max(0, last_term + rng.choice((-1, 0, 0, 0, 1)))
    commit = rng.choice((0, log.committed, log.committed + 1, last, last + 1, rng.randint(0, last + 1)))

    def true_term(i):
        if i < log.dummy_index or i > log.last_index:
            return 0
        return log.dummy_term if i == log.dummy_index else log.terms[i - log.dummy_index - 1]
    commit_term = true_term(commit) if rng.random() < 0.7 else rng.randint(0, 14)
    return Msg(kind, term, frm, index=index, log_term=log_term, commit=commit, commit_term=commit_term,
               priority=rng.choice((0, 0, 0, -1, 1, 2)), force=rng.random() < 0.3)


def make_stream(seed, cfg, groups, n_ops):
    """A seeded stream the way a host drives the gated engine. Events:
        ("W", g, canonical)                   rg_follow_write of the log
        ("G", g, soft tuple as written, soft tuple after)   rg_follow_soft_write
        ("M", g, Msg, answer, canonical after, soft after)  one gated record
        ("K", sorted due groups, {g: soft after})            one rg_follow_clock over the whole arena (cap = everything)
    Returns (events, {coverage key: count})."""
    rng = random.Random(seed)
    nodes, events, cov = {}, [], {}

    def load(g):
        log = F.random_log(rng, 12, bounded=True)
        nodes[g] = Node(cfg, g, log) if g not in nodes else nodes[g]
        nodes[g].log = log
        events.append(("W", g, log.canonical()))
        w = random_soft(rng, cfg, log)
        nodes[g].load(*w)
        events.append(("G", g, w, nodes[g].soft()))
    for g in groups:
        load(g)
    for _ in range(n_ops):
        x = rng.random()
        if x < 0.04:
            due = sorted(g for g in groups if nodes[g].tick())
            events.append(("K", due, {g: nodes[g].soft() for g in groups}))
            cov["tick"] = cov.get("tick", 0) + 1
            cov["hup"] = cov.get("hup", 0) + len(due)
            for g in due:  # the host's hup(): campaign, or pre-campaign
                n = nodes[g]
                if cfg.pre_vote:
                    w = (n.term, n.vote, 0, n.priority, PRE_CANDIDATE, n.elapsed, n.timeout, n.promotable)
                else:
                    w = (n.term + 1, g % 7 + 10, 0, n.priority, CANDIDATE, 0, 0, n.promotable)
                n.load(*w)
                events.append(("G", g, w, n.soft()))
            continue
        g = rng.choice(groups)
        n = nodes[g]
        if len(n.log.terms) > 44 or x < 0.05:
            load(g)
            continue
        m = random_msg(rng, n)
        role = n.role
        rel = "<" if m.term < n.term else "=" if m.term == n.term else ">"
        a = n.step(m)
        for key in (("gate", a[0]), ("kind", m.kind, rel), ("role", role, rel), ("status", a[3][0])) + tuple(("ev", b) for b in (1, 2, 4, 8) if a[1] & b):
            cov[key] = cov.get(key, 0) + 1
        events.append(("M", g, m, a, n.log.canonical(), n.soft()))
        if a[3][0] == F.HOST:  # the host steps the message itself and re-loads the group
            load(g)
    return events, cov


def check_coverage(cov, cfg):
    want = [("gate", k) for k in (G_PASS, G_IGNORED, G_VOTE_GRANT, G_VOTE_REJECT)]
    want += [("kind", k, rel) for k in (APPEND, HEARTBEAT, VOTE, PREVOTE, TOUCH) for rel in "<=>"]
    want += [("role", r, rel) for r in (FOLLOWER, PRE_CANDIDATE, CANDIDATE) for rel in "<=>"]
    want += [("status", s) for s in (F.NONE, F.ACCEPT, F.REJECT, F.STALE, F.HEARTBEAT, F.FAULT, F.HOST)]
    want += [("ev", b) for b in (1, 2, 4, 8)] + [("gate", G_PREVOTE_LOW), "tick", "hup"]
    if cfg.check_quorum or cfg.pre_vote:
        want.append(("gate", G_STALE_LEADER))
    missing = [k for k in want if not cov.get(k)]
    assert not missing, (missing, cov)
