"""The dense vote step (include/raftgroups_vote.h) as a literal Python model: Raft::step of a MsgRequestVote / MsgRequestPreVote at
a group this store follows OR leads. Citations: pingcap/raft-rs v0.6.0.

    Raft::step, the term gate        src/raft.rs:1282-1411
        m.term > self.term, the vote kinds: the lease        :1285-1317   in_lease = check_quorum && leader_id != INVALID_ID &&
                                                                          election_elapsed < election_timeout (:1289-1291)
        the pre-vote exception                               :1319-1330
        become_follower(m.term, INVALID_ID)                  :1346
        m.term < self.term                                   :1349-1410 (a pre-vote is answered with a reject, a vote ignored)
    Raft::step, the vote step        src/raft.rs:1418-1461 (can_vote :1420-1426)
    Raft::maybe_commit_by_vote       src/raft.rs:2126-2164 (`self.state == StateRole::Leader` returns at :2131)
    Raft::tick_heartbeat             src/raft.rs:1051-1079 (the only place a leader's election_elapsed advances)
    Raft::reset / become_follower    src/raft.rs:942-971, :1082-1087

It COMPOSES the models the other stages have and restates nothing of them: the followed group is a gate_model.Node (its step IS
the answer of a group that is not led, and the vote step of a group once it is deposed), the leader's log is handoff_model's
lead dict (demote, log_of), the leader's clock is lead_clock_model's dict -- its "el" is the Leader's REAL election_elapsed, and
the lease below is evaluated on it as the reference writes it --, the lead-side stop is term_gate_model's, the pending reads are
a readonly_model.Group. Nothing below is derived from csrc/rg_vote.h.

ONE departure, loud: at an equal term a request whose `from` is the id the leader voted for (its own) would pass can_vote; no
peer sends it, the engine answers FAULT, and so does the model. Following the reference there would let a Leader grant a real
vote -- vote = from, election_elapsed = 0 -- and go on leading, which needs a store into a led group's clock cell that no stage
has; the record can only be forged or corrupted, so it is the host's. On this one branch the model and the code share a rule
written down here, not one taken from the reference: the twin checks only that both follow it."""
import copy

import follower_model as F
import gate_model as G
import handoff_model as H
import lead_clock_model as L
import readonly_model as RO  # noqa: F401  (the type of `read_only`)
import term_gate_model as T

EV_LED, EV_TRANSFER_ABORTED, EV_DEPOSED = 0x20, 0x40, 0x80
FAULT_ANSWER = (F.FAULT, G.G_NONE, 0, 0, 0, 0, 0)
NO_LEAD = L.NO_LEAD


def in_lease(check_quorum, leader_id, election_elapsed, election_timeout):
    """raft.rs:1289-1291, as written"""
    return check_quorum and leader_id != G.INVALID_ID and election_elapsed < election_timeout


def win_state(node):
    return node.role == G.FOLLOWER and getattr(node, "self_id", 0) != 0 and node.lead == node.self_id


def answer_of(node, a):
    """gate_model.Node.step's answer in this call's fields: (status, gate, events, term, commit, log_term, last_index)"""
    gate, ev, resp_term, resp = a
    return (resp[0], gate, ev, resp_term, resp[2], resp[5], node.log.last_index)


def step_follower(node, m):
    """NOT LED: exactly the gated step."""
    return answer_of(node, node.step(m))


def step_leader(cfg, election_tick, node, lead, clock, read_only, m):
    """LED: Raft::step of `m` at a Raft in the Leader role. node: the followed group in the win state (term, vote, priority; its
    log is stale and is replaced on a deposition); lead: handoff_model's lead dict; clock: lead_clock_model's dict or None (the
    layer is off: a leadership the clock never saw has election_elapsed 0); read_only: readonly_model.Group or None.
    -> (answer, deposed). Everything changes only where deposed; FAULT and HOST change nothing."""
    if node.term != lead["cur_term"]:
        return FAULT_ANSWER, False
    if clock is not None and not T.led(clock):
        return FAULT_ANSWER, False  # the lead side has stopped the group already
    a, c = H.demote(lead)
    if a[0] != H.DONE:
        return FAULT_ANSWER, False
    log = H.log_of(c)  # the Leader's RaftLog
    cur, last, committed = node.term, c["last_index"], c["committed"]
    election_elapsed = clock["el"] if clock is not None and clock["tag"] == clock["cur_term"] else 0
    host = (F.HOST, G.G_PASS, 0, cur, committed, 0, last)
    if m.term > cur:
        if not m.force and in_lease(cfg.check_quorum, node.lead, election_elapsed, election_tick):
            return (F.NONE, G.G_IGNORED, EV_LED, cur, committed, 0, last), False
        if m.kind == G.PREVOTE:
            pass  # :1319-1330: never change our term in response to a pre-vote request
        else:  # :1346 -- the Leader becomes a Follower and the SAME step goes on to the vote step
            n2, lead2 = copy.deepcopy(node), H.copy_lead(lead)
            clock2, ro2 = (L.copy_group(clock) if clock is not None else None), copy.deepcopy(read_only)
            lead2["cfg"] = lead2.get("cfg", 0)
            transfer = lead2["cfg"] >> 20 & 0xF
            d, c2 = T.depose(n2, lead2, m.term, clock2, ro2)
            assert d[0] == H.DONE
            n2.log = H.log_of(c2)
            before = (node.term, node.vote, node.lead, committed)
            n2._events = 0
            try:
                gate, resp_term, resp = n2._step(m)  # equal terms now: can_vote by vote == 0 && leader_id == 0
            except F.Host:
                return host, False
            ev = n2._events | EV_LED | EV_DEPOSED | (EV_TRANSFER_ABORTED if transfer else 0)
            if (n2.term, n2.vote, n2.log.committed) != (before[0], before[1], before[3]):
                ev |= G.EV_HARD_STATE
            if n2.lead != before[2]:
                ev |= G.EV_LEADER_CHANGED
            node.__dict__.update(n2.__dict__)
            lead.update(lead2)
            if clock is not None:
                clock.update(clock2)
            if read_only is not None:
                read_only.__dict__.update(ro2.__dict__)
            return (resp[0], gate, ev, resp_term, resp[2], resp[5], last), True
    elif m.term < cur:
        return (F.NONE, G.G_PREVOTE_LOW if m.kind == G.PREVOTE else G.G_IGNORED, EV_LED, cur, committed, 0, last), False
    # ---- the vote step of a Leader (:1418-1461): nothing is recorded unless a real vote is granted ----
    if m.term == cur and node.vote == m.frm:
        return FAULT_ANSWER, False  # the departure
    can_vote = node.vote == m.frm or (node.vote == G.INVALID_ID and node.lead == G.INVALID_ID) or (m.kind == G.PREVOTE and m.term > cur)
    try:
        if can_vote:
            last_term = F._value(log.term(log.last_index))
            if (m.log_term > last_term or (m.log_term == last_term and m.index >= log.last_index)) and (m.index > log.last_index or node.priority <= m.priority):
                assert m.kind == G.PREVOTE  # a real vote is granted by a Follower only
                return (F.NONE, G.G_VOTE_GRANT, EV_LED, m.term, committed, 0, last), False
        commit_term = F._value(log.term(log.committed))  # commit_info
    except F.Host:
        return host, False
    # maybe_commit_by_vote: `if self.state == StateRole::Leader { return; }` (:2131)
    return (F.NONE, G.G_VOTE_REJECT, EV_LED, cur, committed, commit_term, last), False


def step(cfg, election_tick, node, lead, clock, read_only, m, n_groups=None, lead_group=0):
    """One request of either form. lead None = the dev_lead cell is NO_LEAD (or the column is NULL)."""
    if lead is not None and n_groups is not None and lead_group >= n_groups:
        return FAULT_ANSWER, False
    if lead is None or not win_state(node):
        return step_follower(node, m), False
    return step_leader(cfg, election_tick, node, lead, clock, read_only, m)


# ---- the seeded cases (shared by the CPU and the GPU tests) ----
def leader_case(rng, cfg, group, behind=None, gap=False):
    """(node, lead dict, clock dict): a group a win and a promotion left, somewhere in its leadership. The node's own log is the
    stale summary the arena keeps (empty here)."""
    c = H.random_canon(rng)
    while not c["runs"] or (gap and c["runs"][0][0] == c["dummy_index"] + 1) or c["last_index"] > 1 << 40:
        c = H.random_canon(rng)
    lead = H.fresh_lead(3, L.cfg_word((0, 1, 2), self_slot=0, transferee=(rng.randrange(3) if rng.random() < 0.3 else None)))
    runs = c["runs"]
    older = runs[:-1][-H.TERM_RUNS:]
    lead.update(commit=c["committed"], term_lo=runs[-1][0], term_hi=c["last_index"], cur_term=runs[-1][1], dummy_index=c["dummy_index"], dummy_term=c["dummy_term"],
                run_count=len(older), run_first=[r[0] for r in older] + [0] * (H.TERM_RUNS - len(older)),
                run_term=[r[1] for r in older] + [0] * (H.TERM_RUNS - len(older)))
    self_id = rng.randint(1, 9)
    node = G.Node(cfg, group)
    node.load(lead["cur_term"], self_id, self_id, rng.choice((0, 0, 0, -1, 2)), G.FOLLOWER, rng.randrange(cfg.election_tick), 0, True)
    node.self_id = self_id
    clock = L.new_group(3, lead["cfg"], cur_term=lead["cur_term"])
    clock["el"], clock["hb"] = rng.randrange(cfg.election_tick), 0
    return node, lead, clock


def request_for(rng, cur, last, last_term, committed, true_term, self_id):
    """A (pre-)vote request drawn against a log: the three term relations, logs ahead / equal / behind, priorities, FORCE."""
    kind = rng.choice((G.VOTE, G.PREVOTE))
    x = rng.random()
    term = cur if x < 0.25 else cur + rng.randint(1, 2) if x < 0.8 else max(cur - rng.randint(1, 2), 1)
    frm = rng.choice([p for p in (11, 12, 13) if p != self_id])
    index = max(0, last + rng.choice((-1, 0, 0, 1)))
    log_term = max(0, last_term + rng.choice((-1, 0, 0, 0, 1)))
    commit = rng.choice((0, committed, committed + 1, last, last + 1, rng.randint(0, last + 1)))
    commit_term = true_term(commit) if rng.random() < 0.7 else rng.randint(0, 14)
    return G.Msg(kind, term, frm, index=index, log_term=log_term, commit=commit, commit_term=commit_term, priority=rng.choice((0, 0, 0, -1, 1, 2)),
                 force=rng.random() < 0.35)


def true_term_of(c):
    log = H.log_of(c)

    def t(i):
        if i < log.dummy_index or i > log.last_index:
            return 0
        return log.dummy_term if i == log.dummy_index else log.terms[i - log.dummy_index - 1]
    return t


def random_case(rng, cfg, group):
    """-> (led, node, lead or None, clock or None, Msg): about half led, half not (all three roles, logs with and without gaps)."""
    if rng.random() < 0.5:
        node, lead, clock = leader_case(rng, cfg, group, gap=rng.random() < 0.25)
        kind = rng.random()
        if kind < 0.04:
            node.term += 1  # a term mismatch: FAULT
        elif kind < 0.08:
            clock["led"] = False  # stopped under the current tag: FAULT
        elif kind < 0.12:
            lead["commit"] = lead["term_hi"] + 1  # a log the demotion refuses: FAULT
        elif kind < 0.2:
            clock = None
        c = H.demote(lead)[1] or {"committed": 0, "last_index": 0, "dummy_index": 0, "dummy_term": 0, "runs": []}
        m = request_for(rng, node.term, c["last_index"], lead["cur_term"], c["committed"], true_term_of(c), node.self_id)
        return True, node, lead, clock, m
    log = F.random_log(rng, 12, bounded=True)
    node = G.Node(cfg, group, log)
    node.load(*G.random_soft(rng, cfg, log))
    m = G.random_msg(rng, node)
    while m.kind not in (G.VOTE, G.PREVOTE):
        m = G.random_msg(rng, node)
    return False, node, None, None, m


def table_cases(cfg_flags_list=(0, G.CHECK_QUORUM)):
    """The case table of the header crossed with {VOTE, PREVOTE} x {FORCE, not} x {CHECK_QUORUM, not} x {log ahead, equal, behind}
    x {priority lower, equal, higher} x {m.term below, equal, above}: (cfg, node, lead, clock, Msg) on one fixed leader."""
    out = []
    for flags in cfg_flags_list:
        cfg = G.Config(5, flags=flags, seed=9)
        for kind in (G.VOTE, G.PREVOTE):
            for force in (False, True):
                for d_log in (1, 0, -1):
                    for d_prio in (-1, 0, 1):
                        for d_term in (-1, 0, 1, 3):
                            for el in (0, cfg.election_tick - 1):
                                lead = H.fresh_lead(3, L.cfg_word((0, 1, 2), self_slot=0, transferee=1 if d_prio == 0 else None))
                                lead.update(commit=5, term_lo=4, term_hi=7, cur_term=6, dummy_index=0, dummy_term=0, run_count=1,
                                            run_first=[1] + [0] * (H.TERM_RUNS - 1), run_term=[2] + [0] * (H.TERM_RUNS - 1))
                                node = G.Node(cfg, 7)
                                node.load(6, 3, 3, 1, G.FOLLOWER, 2, 0, True)
                                node.self_id = 3
                                clock = L.new_group(3, lead["cfg"], cur_term=6)
                                clock["el"] = el
                                m = G.Msg(kind, 6 + d_term, 12, index=7 + d_log, log_term=6, commit=6, commit_term=6, priority=1 + d_prio, force=force)
                                out.append((cfg, node, lead, clock, m))
    return out
