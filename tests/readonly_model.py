"""ReadIndex restated in Python: the checker of the engine's pending-read queues (CPU and GPU tests).

A restatement of the reference (pingcap/raft-rs v0.6.0; file:line relative to its tree), written from its data structures and
not from the engine's:

    src/read_only.rs:65-139    ReadOnly: pending_read_index (a map ctx -> {index, acks}) + read_index_queue (a deque of ctx)
    src/raft.rs:2056-2091      the MsgReadIndex step of a leader
    src/raft.rs:1805-1818      the read-only half of handle_heartbeat_response
    src/raft.rs:2650-2664      post_conf_change: "the quorum size is now smaller, consider to response some read requests"
    src/raft.rs:957            Raft::reset: replaces the ReadOnly -- at a term change, and at a step-down at the SAME term
    src/tracker.rs:367-372     has_quorum -> vote_result (src/quorum/majority.rs:130-154, src/quorum/joint.rs:56-67)

Contexts are integers here (the host's handles for the context bytes, 0 = empty), peers are slots, and a group's membership is
the engine's configuration word (RG_CFG_*). The one thing the reference does not have is the bound: a queue holds `depth`
reads; a request beyond that is refused with FULL and changes nothing.
"""
NOT_READY, READY, QUEUED, DUPLICATE, FULL = 0, 1, 2, 3, 4
STATUS_NAMES = {NOT_READY: "NOT_READY", READY: "READY", QUEUED: "QUEUED", DUPLICATE: "DUPLICATE", FULL: "FULL"}
ACK_LAST_SELF = 1
WON, PENDING, LOST = "Won", "Pending", "Lost"


def cfg_incoming(c):
    return {s for s in range(8) if (c >> s) & 1}


def cfg_outgoing(c):
    return {s for s in range(8) if (c >> (8 + s)) & 1}


def cfg_self(c):
    return (c >> 16) & 7


def cfg_present(c):
    return {s for s in range(8) if (c >> (24 + s)) & 1}


def majority_vote_result(voters, check):
    """MajorityConfig::vote_result (majority.rs:130-154)."""
    if not voters:
        return WON  # "by convention, the elections on an empty config win"
    yes = missing = 0
    for v in voters:
        r = check(v)
        if r is None:
            missing += 1
        elif r:
            yes += 1
    q = len(voters) // 2 + 1
    if yes >= q:
        return WON
    if yes + missing >= q:
        return PENDING
    return LOST


def joint_vote_result(incoming, outgoing, check):
    """JointConfig::vote_result (joint.rs:56-67)."""
    i, o = majority_vote_result(incoming, check), majority_vote_result(outgoing, check)
    if i == WON and o == WON:
        return WON
    if i == LOST or o == LOST:
        return LOST
    return PENDING


def has_quorum(cfg, acks):
    """ProgressTracker::has_quorum (tracker.rs:367-372): `potential_quorum.get(&id).map(|_| true)` -- in the set = yes, else
    no vote at all."""
    return joint_vote_result(cfg_incoming(cfg), cfg_outgoing(cfg), lambda s: True if s in acks else None) == WON


def is_singleton(cfg):
    """joint.rs:77"""
    return len(cfg_incoming(cfg)) == 1 and not cfg_outgoing(cfg)


class ReadOnly:
    """read_only.rs:65-139 with integer contexts."""

    def __init__(self):
        self.pending_read_index = {}  # ctx -> [index, acks]
        self.read_index_queue = []

    def add_request(self, index, ctx, self_id):
        if ctx in self.pending_read_index:
            return
        self.pending_read_index[ctx] = [index, {self_id}]
        self.read_index_queue.append(ctx)

    def recv_ack(self, id_, ctx):
        rs = self.pending_read_index.get(ctx)
        if rs is None:
            return None
        rs[1].add(id_)
        return rs[1]

    def advance(self, ctx):
        rss = []
        if ctx in self.read_index_queue:
            i = self.read_index_queue.index(ctx)
            for _ in range(i + 1):
                c = self.read_index_queue.pop(0)
                index, _acks = self.pending_read_index.pop(c)
                rss.append((c, index))
        return rss

    def last_pending_request_ctx(self):
        return self.read_index_queue[-1] if self.read_index_queue else None

    def pending_read_count(self):
        return len(self.read_index_queue)


class Group:
    """The leader of one group, as far as reads go. The test owns cfg / commit / term_lo / term and sets them the way its
    scenario moves the engine's columns; a new term goes through set_term (Raft::reset), a step-down at the same term through
    reset (Raft::reset as well)."""

    def __init__(self, cfg, commit=0, term_lo=0, term=0, depth=16):
        self.cfg, self.commit, self.term_lo, self.term, self.depth = cfg, commit, term_lo, term, depth
        self.read_only = ReadOnly()

    def set_term(self, term):
        if term != self.term:
            self.term = term
            self.read_only = ReadOnly()  # raft.rs:957

    def reset(self):
        """Raft::reset(self.term) at the UNCHANGED term -- become_follower(term, INVALID_ID) of a check-quorum step-down
        (raft.rs:1963-1972 -> :1082-1087): `self.read_only = ReadOnly::new(self.read_only.option)` (raft.rs:957) runs
        unconditionally. The queue is empty afterwards and nobody is answered: nothing is emitted."""
        self.read_only = ReadOnly()  # raft.rs:957

    def commit_to_current_term(self):
        return self.commit >= self.term_lo  # raft.rs:581 over the engine's log summary: term(committed) == self.term

    def request(self, ctx, lease=False):
        """raft.rs:2056-2091 -> (status, [read states (ctx, index)])"""
        assert ctx != 0
        if not self.commit_to_current_term():
            return NOT_READY, []
        if is_singleton(self.cfg) or lease:
            return READY, [(ctx, self.commit)]
        if ctx in self.read_only.pending_read_index:
            return DUPLICATE, []  # (the host still broadcasts the heartbeat with this ctx)
        if self.read_only.pending_read_count() == self.depth:
            return FULL, []
        self.read_only.add_request(self.commit, ctx, cfg_self(self.cfg))
        return QUEUED, []

    def ack(self, slot, ctx, flags=0):
        """raft.rs:1805-1818, or with ACK_LAST_SELF raft.rs:2650-2664 -> [read states]"""
        if flags & ACK_LAST_SELF:
            ctx = self.read_only.last_pending_request_ctx()
            if ctx is None:
                return []
            slot = cfg_self(self.cfg)
        else:
            if ctx == 0 or slot not in cfg_present(self.cfg):
                return []
        acks = self.read_only.recv_ack(slot, ctx)
        if acks is None or not has_quorum(self.cfg, acks):
            return []
        return self.read_only.advance(ctx)

    def last_pending(self):
        return self.read_only.last_pending_request_ctx() or 0

    def queue(self):
        """[(ctx, index, acks bitmask)] oldest first"""
        out = []
        for c in self.read_only.read_index_queue:
            index, acks = self.read_only.pending_read_index[c]
            out.append((c, index, sum(1 << s for s in acks)))
        return out


class Shard:
    """G groups and the accumulating list of read states, driven like the engine's entry points."""

    def __init__(self, cfgs, depth):
        self.groups = [Group(int(c), depth=depth) for c in cfgs]
        self.states = []  # (group, ctx, index)

    def read_index(self, reqs, lease=False):
        """reqs: [(group, ctx)] in arrival order -> statuses"""
        st = []
        for g, ctx in reqs:
            s, rs = self.groups[g].request(ctx, lease)
            st.append(s)
            self.states += [(g, c, i) for c, i in rs]
        return st

    def read_acks(self, acks):
        """acks: [(group, slot, ctx, flags)]"""
        for g, slot, ctx, flags in acks:
            self.states += [(g, c, i) for c, i in self.groups[g].ack(slot, ctx, flags)]

    def read_acks_dense(self, ctx_cols):
        """ctx_cols[slot][group]; slots in ascending order per group"""
        for g in range(len(self.groups)):
            for slot in range(len(ctx_cols)):
                self.states += [(g, c, i) for c, i in self.groups[g].ack(slot, int(ctx_cols[slot][g]), 0)]

    def drain(self):
        out, self.states = self.states, []
        return out

    def last_pending(self):
        return [g.last_pending() for g in self.groups]

    def counts(self):
        return [g.read_only.pending_read_count() for g in self.groups]


def by_group(states):
    """The engine's list keeps a group's states in order and says nothing about the order between groups: compare lists after
    a STABLE sort by group."""
    return sorted([tuple(int(x) for x in s) for s in states], key=lambda s: s[0])
