"""The leader's term gate and the deposition (include/raftgroups_term.h) as a literal Python model: the term check of Raft::step
for the two kinds of record a dense leader tick carries, and the become_follower that follows a higher term. Citations:
pingcap/raft-rs v0.6.0.

    Raft::step, the term gate        src/raft.rs:1282-1411
        m.term == 0: a local message                     :1282-1283
        m.term > self.term                               :1284-1348 (the lease of the vote kinds :1285-1317, the pre-vote
                                                         exception :1319-1330, become_follower(m.term, m.from) for MsgAppend /
                                                         MsgHeartbeat / MsgSnapshot :1340-1344, else become_follower(m.term,
                                                         INVALID_ID) :1346)
        m.term < self.term                               :1349-1410 (only MsgAppend / MsgHeartbeat and MsgRequestPreVote are
                                                         answered; "ignore other cases" -- every response kind -- :1399-1409)
    Raft::reset                      src/raft.rs:942-971 (lead_transferee :952, ReadOnly::new :957)
    Raft::become_follower            src/raft.rs:1082-1087

It COMPOSES the models the other stages have and restates nothing of them: a led group is lead_clock_model's dict (clock cells,
cur_term, cfg word), its pending reads are a readonly_model.Group, the followed group it goes back to is a gate_model.Node, the
log that travels with it is handoff_model's lead dict. Nothing below is derived from csrc/rg_term.h."""
import gate_model as G
import handoff_model as H
import lead_clock_model as L

MF_VALID, MF_REJECT, MF_HAS_RS, MF_INS_FULL, MF_SENT, MF_APPEND, MF_HEARTBEAT, MF_HAS_LOGTERM = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80
RESPONSE_BITS = MF_VALID | MF_REJECT | MF_HAS_RS | MF_HAS_LOGTERM | MF_HEARTBEAT  # what IS the message; SENT / INS_FULL are the host's facts
EV_TRANSFER_ABORTED, EV_STALE, EV_NOT_LED, EV_DEPOSED = 0x08, 0x20, 0x40, 0x80
LOCAL, EQUAL, LOWER, HIGHER = "local", "equal", "lower", "higher"
MSG_KINDS = ("MsgAppendResponse", "MsgHeartbeatResponse")


def is_record(flag):
    """A slot carries a MsgAppendResponse (VALID) or a MsgHeartbeatResponse (HEARTBEAT)."""
    return bool(flag & (MF_VALID | MF_HEARTBEAT))


def term_branch(term, m_term):
    """Which arm of the gate a message of term m_term takes at a node of term `term` (raft.rs:1282, :1284, :1349)."""
    if m_term == 0:
        return LOCAL  # :1282-1283
    if m_term > term:
        return HIGHER  # :1284
    if m_term < term:
        return LOWER  # :1349
    return EQUAL


def led(g):
    """The clock's lazy-arming rule, read only: a tag that differs from RG_COL_CUR_TERM is a leadership the clock has not seen."""
    return g["tag"] != g["cur_term"] or g["led"]


def lead_stop(g, read_only=None):
    """What become_follower(T, INVALID_ID) -> reset (raft.rs:942-971) does to the cells the LEADER engine has for the group, as a
    check-quorum step-down does it: the clock cell stopped under the tag of the current term (lead_clock_model.step_down's rule for
    a leadership the clock never saw), abort_leader_transfer (:952), `self.read_only = ReadOnly::new(..)` (:957). RG_COL_CUR_TERM
    stays. Idempotent. -> EV_TRANSFER_ABORTED or 0"""
    if g["tag"] != g["cur_term"]:
        g["tag"], g["hb"], g["el"] = g["cur_term"], 0, 0
    g["led"] = False
    ev = EV_TRANSFER_ABORTED if g["cfg"] >> 20 & 0xF else 0
    L.abort_leader_transfer(g)  # :952
    if read_only is not None:
        read_only.reset()  # :957
    return ev


def gate(g, flags, terms, P, read_only=None):
    """rgt_lead_gate_device of one group. g: lead_clock_model's dict; flags: the row's 8 flag bytes; terms: Message.term per slot.
    -> (filtered row, events, new_term or None, stale records, records of a not-led group). THE ORDER RULE: the deposing record
    is stepped FIRST; step_follower then ignores every response, so the rest of the row is dropped whatever it holds."""
    row = list(flags)
    records = [s for s in range(P) if is_record(row[s])]
    if not led(g):  # a follower has no arm for the two kinds (step_follower, raft.rs:2257)
        return [0] * 8, EV_NOT_LED, None, 0, len(records)
    branch = {s: term_branch(g["cur_term"], terms[s]) for s in records}
    higher = [terms[s] for s in records if branch[s] == HIGHER]
    if higher:
        new_term = max(higher)  # a lower one of them is stale after the first become_follower, a higher one runs it again (:1346)
        ev = EV_DEPOSED | lead_stop(g, read_only)
        return [0] * 8, ev, new_term, 0, 0
    stale = [s for s in records if branch[s] == LOWER]  # :1399-1409: ignored, nothing is sent
    for s in stale:
        row[s] &= ~RESPONSE_BITS & 0xFF
    return row, (EV_STALE if stale else 0), None, len(stale), 0


def depose(node, lead, new_term, clock=None, read_only=None, soft=True):
    """rgt_follow_depose of one record: `node` a gate_model.Node with self_id (what a win left), `lead` handoff_model's lead dict,
    `clock` / `read_only` the lead group's clock dict / readonly_model.Group or None. soft = False: the scan form, which leaves the
    soft cells to the gated step. -> ((status, term, last_index, commit), canonical log or None); nothing changes unless DONE."""
    if node.role != G.FOLLOWER or node.lead != node.self_id or node.self_id == 0:
        return (H.NOT_WON, 0, 0, 0), None
    if node.term != lead["cur_term"]:
        return (H.FAULT, 0, 0, 0), None
    if soft and new_term <= node.term:
        return (H.FAULT, 0, 0, 0), None
    a, c = H.demote(lead)
    if a[0] != H.DONE:
        return (H.FAULT, 0, 0, 0), None
    if soft:
        node._events = 0
        node.become_follower(new_term, G.INVALID_ID)  # raft.rs:1346
    g = clock if clock is not None else {"tag": lead["cur_term"], "cur_term": lead["cur_term"], "hb": 0, "el": 0, "led": False, "cfg": lead["cfg"]}
    lead_stop(g, read_only)
    lead["cfg"] = g["cfg"]
    return (H.DONE, new_term, a[2], a[3]), c


def scan_selects(node, lead, kind, m_term):
    """rgt_follow_depose_scan_device's selection for a follow group that names `lead`: a message of a kind the dense gated step
    takes, the win state at the lead group's term, a higher term in the record."""
    return (kind in (G.APPEND, G.HEARTBEAT, G.TOUCH) and node.role == G.FOLLOWER and node.lead == node.self_id and node.self_id != 0
            and node.term == lead["cur_term"] and m_term > node.term)


class Leader:
    """A whole Raft in the Leader role, as far as the gate goes: the led group, its pending reads, and the follower it becomes."""

    def __init__(self, node, lead, clock, read_only=None):
        self.node, self.lead, self.clock, self.read_only = node, lead, clock, read_only

    @property
    def state(self):
        return "Leader" if led(self.clock) else "Follower"

    def _depose(self, new_term):
        a, c = depose(self.node, self.lead, new_term, self.clock, self.read_only)
        assert a[0] == H.DONE, a
        self.node.log = H.log_of(c)  # the demotion's log import

    def step_response(self, kind, m_term):
        """Raft::step of a MsgAppendResponse / MsgHeartbeatResponse of term m_term -> 'stepped' | 'ignored' | 'deposed'"""
        assert kind in MSG_KINDS
        flags = [(MF_VALID if kind == MSG_KINDS[0] else MF_HEARTBEAT)] + [0] * 7
        _, ev, new_term, _, _ = gate(self.clock, flags, [m_term] + [0] * 7, 1, self.read_only)
        if ev & EV_DEPOSED:
            self._depose(new_term)
            return "deposed"
        return "ignored" if ev & (EV_STALE | EV_NOT_LED) else "stepped"

    def step_higher(self, m_term, from_id):
        """Raft::step of any OTHER kind of a higher term that is not held back by the lease or the pre-vote exception
        (raft.rs:1340-1347): become_follower(m.term, from_id), from_id = m.from for MsgAppend / MsgHeartbeat / MsgSnapshot, else 0."""
        assert m_term > self.node.term
        self._depose(m_term)
        self.node.lead = from_id  # become_follower's second argument (:1085)
        return "deposed"


# ---- the seeded rows (shared by the CPU and the GPU tests) ----
FLAG_BITS = (MF_VALID, MF_REJECT, MF_HAS_RS, MF_INS_FULL, MF_SENT, MF_APPEND, MF_HEARTBEAT, MF_HAS_LOGTERM)


def random_row(rng, P, cur_term, calm=0.0):
    """(flags[8], terms[8]): every flag bit, terms of 0, below, at and above cur_term; bytes beyond P too (they are not records).
    calm: the share of rows without a higher term."""
    flags, terms = [0] * 8, [0] * 8
    quiet = rng.random() < calm
    for s in range(8):
        r = rng.random()
        if r < 0.3:
            continue
        flags[s] = rng.randrange(256) if r < 0.6 else rng.choice(FLAG_BITS) | rng.choice(FLAG_BITS)
        pick = rng.random()
        terms[s] = 0 if pick < 0.2 else cur_term if pick < 0.6 else rng.randint(max(cur_term - 2, 0), max(cur_term - 1, 0)) if pick < 0.8 else cur_term + rng.randint(1, 3)
        if quiet and terms[s] > cur_term:
            terms[s] = cur_term
    return flags, terms


def random_clock(rng, cfg_word, cur_term):
    """A clock dict in one of the three states the gate tells apart: led, stopped, a tag that differs from RG_COL_CUR_TERM (either
    way round the STOPPED bit)."""
    g = L.new_group(8, cfg_word, cur_term=cur_term)
    g["el"], g["hb"] = rng.randrange(5), rng.randrange(2)
    kind = rng.random()
    if kind < 0.25:
        g["led"] = False
    elif kind < 0.45:
        g["tag"], g["led"] = cur_term - 1, rng.random() < 0.5
    return g
