"""A plain model of the HOST half of the message-at-a-time mirror (rg_set_peers / rg_step / rg_step_heartbeat_response /
rg_local_* / rg_mark_sent / rg_report_* / rg_flush) -- TEST INFRASTRUCTURE ONLY.

Written from INTEGRATION.md section 2 and the reference lines it cites: RawNode::step refuses a response from an id
without a Progress BEFORE Raft::step looks at the term (raw_node.rs:402-411); Raft::step's term gate (raft.rs:1282-1411:
term 0 is a local message and skips it, a higher term makes the leader step down, a lower one is ignored). Per group the
model holds the peer ids, the REGISTERED term (the gate) and the queued flag byte and values of every slot. Every call
answers the error code the engine must answer, the checks in this order: peer lookup, term gate, the own-id drop, slot busy.

flush() turns the queue into an oracle_lib.alloc_msgs() dict, ticks the ORACLE on a state that carries a term table
(oracle_lib.add_term_table: a cur_term per group) and settles the elections of the flush from the oracle's result words:
RG_OUT_BECAME_LEADER (0x10) -- the gate stays at the new term; otherwise it goes back to the term it had when the election
was queued. Nothing of the engine ever feeds the model.

The second half of the file is the driver the road tests share (tests/test_mirror_edges_gpu.py): it makes the same calls on
the model and -- when one is given -- on an engine, and compares the codes. `python tests/mirror_model.py` runs the driver on
every road WITHOUT an engine and checks that model and oracle alone meet the caps the tests assert.
"""
import collections

import numpy as np

import fuzz
import oracle_lib as O

OK, INVALID_ARG, PEER_NOT_FOUND, SLOT_BUSY, HIGHER_TERM, STATE = 0, -1, -5, -6, -7, -8
MF_VALID, MF_REJECT, MF_HAS_RS, MF_INS_FULL, MF_SENT, MF_APPEND, MF_HEARTBEAT, MF_HAS_LOGTERM = 1, 2, 4, 8, 16, 32, 64, 128
MF_BECOME_LEADER = MF_REJECT  # on the leader's own slot (new term in m_hint)
OUT_FAULT, OUT_BECAME_LEADER = 0x2, 0x10
F, MI, MC, MH, MRS, MLT = range(6)  # one queued cell: flag byte, m_index, m_commit, m_hint, m_rs, m_logterm

Flushed = collections.namedtuple("Flushed", "gout dirty n_records accepted refused")


class Mirror:
    def __init__(self, st, max_inflight=0):
        """st: an oracle_lib state dict WITH a term table; the model owns it (and the oracle cluster loaded from it)."""
        assert "cur_term" in st
        self.G, self.P = st["n_groups"], st["n_slots"]
        self.st, self.max_inflight = st, max_inflight
        self._load()
        self.registered = False  # rg_set_peers was called at least once
        self.peers = [[0] * 8 for _ in range(self.G)]
        self.terms = [0] * self.G
        self.queue = {}      # group -> {slot: cell}; a group is listed iff one of its flag bytes is not 0
        self.elections = []  # (group, the term its gate had) of the pending flush
        self.msgs = O.alloc_msgs(self.G, self.P)
        self.gout = np.zeros(self.G, dtype=np.uint32)

    def _load(self):
        self.cl = O.Cluster(self.G)
        self.cl.load_soa(self.st, term=0, max_inflight=self.max_inflight)  # (the term table gives every group its own term)
        if self.max_inflight:
            self.cl.set_own_inflights(True)
        self.self_slot = ((self.st["cfg"] >> 16) & 7).astype(np.int64).tolist()

    # ---- the oracle's side -------------------------------------------------------------------------
    def state(self):
        self.cl.store_soa(self.st)
        return self.st

    def cur_term(self, g):
        return int(self.cl.L.ro_group_term(self.cl.h, g))

    def last_index(self, g):
        return int(self.cl.last_index(g))

    def committed(self, g):
        return int(self.cl.committed(g))

    def snapshot(self):
        """What rg_checkpoint images: the device's columns. The mirror's tables are NOT part of it."""
        return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in self.state().items()}

    def restore(self, image):
        self.st = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in image.items()}
        self._load()

    def permute(self, perm):
        """rg_permute_groups: position i takes old position perm[i] -- columns, peer ids and gates alike; refused while
        anything is queued."""
        if self.registered and self.queue:
            return SLOT_BUSY
        st, G = self.state(), self.G
        p = np.asarray(perm, dtype=np.int64)
        for k in ("match", "next", "pr_commit", "pend_snap", "pend_rs", "gid", "run_first", "run_term"):
            st[k][:, :G] = st[k][:, p]
        for k in ("pflags", "commit", "term_lo", "term_hi", "cfg", "dummy_index", "dummy_term", "cur_term"):
            st[k][:] = st[k][p]
        self.peers = [self.peers[int(i)] for i in p]
        self.terms = [self.terms[int(i)] for i in p]
        self._load()
        return OK

    # ---- the calls -----------------------------------------------------------------------------------
    def set_peers(self, g, ids, term):
        if not 0 <= g < self.G or len(ids) > self.P:
            return INVALID_ARG
        self.registered = True
        self.peers[g] = [int(ids[i]) if i < len(ids) else 0 for i in range(8)]
        self.terms[g] = int(term)
        return OK

    def _find(self, g, pid):
        if pid == 0:  # id 0 is illegal (raw_node.rs:303): never found, not even on an unused slot
            return None
        for s in range(self.P):
            if self.peers[g][s] == pid:
                return s
        return None

    def _cell(self, g, s):
        return self.queue.setdefault(g, {}).setdefault(s, [0, 0, 0, 0, 0, 0])

    def _flags(self, g, s):
        return self.queue.get(g, {}).get(s, (0,))[F]

    def _response(self, g, from_, term):
        """The four checks every response passes, in order -> (code, slot); slot is None where the call ends."""
        if not 0 <= g < self.G:
            return INVALID_ARG, None
        if not self.registered:
            return STATE, None
        s = self._find(g, from_)
        if s is None:                      # 1. peer lookup (raw_node.rs:407-410)
            return PEER_NOT_FOUND, None
        if term != 0:                      # 2. term gate (raft.rs:1282-1411); term 0 skips it
            if term > self.terms[g]:
                return HIGHER_TERM, None
            if term < self.terms[g]:
                return OK, None
        if s == self.self_slot[g]:         # 3. the leader's own id: dropped (its REJECT bit is RG_MF_BECOME_LEADER)
            return OK, None
        if self._flags(g, s) & (MF_VALID | MF_HEARTBEAT):  # 4. one response per peer and flush
            return SLOT_BUSY, None
        return OK, s

    def step(self, g, from_, term, index, commit=0, reject=False, reject_hint=0, request_snapshot=0, ins_full=False,
             log_term=0):
        code, s = self._response(g, from_, term)
        if s is None:
            return code
        c = self._cell(g, s)
        c[MI], c[MC], c[MH], c[MRS], c[MLT] = index, commit, reject_hint, request_snapshot, log_term
        c[F] |= MF_VALID | (MF_REJECT if reject else 0) | (MF_HAS_RS if request_snapshot else 0) | \
            (MF_INS_FULL if ins_full else 0) | (MF_HAS_LOGTERM if reject and log_term else 0)
        return OK

    def step_heartbeat_response(self, g, from_, term, commit=0, ins_full=False):
        code, s = self._response(g, from_, term)
        if s is None:
            return code
        c = self._cell(g, s)
        c[MC] = commit
        c[F] |= MF_HEARTBEAT | (MF_INS_FULL if ins_full else 0)
        return OK

    def _local(self, g):
        if not 0 <= g < self.G:
            return INVALID_ARG
        return OK if self.registered else STATE

    def local_append(self, g, new_last_index):
        code = self._local(g)
        if code:
            return code
        c = self._cell(g, self.self_slot[g])  # (a second call replaces the first: the newest last index counts)
        c[MC] = new_last_index
        c[F] |= MF_APPEND
        return OK

    def local_persisted(self, g, index):
        code = self._local(g)
        if code:
            return code
        if self._flags(g, self.self_slot[g]) & MF_VALID:
            return SLOT_BUSY
        c = self._cell(g, self.self_slot[g])
        c[MI] = index
        c[F] |= MF_VALID
        return OK

    def local_become_leader(self, g, term):
        code = self._local(g)
        if code:
            return code
        if term <= self.terms[g]:
            return INVALID_ARG
        if g in self.queue:  # whatever is queued belongs to the old term (a second election included)
            return SLOT_BUSY
        c = self._cell(g, self.self_slot[g])
        c[MH] = term
        c[F] |= MF_BECOME_LEADER
        self.elections.append((g, self.terms[g]))
        self.terms[g] = int(term)  # responses of the new term pass from now on; flush() settles
        return OK

    def mark_sent(self, g, pid):
        code = self._local(g)
        if code:
            return code
        s = self._find(g, pid)
        if s is None:
            return PEER_NOT_FOUND
        if s != self.self_slot[g]:  # (the leader sends itself nothing)
            self._cell(g, s)[F] |= MF_SENT
        return OK

    def _report(self, g, pid, apply):
        code = self._local(g)
        if code:
            return code
        s = self._find(g, pid)
        if s is None:  # "no progress available": ignored (raw_node.rs:692-709 drops the step's result)
            return OK
        if g in self.queue:  # local messages apply in call order: flush first
            return SLOT_BUSY
        apply(s + 1)
        return OK

    def report_unreachable(self, g, pid):
        return self._report(g, pid, lambda i: self.cl.L.ro_handle_unreachable(self.cl.h, g, i))

    def report_snapshot(self, g, pid, failure):
        return self._report(g, pid, lambda i: self.cl.L.ro_handle_snapshot_status(self.cl.h, g, i, bool(failure)))

    # ---- the flush -----------------------------------------------------------------------------------
    def n_records(self):
        return sum(1 for cells in self.queue.values() for c in cells.values() if c[F])

    def flush(self):
        if not self.registered:
            return STATE
        m, n = self.msgs, self.n_records()
        m["m_flags"][...] = 0
        for g, cells in self.queue.items():
            for s, c in cells.items():
                m["m_flags"][g, s] = c[F]
                m["m_index"][s, g], m["m_commit"][s, g], m["m_hint"][s, g] = c[MI], c[MC], c[MH]
                m["m_rs"][s, g], m["m_logterm"][s, g] = c[MRS], c[MLT]
        self.gout[:] = 0
        self.cl.tick_soa(m, self.gout)
        accepted, refused = [], []
        for g, old in reversed(self.elections):
            if int(self.gout[g]) & OUT_BECAME_LEADER:
                accepted.append(g)
            else:
                refused.append(g)
                self.terms[g] = old
        dirty = np.array(sorted(self.queue), dtype=np.uint64)
        self.queue, self.elections = {}, []
        return Flushed(self.gout.copy(), dirty, n, accepted, refused)


# =====================================================================================================
# the driver: the same calls on the model and (when there is one) on an engine
# =====================================================================================================
TERM = 5  # every group is loaded at this term; the first round of elections spreads them


def peer_id(g, s):
    """Every group has peer ids of its own (a table that moved terms but not ids, or the reverse, answers wrongly)."""
    return 1000 * (g + 1) + 10 * s + 3


def make_state(seed, G, P):
    rng = np.random.default_rng(seed)
    st = O.add_term_table(O.alloc_state(G, P))
    st["cfg"][:] = fuzz.random_cfg(rng, G, P)
    fuzz.random_state(rng, st, small_values=True)
    fuzz.random_term_table(rng, st, TERM, max_runs=2)  # (room for the elections: no reject is handed back to the host)
    return st


class Both:
    """Makes every call on the model and on the engine (if any) and compares the codes."""

    def __init__(self, model, eng=None):
        self.model, self.eng = model, eng
        self.codes = collections.Counter()

    def call(self, name, *a, **kw):
        want = getattr(self.model, name)(*a, **kw)
        if self.eng is not None:
            try:
                getattr(self.eng, name)(*a, **kw)
                got = OK
            except RuntimeError as e:  # raft_rs_amd.EngineError
                got = e.code
            assert got == want, (name, a, kw, "engine", got, "model", want)
        self.codes[name, want] += 1
        return want

    def ok(self, name, *a, **kw):
        code = self.call(name, *a, **kw)
        assert code == OK, (name, a, kw, code)


def ids_of(model, g):
    return [peer_id(g, s) for s in range(model.P)]


def register_all(both, term=TERM):
    for g in range(both.model.G):
        both.ok("set_peers", g, ids_of(both.model, g), term)


def first_round(both):
    """Well-formed elections at different terms: afterwards the groups' terms differ (TERM + 1 .. TERM + 7)."""
    for g in range(both.model.G):
        both.ok("local_become_leader", g, TERM + 1 + g % 7)


def warm_up(both, acks):
    """Every group proposes two entries and persists them; with `acks` every peer acknowledges them at the group's term
    (Probe -> Replicate), without, the send stage of an engine with device Inflights fills its windows."""
    m = both.model
    for g in range(m.G):
        last = m.last_index(g) + 2
        both.ok("local_append", g, last)
        both.ok("local_persisted", g, last)
        for s in range(m.P):
            if acks and s != m.self_slot[g]:
                both.ok("step", g, peer_id(g, s), m.terms[g], last, commit=m.committed(g))


def ordinary(both, rng, g, fill, host_inflights):
    """Kind (d): traffic of the registered term -- accepts, rejects, heartbeat responses, proposals, sent marks."""
    m = both.model
    last, t, me = m.last_index(g), m.terms[g], m.self_slot[g]
    if fill or rng.random() < 0.6:
        new_last = last + int(rng.integers(0, 3))
        both.ok("local_append", g, new_last)
        both.ok("local_persisted", g, new_last - int(rng.integers(0, 2)) if new_last else 0)
        last = new_last
    for s in range(m.P):
        if s == me or not (fill or rng.random() < 0.7):
            continue
        pid, r = peer_id(g, s), rng.random()
        full = bool(host_inflights and rng.random() < 0.1)
        if host_inflights and rng.random() < 0.4:
            both.ok("mark_sent", g, pid)
        if r < 0.2:
            both.ok("step_heartbeat_response", g, pid, t, int(rng.integers(0, last + 1)), ins_full=full)
        elif r < 0.35:
            idx = int(rng.integers(0, last + 2))
            both.ok("step", g, pid, t, idx, reject=True, reject_hint=int(rng.integers(0, idx + 1)),
                    request_snapshot=int(rng.integers(1, 30)) if rng.random() < 0.1 else 0, ins_full=full)
        else:
            idx = int(rng.integers(max(0, last - 6), last + 1))
            both.ok("step", g, pid, t, idx, commit=min(idx, m.committed(g)), ins_full=full)
    if g not in m.queue:  # (every group of the flush carries something)
        both.ok("local_append", g, last + 1)


def won_election(both, rng, g, term, fill):
    """Kind (c): the documented way to win an election in ONE flush -- rg_local_become_leader, then the proposals, the
    persisted index and the peers' responses of the NEW term behind it. (Where the device refuses the election, what is
    queued behind it is applied as ordinary messages of the old term's Progress set.)"""
    m = both.model
    last, me = m.last_index(g), m.self_slot[g]
    both.ok("local_become_leader", g, term)
    assert m.terms[g] == term
    both.ok("local_append", g, last + 3)  # (become_leader's empty entry is last + 1)
    both.ok("local_persisted", g, last + 1)
    for s in range(m.P):
        if s != me and (fill or rng.random() < 0.8):
            if rng.random() < 0.2:
                both.ok("step_heartbeat_response", g, peer_id(g, s), term, m.committed(g))
            else:
                both.ok("step", g, peer_id(g, s), term, last + 1, commit=m.committed(g))


def road_events(both, rng, touched, fill=False, host_inflights=True):
    """One flush with the four kinds of group -> {kind: [groups]}. fill: every slot of every (c) / (d) group carries an
    event and (a) / (b) are 8 groups each (the record count is the point)."""
    m = both.model
    groups = [int(g) for g in rng.choice(m.G, size=touched, replace=False)]
    n = 8 if fill else touched // 5
    kinds = {"a": groups[:n], "b": groups[n:2 * n]}
    rest = groups[2 * n:]
    k = len(rest) // 3 if fill else n
    kinds.update(c_acc=rest[:k], c_ref=rest[k:2 * k], d=rest[2 * k:])
    cur = {g: m.cur_term(g) for g in groups}
    for g in kinds["b"] + kinds["c_ref"]:
        # RG_COL_CUR_TERM and the registered term came apart (a reloaded column, a restore): the host believes an older term
        both.ok("set_peers", g, ids_of(m, g), cur[g] - 2)
    for g in kinds["a"]:
        both.ok("local_become_leader", g, cur[g] + 1 + g % 3)
    for g in kinds["b"]:
        both.ok("local_become_leader", g, cur[g] - g % 2)  # above the registered term, not above the device's
    for g in kinds["c_acc"]:
        won_election(both, rng, g, cur[g] + 2, fill)
    for g in kinds["c_ref"]:
        won_election(both, rng, g, cur[g] - g % 2, fill)
    for g in kinds["d"]:
        ordinary(both, rng, g, fill, host_inflights)
    behind = set(kinds["b"] + kinds["c_ref"])
    kinds["registered"] = {g: (cur[g] - 2 if g in behind else cur[g]) for g in groups}
    kinds["touched"] = groups
    return kinds


def check_caps(kinds, res, least=8):
    """The conditions that keep a road test honest, from the ORACLE's result words."""
    acc, ref = set(res.accepted), set(res.refused)
    assert len(acc) >= 2 * least and len(ref) >= 2 * least, (len(acc), len(ref))
    for k in ("a", "b", "c_acc", "c_ref", "d"):
        assert len(kinds[k]) >= least, (k, len(kinds[k]))
    assert set(kinds["a"]) | set(kinds["c_acc"]) == acc, "every well-formed election is accepted, no other"
    assert set(kinds["b"]) | set(kinds["c_ref"]) == ref, "every stale election is refused, no other"
    for g in ref:
        assert int(res.gout[g]) & OUT_FAULT, g
    assert sorted(res.dirty.tolist()) == sorted(kinds["touched"])


def probe_and_answer(both, rng, kinds, res):
    """The gate after the flush, probed on every election group and on 16 quiet ones: term + 1 answers RG_ERR_HIGHER_TERM,
    term - 1 is dropped (RG_OK, nothing queued: the quiet groups stay out of the next flush's result list), a response AT
    the term is queued (its repeat answers RG_ERR_SLOT_BUSY). The election groups' peers then all answer at the term the
    gate holds -- the old one where the device refused, the new one where it accepted. -> the groups the next flush lists."""
    m = both.model
    elect = res.accepted + res.refused
    in_flush = set(kinds["touched"])
    quiet = [g for g in (int(x) for x in rng.permutation(m.G)) if g not in in_flush][:16]
    for g in res.accepted:
        assert m.terms[g] == m.cur_term(g) > kinds["registered"][g], g
    for g in res.refused:
        assert m.terms[g] == kinds["registered"][g] < m.cur_term(g), g
    for g in elect + quiet:
        t = m.terms[g]
        assert t >= 2
        pid = m.peers[g][(m.self_slot[g] + 1) % m.P]  # (the ids the position answers to: they move with a permutation)
        assert both.call("step", g, pid, t + 1, m.last_index(g)) == HIGHER_TERM
        assert both.call("step", g, pid, t - 1, m.last_index(g)) == OK
        assert both.call("step_heartbeat_response", g, pid, t + 1) == HIGHER_TERM
        assert both.call("step_heartbeat_response", g, pid, t - 1) == OK
        assert g not in m.queue
    for g in elect:
        t, last = m.terms[g], m.last_index(g)
        for s in range(m.P):
            if s != m.self_slot[g]:
                both.ok("step", g, m.peers[g][s], t, last, commit=m.committed(g))
        if m.P > 1:
            assert both.call("step", g, m.peers[g][(m.self_slot[g] + 1) % m.P], t, last) == SLOT_BUSY
    return sorted(elect) if m.P > 1 else []


# G, P, groups touched, every slot filled: the smallest shapes that select each road of a flush (rg_flush_impl /
# rg_sparse_roundtrip; RG_INGEST_BLOCK = 256 records, RG_ZEROCOPY_MAX = 1024 groups, RG_ROUNDTRIP_MAX = 16384 records, and
# the dense tick from half of G on)
ROADS = {
    "one_launch": (2100, 5, 40, False),
    "pinned_list": (2100, 5, 300, False),
    "copied_list": (6000, 7, 1100, False),
    "three_call": (6000, 7, 2500, True),
    "dense": (2100, 5, 1100, False),
    "mailbox": (2100, 5, 40, False),
}
INGEST_BLOCK, ZEROCOPY_MAX, ROUNDTRIP_MAX = 256, 1024, 16384


def check_road_shape(road, G, res):
    """Does the flush `res` select the road? (the rules of rg_flush_impl and rg_sparse_roundtrip, restated)"""
    n_groups, n_rec = len(res.dirty), res.n_records
    if road == "dense":
        assert n_groups * 2 >= G
        return
    assert n_groups * 2 < G, "half of G or more goes through the dense tick"
    if road in ("one_launch", "mailbox"):
        assert n_rec <= INGEST_BLOCK
    elif road == "pinned_list":
        assert n_rec > INGEST_BLOCK and min(n_rec, G) <= ZEROCOPY_MAX
    elif road == "copied_list":
        assert min(n_rec, G) > ZEROCOPY_MAX and n_rec <= ROUNDTRIP_MAX
    else:
        assert n_rec > ROUNDTRIP_MAX


def drive_road(both, road, flush, seed, host_inflights=True, before_road=None):
    """The whole sequence of one road: registration, the first round of elections, two warm-up rounds, the road's flush with
    the four kinds of group, the gate probe and the second flush. flush(tag) flushes the engine (if any) and the model,
    compares them and returns the model's Flushed."""
    m = both.model
    G, P, touched, fill = ROADS[road]
    assert (m.G, m.P) == (G, P)
    rng = np.random.default_rng(seed)
    register_all(both)
    first_round(both)
    res = flush("first round")
    assert len(res.accepted) == G and len({m.cur_term(g) for g in range(G)}) == 7
    warm_up(both, acks=True)
    flush("warm-up 1")
    warm_up(both, acks=False)
    flush("warm-up 2")
    if before_road:
        before_road(rng)
    kinds = road_events(both, rng, touched, fill, host_inflights)
    res = flush(road)
    check_caps(kinds, res)
    check_road_shape(road, G, res)
    listed = probe_and_answer(both, rng, kinds, res)
    res2 = flush("second flush")
    assert res2.dirty.tolist() == listed, "only the groups whose peers answered AT the gate's term are in the next flush"
    assert not res2.accepted and not res2.refused
    return kinds, res, res2


if __name__ == "__main__":
    # the seeds and shapes meet the caps with the model and the oracle alone (no engine)
    for road_ in ROADS:
        for inflights_ in (0, 3):
            if inflights_ and ROADS[road_][0] != 2100:
                continue
            G_, P_ = ROADS[road_][:2]
            model_ = Mirror(make_state(77, G_, P_), max_inflight=inflights_)
            both_ = Both(model_)
            if inflights_:
                def flush_(tag, model_=model_):
                    r = model_.flush()
                    model_.cl.send_stage_soa(r.gout, 1)
                    return r
            else:
                def flush_(tag, model_=model_):
                    return model_.flush()
            kinds_, res_, res2_ = drive_road(both_, road_, flush_, seed=100 + len(road_), host_inflights=not inflights_)
            print(f"{road_:12s} inflights={inflights_}: groups {len(res_.dirty)}, records {res_.n_records}, accepted "
                  f"{len(res_.accepted)}, refused {len(res_.refused)}, kinds "
                  f"{ {k: len(kinds_[k]) for k in ('a', 'b', 'c_acc', 'c_ref', 'd')} }, second flush {len(res2_.dirty)} groups")
    print("mirror_model self-check ok")
