"""The hand-off (include/raftgroups.h: "The hand-off") as a literal Python model: promotion of a followed group that won its
election into a group of the leader engine -- Raft::become_leader (src/raft.rs:1151-1202) with Raft::reset (:942-971) -- and the
demotion that refreshes the arena's log summary from a led group. Citations: pingcap/raft-rs v0.6.0.

The follower side is an elect_model.Node (gate_model's soft state, follower_model's Log); the leader side is a dict of the
leader engine's columns for ONE group:

    commit, term_lo, term_hi, cur_term, dummy_index, dummy_term, run_count        ints
    run_first, run_term                                                            lists of TERM_RUNS ints
    cfg                                                                            the RG_CFG_* word
    pflags, match, next, pr_commit, pend_snap, pend_rs, gid                        lists of P ints (pflags: one byte per slot)

The log arithmetic is done on LISTS OF RUNS (first, term) -- concatenate, append, keep the newest ones -- not on the shifting
tables the kernels use, so that the two are independent restatements."""
import follower_model as F
import gate_model as G

TERM_RUNS = F.TERM_RUNS
FOLLOW_RUNS = TERM_RUNS + 1
LIM = 1 << 63
NONE, DONE, NOT_WON, CONF, NOT_PERSISTED, FAULT = range(6)
OUT_APPENDED, OUT_BECAME_LEADER = 0x8, 0x10
PF_STATE_MASK, PF_PENDING_CONF, PF_PEND_SNAP, PF_PEND_RS = 0x03, 0x20, 0x40, 0x80
PROBE, REPLICATE = 0, 1
LOG_KEYS = ("commit", "term_lo", "term_hi", "cur_term", "dummy_index", "dummy_term", "run_count", "run_first", "run_term")
SLOT_KEYS = ("match", "next", "pr_commit", "pend_snap", "pend_rs", "gid")


def cfg_fields(cfg):
    """(incoming, outgoing, self, transferee + 1, present) of an RG_CFG_* word"""
    return cfg & 0xFF, cfg >> 8 & 0xFF, cfg >> 16 & 7, cfg >> 20 & 0xF, cfg >> 24 & 0xFF


def mask(slots):
    return sum(1 << s for s in slots)


def fresh_lead(P, cfg, sentinel=0):
    """A lead group whose every cell holds `sentinel` (what a test preloads), with the cfg word given."""
    d = {k: sentinel for k in LOG_KEYS[:7]}
    d["run_first"], d["run_term"] = [sentinel] * TERM_RUNS, [sentinel] * TERM_RUNS
    d["run_count"] = 0
    d["cfg"] = cfg
    d["pflags"] = [0] * P
    for k in SLOT_KEYS:
        d[k] = [sentinel] * P
    return d


def copy_lead(d):
    return {k: (list(v) if isinstance(v, list) else v) for k, v in d.items()}


def state_check(c):
    """rg_follow_state_check on a canonical dict: 0 = canonical, else the rule it breaks"""
    runs = c["runs"]
    if len(runs) > FOLLOW_RUNS:
        return 1
    if c["last_index"] >= LIM:
        return 2
    if c["committed"] > c["last_index"] or c["committed"] < c["dummy_index"] or c["last_index"] < c["dummy_index"]:
        return 3
    if c["dummy_index"] == 0 and c["dummy_term"] != 0:
        return 4
    if (len(runs) == 0) != (c["last_index"] == c["dummy_index"]):
        return 5
    prev = (c["dummy_index"], c["dummy_term"])
    for k, (first, term) in enumerate(runs):
        if first <= prev[0]:
            return 6
        if term < prev[1] if k == 0 else term <= prev[1]:
            return 7
        prev = (first, term)
    if runs and runs[-1][0] > c["last_index"]:
        return 8
    return 0


def promote(node, lead, P, persisted=None):
    """One promotion record: (status, term, last_index, commit, out). `lead` changes only where the status is DONE; `node` never
    does. persisted None = the host vouches for persisted == last_index."""
    c = node.log.canonical()
    last = c["last_index"]
    if persisted is None:
        persisted = last
    if node.role != G.FOLLOWER or node.lead != node.self_id or node.self_id == 0:
        return (NOT_WON, 0, 0, 0, 0)
    incoming, outgoing, self_slot, _, present = cfg_fields(lead["cfg"])
    if (mask(node.incoming), mask(node.outgoing), node.self_slot) != (incoming, outgoing, self_slot) or not present >> self_slot & 1 or self_slot >= P:
        return (CONF, 0, 0, 0, 0)
    if persisted != last:
        return (NOT_PERSISTED, 0, 0, 0, 0)
    last_term = c["runs"][-1][1] if c["runs"] else c["dummy_term"]
    if last + 1 >= LIM or not node.term > last_term:
        return (FAULT, 0, 0, 0, 0)
    # the log: F's runs, then the empty entry of term T as a run of its own; the table keeps the newest TERM_RUNS older runs
    runs = list(c["runs"]) + [(last + 1, node.term)]
    older = runs[:-1][-TERM_RUNS:]
    lead["dummy_index"], lead["dummy_term"], lead["commit"] = c["dummy_index"], c["dummy_term"], c["committed"]
    lead["run_first"] = [r[0] for r in older] + [0] * (TERM_RUNS - len(older))
    lead["run_term"] = [r[1] for r in older] + [0] * (TERM_RUNS - len(older))
    lead["run_count"] = len(older)
    lead["term_lo"] = lead["term_hi"] = last + 1
    lead["cur_term"] = node.term
    # reset (raft.rs:942-971): every Progress = Progress::new(last_index + 1) keeping committed_index and commit_group_id;
    # become_leader (:1176-1181): the own one matched = persisted, Replicate, committed_index = committed
    for s in range(P):
        if not present >> s & 1:
            continue
        pb = lead["pflags"][s]
        lead["pend_snap"][s] = 0 if pb & PF_PEND_SNAP else lead["pend_snap"][s]  # (the flag bits are exact)
        lead["pend_rs"][s] = 0 if pb & PF_PEND_RS else lead["pend_rs"][s]
        if s == self_slot:
            lead["match"][s], lead["next"][s], lead["pr_commit"][s] = persisted, persisted + 1, c["committed"]
            lead["pflags"][s] = (pb & PF_PENDING_CONF) | REPLICATE
        else:
            lead["match"][s], lead["next"][s] = 0, last + 1
            lead["pflags"][s] = PROBE
    lead["cfg"] &= ~(0xF << 20)  # abort_leader_transfer (:953)
    return (DONE, node.term, last + 1, c["committed"], OUT_BECAME_LEADER | OUT_APPENDED)


def demote(lead):
    """One demotion record: ((status, term, last_index, commit), canonical dict or None). Nothing of `lead` changes."""
    n = lead["run_count"]
    if n > TERM_RUNS:
        return (FAULT, 0, 0, 0), None
    runs = list(zip(lead["run_first"][:n], lead["run_term"][:n]))
    if lead["term_lo"] <= lead["term_hi"]:
        runs.append((lead["term_lo"], lead["cur_term"]))
    c = {"committed": lead["commit"], "last_index": lead["term_hi"], "dummy_index": lead["dummy_index"], "dummy_term": lead["dummy_term"], "runs": runs}
    if state_check(c):
        return (FAULT, 0, 0, 0), None
    return (DONE, lead["cur_term"], lead["term_hi"], lead["commit"]), c


def log_of(c):
    """A bounded follower_model.Log with the canonical form `c` (the entries of a declared gap take the first known term)."""
    runs = c["runs"]
    known = runs[0][0] if runs else c["dummy_index"] + 1
    terms = [runs[0][1]] * (known - c["dummy_index"] - 1) if runs else []
    for k, (first, term) in enumerate(runs):
        end = runs[k + 1][0] if k + 1 < len(runs) else c["last_index"] + 1
        terms += [term] * (end - first)
    return F.Log(c["dummy_index"], c["dummy_term"], terms, c["committed"], True, known)


# ---- the edge list and the seeded sweep (shared by the CPU and the GPU tests) ----
def canon(dummy_index, dummy_term, runs, last_index, committed=None):
    return {"committed": dummy_index if committed is None else committed, "last_index": last_index, "dummy_index": dummy_index, "dummy_term": dummy_term,
            "runs": list(runs)}


def nine_runs(base=0):
    return [(base + 1 + 3 * k, 2 + k) for k in range(FOLLOW_RUNS)]


# name -> (canonical log, T): the log shapes of the issue's edge list
LOG_EDGES = {
    "empty_dummy0": (canon(0, 0, [], 0), 1),
    "empty_behind_snapshot": (canon(100, 4, [], 100), 6),
    "one_run": (canon(0, 0, [(1, 3)], 7, 5), 4),
    "eight_older_plus_tail": (canon(0, 0, nine_runs(), 30, 28), 20),  # the oldest run is dropped: a gap is declared
    "gap_present": (canon(10, 2, [(15, 4), (18, 6)], 21, 16), 9),
    "last_2_63_minus_2": (canon(LIM - 6, 3, [(LIM - 4, 5)], LIM - 2, LIM - 3), 7),
    "last_2_63_minus_1": (canon(LIM - 6, 3, [(LIM - 4, 5)], LIM - 1, LIM - 3), 7),  # FAULT
}


class Follower:
    """What the model needs of an elect_model.Node, for callers that hold a canonical log (huge indices: no entry list)."""

    def __init__(self, c, term, self_id, incoming, outgoing, self_slot, role=G.FOLLOWER, lead=None):
        self._c = c
        self.term, self.self_id, self.role = term, self_id, role
        self.lead = self_id if lead is None else lead
        self.incoming, self.outgoing, self.self_slot = set(incoming), set(outgoing), self_slot
        self.log = self

    def canonical(self):
        return self._c


def random_canon(rng):
    """A canonical log: 0..FOLLOW_RUNS runs, sometimes above a declared gap, sometimes near 2^63."""
    dummy_index = rng.choice((0, 0, 5, 1000, LIM - 60))
    dummy_term = 0 if dummy_index == 0 else rng.randint(1, 3)
    n = rng.choice((0, 1, 1, 2, 3, 5, TERM_RUNS, FOLLOW_RUNS))
    first = dummy_index + 1 + (rng.randint(1, 4) if n and rng.random() < 0.3 else 0)
    runs, term = [], dummy_term + rng.randint(0 if first == dummy_index + 1 and dummy_term else 1, 2)
    for _ in range(n):
        runs.append((first, term))
        first += rng.randint(1, 5)
        term += rng.randint(1, 3)
    last = first - 1 if n else dummy_index
    return canon(dummy_index, dummy_term, runs, last, rng.randint(dummy_index, last))


def random_case(rng, P):
    """(Follower, lead dict, persisted) for one random promotion: mostly DONE, every refusal now and then."""
    c = random_canon(rng)
    slots = list(range(P))
    self_slot = rng.randrange(P)
    incoming = set(rng.sample(slots, rng.randint(1, P))) | {self_slot}
    outgoing = set(rng.sample(slots, rng.randint(1, P))) if rng.random() < 0.3 else set()
    present = incoming | outgoing | ({s for s in slots if rng.random() < 0.3})
    last_term = c["runs"][-1][1] if c["runs"] else c["dummy_term"]
    term = last_term + rng.randint(1, 3)
    role, lead_id, self_id = G.FOLLOWER, None, rng.randint(1, 9)
    kind = rng.random()
    if kind < 0.05:
        role = rng.choice((G.PRE_CANDIDATE, G.CANDIDATE))
        lead_id = 0
    elif kind < 0.10:
        lead_id = self_id + 1
    elif kind < 0.13:
        self_id, lead_id = 0, 0
    elif kind < 0.18:
        term = last_term - rng.randint(0, 1) if last_term else 0
    f = Follower(c, term, self_id, incoming, outgoing, self_slot, role, lead_id)
    l_in, l_out, l_self, l_present = set(incoming), set(outgoing), self_slot, set(present)
    if 0.18 <= kind < 0.22:
        l_in ^= {rng.randrange(P)}
    elif 0.22 <= kind < 0.25:
        l_out ^= {rng.randrange(P)}
    elif 0.25 <= kind < 0.28 and P > 1:
        l_self = (self_slot + 1) % P
        l_present |= {l_self}
    elif 0.28 <= kind < 0.31:
        l_present -= {self_slot}
    cfg = mask(l_in) | mask(l_out) << 8 | l_self << 16 | (0x80000 if rng.random() < 0.2 else 0) | (rng.randint(1, P) << 20 if rng.random() < 0.3 else 0) | \
        mask(l_present) << 24
    lead = fresh_lead(P, cfg, sentinel=0xAB00000000000000 + rng.randint(0, 99))
    lead["run_count"] = rng.randint(0, TERM_RUNS)
    for s in range(P):
        lead["pflags"][s] = rng.randrange(256)
        lead["gid"][s] = rng.randint(0, 3)
    persisted = c["last_index"] - 1 if 0.31 <= kind < 0.35 and c["last_index"] else None
    return f, lead, persisted


def random_lead_log(rng, lead):
    """Overwrite the log columns of `lead` with a random table: mostly canonical, sometimes not (demotion answers FAULT)."""
    c = random_canon(rng)
    runs = c["runs"]
    tail = bool(runs) and rng.random() < 0.85
    older = runs[:-1] if tail else runs[:TERM_RUNS]
    lead["dummy_index"], lead["dummy_term"], lead["commit"] = c["dummy_index"], c["dummy_term"], c["committed"]
    lead["run_first"] = [r[0] for r in older] + [0] * (TERM_RUNS - len(older))
    lead["run_term"] = [r[1] for r in older] + [0] * (TERM_RUNS - len(older))
    lead["run_count"] = len(older)
    lead["term_hi"] = c["last_index"]
    lead["term_lo"], lead["cur_term"] = (runs[-1][0], runs[-1][1]) if tail else (c["last_index"] + 1, (runs[-1][1] if runs else c["dummy_term"]) + 1)
    bad = rng.random()
    if bad < 0.05:
        lead["commit"] = c["last_index"] + 1
    elif bad < 0.10 and older:
        lead["run_term"][len(older) - 1] = lead["cur_term"] if tail else 0
    elif bad < 0.13:
        lead["run_count"] = TERM_RUNS + 1
    elif bad < 0.16:
        lead["term_hi"] = LIM


# ---- the cases of the GPU tests (tests/test_handoff_gpu.py; tests/test_handoff_host.py checks them against the oracle) ----
SENTINEL = 0x5EED5EED5EED5EED  # what the cells of absent slots are preloaded with
N_FOLLOW = 257
SHAPES = {3: 300, 8: 70}  # slots -> groups of the two leader engines


def make_lead(P, cfg, rng, own_flags=0):
    """A lead group as a previous leadership left it: random Progress cells in the present slots (the PEND bits of the flag
    bytes exact, as the engine keeps them), SENTINEL in every cell of the absent ones, SENTINEL-like junk in the log columns."""
    incoming, outgoing, self_slot, _, present = cfg_fields(cfg)
    d = fresh_lead(P, cfg, sentinel=SENTINEL)
    d["run_count"] = TERM_RUNS  # (derived from run_first on the way in: every row is non-zero)
    for s in range(P):
        if present >> s & 1:
            d["match"][s], d["next"][s], d["pr_commit"][s] = rng.randint(0, 50), rng.randint(1, 60), rng.randint(0, 50)
            d["gid"][s] = rng.randint(1, 3) if cfg & 0x80000 else 0
            d["pend_snap"][s] = rng.choice((0, 0, 17))
            d["pend_rs"][s] = rng.choice((0, 0, 23))
            low = rng.choice((0, 1, 2)) | rng.choice((0, 4)) | rng.choice((0, 8))
            if s == self_slot:
                low |= own_flags
        else:
            low = 0x08
        d["pflags"][s] = low | (PF_PEND_SNAP if d["pend_snap"][s] else 0) | (PF_PEND_RS if d["pend_rs"][s] else 0)
    return d


def existing_route(lead, c, persisted):
    """What a host does today before it raises RG_MF_BECOME_LEADER: the log columns from rg_follow_read's answer `c`, the own
    slot's matched index = persisted. -> a new lead dict"""
    d = copy_lead(lead)
    runs = c["runs"]
    older = runs[:-1]
    d["dummy_index"], d["dummy_term"], d["commit"] = c["dummy_index"], c["dummy_term"], c["committed"]
    d["run_first"] = [r[0] for r in older] + [0] * (TERM_RUNS - len(older))
    d["run_term"] = [r[1] for r in older] + [0] * (TERM_RUNS - len(older))
    d["run_count"] = len(older)
    d["term_lo"], d["cur_term"] = runs[-1] if runs else (c["dummy_index"] + 1, c["dummy_term"])
    d["term_hi"] = c["last_index"]
    d["match"][cfg_fields(lead["cfg"])[2]] = persisted
    return d


class Case:
    def __init__(self, name, g, L, f, lead, persisted=None, expect=DONE):
        self.name, self.g, self.L, self.f, self.lead, self.persisted, self.expect = name, g, L, f, lead, persisted, expect

    def cells(self):
        """(self_id, conf, yes, no) for rg_follow_elect_write, None where the cells stay as rg_follow_elect_enable left them"""
        f = self.f
        return (f.self_id, mask(f.incoming) | mask(f.outgoing) << 8 | f.self_slot << 16, 0, 0) if f.self_id else None

    def soft(self):
        """(term, vote, lead, priority, role, elapsed, timeout, promotable) for rg_follow_soft_write"""
        f = self.f
        return (f.term, f.self_id if f.role != G.PRE_CANDIDATE else 0, f.lead, 0, f.role, 0, 0, 1)


def gpu_cases(P, seed=5):
    """The promoted edges on the P-slot engine: log shapes, configurations and positions of the issue's list."""
    import random
    rng = random.Random(seed * 100 + P)
    Gn, n = SHAPES[P], N_FOLLOW
    E = LOG_EDGES
    if P == 3:
        cfg = mask((0, 1, 2)) | 1 << 16 | 7 << 24
        rows = [("empty_dummy0", 0, 0), ("empty_behind_snapshot", 255, Gn - 1), ("one_run", n - 1, 1), ("eight_older_plus_tail", 100, 10), ("gap_present", 101, 11),
                ("last_2_63_minus_2", 37, 150), ("last_2_63_minus_1", 38, 151)]
        return [Case(name, g, L, Follower(E[name][0], E[name][1], 7, (0, 1, 2), (), 1), make_lead(3, cfg, rng), None,
                     FAULT if name == "last_2_63_minus_1" else DONE) for name, g, L in rows]
    out = []
    # self slot 7 of 8, joint, learners in PRESENT, TRANSFEREE set, RG_PF_PENDING_CONF on the own slot, group commit with gids
    cfg = mask((5, 6, 7)) | mask((4, 5, 7)) << 8 | 7 << 16 | 0x80000 | 5 << 20 | mask((1, 4, 5, 6, 7)) << 24
    c, t = E["one_run"]
    out.append(Case("slot7_joint_learners_transferee_pendingconf_gids", 0, Gn - 1, Follower(c, t, 9, (5, 6, 7), (4, 5, 7), 7), make_lead(8, cfg, rng, PF_PENDING_CONF),
                    c["last_index"]))
    cfg = mask((0, 1, 2)) | 0 << 16 | mask((0, 1, 2, 3, 6)) << 24  # learners 3 and 6
    c, t = E["empty_behind_snapshot"]
    out.append(Case("learners", 255, 0, Follower(c, t, 4, (0, 1, 2), (), 0), make_lead(8, cfg, rng)))
    cfg = mask((0, 1, 2, 3, 4, 5, 6, 7)) | mask((3,)) << 8 | 3 << 16 | 0x80000 | 0xFF << 24
    c, t = E["eight_older_plus_tail"]
    out.append(Case("all_eight_group_commit", n - 1, 1, Follower(c, t, 4, range(8), (3,), 3), make_lead(8, cfg, rng)))
    cfg = mask((2, 4)) | 4 << 16 | 2 << 20 | mask((2, 4)) << 24
    for k, name in enumerate(("gap_present", "last_2_63_minus_2")):  # a neighbouring pair
        c, t = E[name]
        out.append(Case("pair_" + name, 7 + k, 33 + k, Follower(c, t, 5, (2, 4), (), 4), make_lead(8, cfg, rng)))
    return out


def refusal_cases(seed=6):
    """On the 3-slot engine: NOT_WON three ways, CONF five ways, NOT_PERSISTED, FAULT."""
    import random
    rng = random.Random(seed)
    c, t = LOG_EDGES["one_run"]
    good = mask((0, 1, 2)) | 1 << 16 | 7 << 24
    out = []
    for k, (role, lead_id, self_id) in enumerate(((G.CANDIDATE, 0, 7), (G.FOLLOWER, 8, 7), (G.FOLLOWER, 0, 0))):
        out.append(Case("not_won%d" % k, 20 + k, 40 + k, Follower(c, t, self_id, (0, 1, 2), (), 1, role, lead_id), make_lead(3, good, rng), None, NOT_WON))
    # self differs; incoming differs; outgoing differs; the self slot has no Progress; the arena's self slot is beyond the engine's slots
    for k, (cfg, f_self, f_in) in enumerate(((7 | 0 << 16 | 7 << 24, 1, (0, 1, 2)), (3 | 1 << 16 | 7 << 24, 1, (0, 1, 2)), (7 | 4 << 8 | 1 << 16 | 7 << 24, 1, (0, 1, 2)),
                                             (7 | 1 << 16 | 5 << 24, 1, (0, 1, 2)), (7 | 2 << 16 | 7 << 24, 5, (0, 1, 2)))):
        out.append(Case("conf%d" % k, 30 + k, 50 + k, Follower(c, t, 7, f_in, (), f_self), make_lead(3, cfg, rng), None, CONF))
    out.append(Case("not_persisted", 60, 70, Follower(c, t, 7, (0, 1, 2), (), 1), make_lead(3, good, rng), c["last_index"] - 1, NOT_PERSISTED))
    out.append(Case("term_not_above", 61, 71, Follower(c, 3, 7, (0, 1, 2), (), 1), make_lead(3, good, rng), None, FAULT))
    return out
