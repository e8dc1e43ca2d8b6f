"""The leader's clock (include/raftgroups_lead.h) as a literal Python model: one Raft::tick of a group this
store leads, the check-quorum step-down, and the way back into the follower arena. Citations: pingcap/raft-rs v0.6.0.

A led group is a dict of what the engine holds for it:

    tag, hb, el, led            the clock layer's cells: term tag, heartbeat_elapsed, election_elapsed, not STOPPED
    cur_term                    RG_COL_CUR_TERM (the leader's term since become_leader)
    cfg                         the RG_CFG_* word
    pflags                      list of 8 flag bytes (one per slot)
    match, commit               list of P matched indices, the commit index

The reference keeps a role, a lead_transferee and per-peer Progress structs; here `led` is "state == Leader", the TRANSFEREE bits of
the cfg word are lead_transferee and RG_PF_RECENT_ACTIVE of a flag byte is Progress::recent_active. Nothing below is derived from
csrc/rg_lead.h: the functions follow the reference's statements in the reference's order."""
import gate_model as G
import handoff_model as H

PF_RECENT_ACTIVE = 0x08
CHECK_QUORUM, START_LED = 0x1, 0x100
EV_BEAT, EV_CHECK_QUORUM, EV_STEPPED_DOWN, EV_TRANSFER_ABORTED, EV_NEW_TERM = 0x1, 0x2, 0x4, 0x8, 0x10
TICK_MAX = 16383
NO_LEAD = (1 << 64) - 1
SHAPES = {1: 300, 3: H.SHAPES[3], 5: 300, 8: H.SHAPES[8]}  # slots -> groups of the leader engine (257 + a partial block; 70 = one partial block)


class Config:
    """Config::election_tick / heartbeat_tick / check_quorum; validate (src/config.rs:162-171): heartbeat_tick > 0 and
    election_tick > heartbeat_tick."""

    def __init__(self, election_tick, heartbeat_tick, flags=0):
        self.election_tick, self.heartbeat_tick, self.flags = election_tick, heartbeat_tick, flags

    @property
    def check_quorum(self):
        return bool(self.flags & CHECK_QUORUM)

    def valid(self, reserved=0):
        return (2 <= self.election_tick <= TICK_MAX and 1 <= self.heartbeat_tick < self.election_tick and not self.flags & ~(CHECK_QUORUM | START_LED)
                and reserved == 0)


def new_group(P, cfg, cur_term=1, led=True, pflags=None, match=None, commit=0, tag=None):
    return {"tag": cur_term if tag is None else tag, "hb": 0, "el": 0, "led": led, "cur_term": cur_term, "cfg": cfg,
            "pflags": list(pflags) if pflags is not None else [0] * 8, "match": list(match) if match is not None else [0] * P, "commit": commit}


def copy_group(g):
    return {k: (list(v) if isinstance(v, list) else v) for k, v in g.items()}


def majority_has(voters, active):
    """MajorityConfig::vote_result(|id| active.get(id).map(|_| true)) == Won (majority.rs:130-154): an id that is not in the set
    is MISSING, never a rejection; an empty configuration wins."""
    ids = [s for s in range(8) if voters >> s & 1]
    if not ids:
        return True
    yes = sum(1 for s in ids if s in active)
    return yes >= len(ids) // 2 + 1


def quorum_recently_active(g):
    """ProgressTracker::quorum_recently_active(perspective_of = self) (tracker.rs:346-361), has_quorum (:367-372) over the joint
    configuration (joint.rs:56-67: both halves must win)."""
    incoming, outgoing, self_slot, _, present = H.cfg_fields(g["cfg"])
    active = set()
    for s in range(8):  # for (id, pr) in &mut self.progress
        if not present >> s & 1:
            continue
        if s == self_slot:
            g["pflags"][s] |= PF_RECENT_ACTIVE  # pr.recent_active = true (:351)
            active.add(s)
        elif g["pflags"][s] & PF_RECENT_ACTIVE:
            active.add(s)  # (:356) learner or not
            g["pflags"][s] &= ~PF_RECENT_ACTIVE & 0xFF  # pr.recent_active = false (:357)
    return majority_has(incoming, active) and majority_has(outgoing, active)


def abort_leader_transfer(g):
    g["cfg"] &= ~(0xF << 20)  # self.lead_transferee = None (raft.rs:2775-2777)


def step_down_reset(g, read_only=None):
    """What become_follower(term, INVALID_ID) -> reset(term) (raft.rs:942-971, :1082-1087) does to the cells a leader group has:
    both counters 0 (:949-950), abort_leader_transfer (:952), `self.read_only = ReadOnly::new(..)` (:957) -- the pending reads of
    `read_only`, a readonly_model.Group, are dropped unanswered although the term stays --, and the role (:1086). The Progress reset
    (:964-970) is left to the next become_leader, which runs it again."""
    g["el"] = g["hb"] = 0
    abort_leader_transfer(g)
    if read_only is not None:
        read_only.reset()  # :957
    g["led"] = False


def tick(c, g, read_only=None):
    """One rgx_lead_clock of one group -> the event byte. The lazy arming, then Raft::tick_heartbeat (raft.rs:1051-1079).
    read_only: the group's readonly_model.Group where the engine has the ReadIndex layer (a step-down resets it)."""
    ev = 0
    if g["tag"] != g["cur_term"]:  # a new leadership: Raft::reset ran inside become_leader (:1151-1160)
        g["tag"], g["hb"], g["el"], g["led"] = g["cur_term"], 0, 0, True
        ev |= EV_NEW_TERM
    if not g["led"]:  # (Raft::tick runs tick_election for a non-leader: the follower arena's clock, not this one)
        return ev
    g["hb"] += 1  # :1052
    g["el"] += 1  # :1053
    if g["el"] >= c.election_tick:  # :1056
        g["el"] = 0  # :1057
        if c.check_quorum:  # :1058-1062 -> step_leader's MsgCheckQuorum arm (:1963-1973)
            ev |= EV_CHECK_QUORUM
            if not quorum_recently_active(g):  # check_quorum_active (:2763-2766)
                step_down_reset(g, read_only)  # become_follower(term, INVALID_ID) (:1969-1970)
                ev |= EV_STEPPED_DOWN
        if g["led"] and g["cfg"] >> 20 & 0xF:  # :1063-1065
            abort_leader_transfer(g)
            ev |= EV_TRANSFER_ABORTED
    if not g["led"]:  # :1068-1070
        return ev
    if g["hb"] >= c.heartbeat_tick:  # :1072
        g["hb"] = 0  # :1073
        ev |= EV_BEAT  # MsgBeat -> bcast_heartbeat (:1959-1962)
    return ev


def heartbeat_commits(g, P):
    """send_heartbeat's commit (raft.rs:829-839) for every slot: min(pr.matched, raft_log.committed), 0 without a Progress."""
    present = H.cfg_fields(g["cfg"])[4]
    return [min(g["match"][s], g["commit"]) if present >> s & 1 else 0 for s in range(P)]


def cell_refused(c, n_groups, rec, seen):
    """rgx_lead_clock_write's refusals for one record (group, term, election_elapsed, heartbeat_elapsed, led, reserved bytes)."""
    group, _, el, hb, led, reserved = rec
    return group >= n_groups or el >= c.election_tick or hb >= c.heartbeat_tick or led > 1 or any(reserved) or group in seen


def cell_word(g):
    """The clock cell as the engine packs it (only for the twin's input and output)."""
    return g["hb"] | g["el"] << 14 | (0 if g["led"] else 1 << 31)


def step_down(node, lead, clock=None):
    """rgx_follow_step_down of one record: `node` an elect_model.Node-like follower (term, lead, role, self_id, and for a DONE
    answer reset / become_follower of gate_model.Node), `lead` a handoff_model lead dict, `clock` the lead group's clock dict or
    None. -> ((status, term, last_index, commit), canonical log or None); nothing changes unless the status is DONE."""
    if node.role != G.FOLLOWER or node.lead != node.self_id or node.self_id == 0:
        return (H.NOT_WON, 0, 0, 0), None
    if node.term != lead["cur_term"]:
        return (H.FAULT, 0, 0, 0), None
    a, c = H.demote(lead)
    if a[0] != H.DONE:
        return (H.FAULT, 0, 0, 0), None
    node._events = 0
    node.become_follower(node.term, G.INVALID_ID)  # raft.rs:1969-1970
    if clock is not None:  # STOPPED with the tag of the current term: a promotion the clock never saw must not re-arm the group
        if clock["tag"] != lead["cur_term"]:
            clock["tag"], clock["hb"], clock["el"] = lead["cur_term"], 0, 0
        clock["led"] = False
    return a, c


# ---- the edge list and the seeded sweep (shared by the CPU and the GPU tests) ----
def cfg_word(incoming, outgoing=(), self_slot=0, present=None, transferee=None, group_commit=False):
    present = set(incoming) | set(outgoing) if present is None else present
    return (H.mask(incoming) | H.mask(outgoing) << 8 | self_slot << 16 | (0x80000 if group_commit else 0) | ((transferee + 1) << 20 if transferee is not None else 0)
            | H.mask(present) << 24)


def flags_of(active, other=0):
    """Eight flag bytes: RECENT_ACTIVE on the slots of `active`, `other` (bits without RECENT_ACTIVE) everywhere."""
    return [(PF_RECENT_ACTIVE if s in active else 0) | other for s in range(8)]


def edge_groups(P):
    """name -> (cfg word, pflags): the group and config shapes of the issue's list, on P slots (a shape that needs more slots than
    P is left out)."""
    out = {}
    if P >= 3:
        out["quorum_active"] = (cfg_word((0, 1, 2), self_slot=0), flags_of({1}, 0x21))
        out["quorum_lost"] = (cfg_word((0, 1, 2), self_slot=0), flags_of((), 0x21))
        out["self_not_present"] = (cfg_word((0, 1, 2), self_slot=0, present={1, 2}), flags_of({0, 1}))  # the own flag byte is not a Progress: 1 of 3
        out["self_not_present_active"] = (cfg_word((0, 1, 2), self_slot=0, present={1, 2}), flags_of({1, 2}))
        out["learner_active_not_voter"] = (cfg_word((0, 1), self_slot=0, present={0, 1, 2}), flags_of({2}))  # 1 of 2 voters: lost
        out["transferee_active"] = (cfg_word((0, 1, 2), self_slot=1, transferee=2), flags_of({0}))
        out["transferee_lost"] = (cfg_word((0, 1, 2), self_slot=1, transferee=2), flags_of(()))
    if P >= 5:
        out["joint_incoming_only"] = (cfg_word((0, 1, 2), (2, 3, 4), self_slot=0), flags_of({1}))  # outgoing: 1 of 3 -> lost
        out["joint_both"] = (cfg_word((0, 1, 2), (0, 3, 4), self_slot=0), flags_of({1, 3}))
    out["singleton"] = (cfg_word((0,), self_slot=0), flags_of(()))
    out["empty_voters"] = (cfg_word((), self_slot=0, present={0}), flags_of(()))  # has_quorum of an empty config: stays leader
    if P == 8:
        out["slot7"] = (cfg_word((5, 6, 7), self_slot=7, transferee=5), flags_of({6}, 0x43))
    return out


def random_group(rng, P, c):
    """A led group somewhere in its life: mostly between timeouts, often one increment away from one or both."""
    slots = list(range(P))
    self_slot = rng.randrange(P)
    incoming = set(rng.sample(slots, rng.randint(0, P)))
    if rng.random() < 0.8:
        incoming |= {self_slot}
    outgoing = set(rng.sample(slots, rng.randint(1, P))) if rng.random() < 0.3 else set()
    present = incoming | outgoing | {s for s in slots if rng.random() < 0.3}
    if rng.random() < 0.1:
        present -= {self_slot}
    transferee = rng.randrange(P) if rng.random() < 0.3 else None
    g = new_group(P, cfg_word(incoming, outgoing, self_slot, present, transferee, rng.random() < 0.2), cur_term=rng.randint(1, 9))
    g["pflags"] = [rng.randrange(256) if s < P else 0 for s in range(8)]
    g["match"] = [rng.randint(0, 50) for _ in range(P)]
    g["commit"] = rng.randint(0, 50)
    g["el"] = rng.choice((0, c.election_tick - 1, c.election_tick - 1, rng.randrange(c.election_tick)))
    g["hb"] = rng.choice((0, c.heartbeat_tick - 1, c.heartbeat_tick - 1, rng.randrange(c.heartbeat_tick)))
    g["led"] = rng.random() < 0.85
    if rng.random() < 0.1:
        g["tag"] = g["cur_term"] - 1  # a leadership the clock has not seen yet
    return g


SWEEP_CONFIGS = (Config(2, 1, CHECK_QUORUM), Config(5, 1, CHECK_QUORUM), Config(10, 3, CHECK_QUORUM), Config(10, 3, 0), Config(TICK_MAX, TICK_MAX - 1, CHECK_QUORUM),
                 Config(6, 5, 0))


def sweep(seed, n):
    """n (Config, P, group) triples."""
    import random
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        c = rng.choice(SWEEP_CONFIGS)
        P = rng.choice((1, 3, 3, 5, 8))
        out.append((c, P, random_group(rng, P, c)))
    return out
