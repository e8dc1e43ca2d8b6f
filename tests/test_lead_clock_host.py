"""CPU only: the leader's clock and the step-down. (1) tests/lead_clock_model.py restates the reference line by line; (2) its quorum
half and its heartbeat commits equal the oracle's; (3) three of the reference's tests run as scenarios on it; (4) the arithmetic of
csrc/rg_lead.h -- what the kernels run -- is compiled for the HOST with g++ (tests/host_check/lead_clock_twin.cpp, a stand-alone
program) and diffed against the model on the edge list and over a seeded sweep, then once more under AddressSanitizer + UBSan, run
directly; (5) what the sweep contains is asserted from the model alone; (6) every new name is declared, exported and bound, and the
refusals are host checks; (7) the kernels carry no scratch (tools/kernel_resources.py).

Citations: pingcap/raft-rs v0.6.0."""
import ctypes
import os
import random
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import gate_model as G
import handoff_model as H
import lead_clock_model as L

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_NAMES = ("rgx_lead_version", "rgx_lead_clock_enable", "rgx_lead_clock_write", "rgx_lead_clock_read", "rgx_lead_clock", "rgx_lead_clock_counts", "rgx_follow_step_down",
             "rgx_follow_step_down_device")
SWEEP = 6000
GATE = G.Config(5, 5, 12, G.CHECK_QUORUM, seed=91)


def build_twin(tmp_path, name, extra):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build the host twin")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, os.path.join(HERE, "host_check", "lead_clock_twin.cpp"), "-o", exe])
    return exe


def row_of(pflags):
    return sum(b << (8 * s) for s, b in enumerate(pflags))


def tick_line(c, P, g):
    return "T %d %d %d %d %d %d %d %d %d %d %s" % (c.election_tick, c.heartbeat_tick, c.flags & L.CHECK_QUORUM, L.cell_word(g), g["tag"], g["cur_term"], g["cfg"],
                                                  row_of(g["pflags"]), P, g["commit"], " ".join("%d" % x for x in g["match"] + [0] * (8 - P)))


def edge_ticks():
    """(name, Config, P, group): every shape of lead_clock_model.edge_groups at every position of the two counters that matters --
    between timeouts, at the heartbeat timeout, at the election timeout, at both --, check quorum on and off, led and stopped, armed
    and not; the smallest and the largest tick values."""
    out = []
    for c in (L.Config(2, 1, L.CHECK_QUORUM), L.Config(2, 1, 0), L.Config(6, 3, L.CHECK_QUORUM), L.Config(6, 3, 0), L.Config(L.TICK_MAX, 7, L.CHECK_QUORUM),
              L.Config(L.TICK_MAX, L.TICK_MAX - 1, L.CHECK_QUORUM)):
        for P in (1, 3, 5, 8):
            for name, (cfg, pflags) in L.edge_groups(P).items():
                for el in sorted({0, c.election_tick - 2, c.election_tick - 1}):
                    for hb in sorted({0, c.heartbeat_tick - 1}):
                        for led, stale in ((True, False), (False, False), (False, True), (True, True)):
                            g = L.new_group(P, cfg, cur_term=4, led=led, pflags=pflags, match=[7 + 3 * s for s in range(P)], commit=12, tag=3 if stale else 4)
                            g["el"], g["hb"] = el, hb
                            out.append(("%s/%d/%d/%d" % (name, el, hb, led + 2 * stale), c, P, g))
    return out


def named_sweep(seed, n):
    return [("sweep%d" % k, c, P, g) for k, (c, P, g) in enumerate(L.sweep(seed, n))]


def run_ticks(exe, cases):
    """Every case through the twin and the model. -> the model's event bytes"""
    lines = [tick_line(c, P, g) for _, c, P, g in cases]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    got = out.stdout.split("\n")[:-1]
    assert len(got) == len(cases)
    events = []
    for line, (name, c, P, g) in zip(got, cases):
        m = L.copy_group(g)
        ev = L.tick(c, m)
        hb = L.heartbeat_commits(m, P) + [0] * (8 - P)
        want = [ev, L.cell_word(m), m["tag"], m["cfg"], row_of(m["pflags"])] + hb
        w = line.split()
        assert w[0] == "T" and [int(x) for x in w[1:]] == want, (name, line, want)
        events.append(ev)
    return events


def step_down_cases(seed, n):
    """(node, lead dict) pairs: a soft state that is mostly what a win left, over a lead group whose log is mostly canonical."""
    rng = random.Random(seed)
    out = []
    for k in range(n):
        _, lead, _ = H.random_case(rng, 3)
        H.random_lead_log(rng, lead)
        node = G.Node(GATE, rng.randrange(1 << 20))
        self_id = rng.randint(1, 9)
        kind = rng.random()
        role, lead_id, term = G.FOLLOWER, self_id, lead["cur_term"]
        if kind < 0.05:
            role, lead_id = rng.choice((G.PRE_CANDIDATE, G.CANDIDATE)), 0
        elif kind < 0.10:
            lead_id = self_id + 1
        elif kind < 0.13:
            self_id = lead_id = 0
        elif kind < 0.20:
            term = lead["cur_term"] + rng.choice((-1, 1))
        node.load(max(term, 0), self_id, lead_id, 0, role, rng.randrange(GATE.min_timeout), rng.randrange(GATE.min_timeout, GATE.max_timeout), rng.random() < 0.8)
        node.self_id = self_id
        out.append((node, lead))
    return out


def run_step_downs(exe, cases):
    lines, want = [], []
    for node, lead in cases:
        clock = node.elapsed | int(node.promotable) << 15 | node.timeout << 16
        lines.append("S %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %s %s" % (
            node.role, node.lead, node.self_id, node.term, clock, GATE.seed, GATE.min_timeout, GATE.max_timeout, node.group, lead["commit"], lead["term_lo"],
            lead["term_hi"], lead["cur_term"], lead["dummy_index"], lead["dummy_term"], lead["run_count"], " ".join("%d" % x for x in lead["run_first"]),
            " ".join("%d" % x for x in lead["run_term"])))
        before_lead, before_soft = H.copy_lead(lead), node.soft()
        a, c = L.step_down(node, lead)
        assert lead == before_lead
        if a[0] != H.DONE:
            assert node.soft() == before_soft
            want.append([a[0]])
        else:
            assert (node.term, node.vote, node.role, node.lead, node.elapsed) == (before_soft[0], before_soft[1], G.FOLLOWER, 0, 0)
            assert GATE.min_timeout <= node.timeout < GATE.max_timeout
            new_clock = int(node.promotable) << 15 | node.timeout << 16
            want.append([a[0], a[1], a[2], a[3], 0, new_clock, 2 | (4 if new_clock != clock else 0)])
    out = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    got = out.stdout.split("\n")[:-1]
    assert len(got) == len(cases)
    for line, w in zip(got, want):
        assert line.split()[0] == "S" and [int(x) for x in line.split()[1:]] == w, (line, w)
    return [w[0] for w in want]


WRITE_EDGES = (  # (election_tick, heartbeat_tick, election_elapsed, heartbeat_elapsed, led, reserved bytes) -> refused?
    ((10, 3, 9, 2, 1, (0,) * 7), False), ((10, 3, 0, 0, 0, (0,) * 7), False), ((10, 3, 10, 0, 1, (0,) * 7), True), ((10, 3, 0, 3, 1, (0,) * 7), True),
    ((10, 3, 0, 0, 2, (0,) * 7), True), ((10, 3, 0, 0, 1, (0, 0, 0, 0, 0, 0, 1)), True), ((10, 3, 0, 0, 1, (1, 0, 0, 0, 0, 0, 0)), True),
    ((L.TICK_MAX, L.TICK_MAX - 1, L.TICK_MAX - 1, L.TICK_MAX - 2, 1, (0,) * 7), False), ((2, 1, 1, 0, 1, (0,) * 7), False), ((2, 1, 1, 1, 1, (0,) * 7), True))
CONFIG_EDGES = (((2, 1, 0, 0), True), ((1, 1, 0, 0), False), ((2, 2, 0, 0), False), ((2, 0, 0, 0), False), ((L.TICK_MAX, L.TICK_MAX - 1, 0x101, 0), True),
                ((L.TICK_MAX + 1, 1, 0, 0), False), ((10, 3, 2, 0), False), ((10, 3, 1, 1), False), ((10, 9, 0x100, 0), True))


def composed_group(rng, depth):
    """One group of the composed sweep: a led group of lead_clock_model.random_group one increment before its election timeout, and
    the readonly_model.Group over the same cfg word with 0, 1, depth-1 or depth reads asked for. -> (clock dict, read group,
    [read states emitted by the requests], [contexts asked for])"""
    import readonly_model as RO
    c = L.Config(2, 1, L.CHECK_QUORUM)
    P = rng.choice((3, 3, 5, 8))
    g = L.random_group(rng, P, c)
    g["led"], g["tag"], g["el"], g["hb"] = True, g["cur_term"], c.election_tick - 1, 0
    ro = RO.Group(g["cfg"], commit=g["commit"], term_lo=0, term=g["cur_term"], depth=depth)
    asked = [1000 + k for k in range(rng.choice((0, 1, depth - 1, depth)))]
    emitted = []
    for ctx in asked:
        emitted += ro.request(ctx)[1]
    return c, P, g, ro, emitted, asked


def quorum_acks(ro, P, asked):
    """Every slot answers every context asked for, newest first -- what a quorum of heartbeat responses carries. -> read states"""
    out = []
    for ctx in reversed(asked):
        for s in range(P):
            out += ro.ack(s, ctx)
    return out


def test_model_cites_the_reference_lines():
    """The model is a restatement with its sources named: tick_heartbeat, the two arms of step_leader, quorum_recently_active with
    has_quorum, send_heartbeat's commit and the reset of a step-down."""
    src = open(os.path.join(HERE, "lead_clock_model.py")).read()
    for cite in ("raft.rs:1051-1079", ":1959-1962", ":1963-1973", "tracker.rs:346-361", ":367-372", "raft.rs:829-839", "raft.rs:942-971", ":1068-1070",
                 ":1063-1065", "src/config.rs:162-171"):
        assert cite in src, cite
    doc = L.step_down_reset.__doc__
    assert "(:957)" in doc and "ReadOnly::new" in doc  # the reset of a step-down no longer omits the ReadOnly


def test_step_down_reset_takes_a_read_only_group():
    """step_down_reset(g) alone is what it was; with a readonly_model.Group it empties that group's queue (raft.rs:957) and emits
    nothing; tick() hands the group through, and resets it in no call but the one that steps down."""
    import readonly_model as RO
    cfg3 = L.cfg_word((0, 1, 2), self_slot=0)
    g = L.new_group(3, cfg3 | 2 << 20, cur_term=5)
    g["el"], g["hb"] = 3, 1
    L.step_down_reset(g)
    assert (g["el"], g["hb"], g["led"], g["cfg"]) == (0, 0, False, cfg3)
    ro = RO.Group(cfg3, commit=9, term=5, depth=4)
    assert [ro.request(c)[0] for c in (7, 8)] == [RO.QUEUED] * 2
    g = L.new_group(3, cfg3, cur_term=5)
    L.step_down_reset(g, ro)
    assert ro.queue() == [] and ro.term == 5 and ro.ack(1, 8) == []
    c = L.Config(3, 1, L.CHECK_QUORUM)
    g = L.new_group(3, cfg3, cur_term=5)
    assert ro.request(9)[0] == RO.QUEUED
    seen = []
    for _ in range(3):
        seen.append((L.tick(c, g, ro), len(ro.queue())))
    assert seen == [(L.EV_BEAT, 1), (L.EV_BEAT, 1), (L.EV_CHECK_QUORUM | L.EV_STEPPED_DOWN, 0)]


def test_pending_reads_across_the_step_down_composed():
    """readonly_model + lead_clock_model over a seeded sweep of 200 groups: reads are queued, the clock ticks to the election
    timeout, then the acks that would have formed a quorum arrive. A group that stepped down releases NOTHING and reports no pending
    read; the same acks without the tick -- and on a group that stayed leader -- release exactly the model's states; a read queued
    after a later set_term(T + 1) is unaffected by the earlier reset."""
    import copy
    import readonly_model as RO
    rng = random.Random(957)
    kinds = set()
    for k in range(200):
        depth = (1, 2, 16)[k % 3]
        c, P, g, ro, emitted, asked = composed_group(rng, depth)
        untouched = copy.deepcopy(ro)
        want = quorum_acks(untouched, P, asked)  # ... without the step-down
        assert set(want) <= {(ctx, g["commit"]) for ctx in asked} - set(emitted) and len(set(want)) == len(want)
        pending = len(ro.queue())
        ev = L.tick(c, g, ro)
        assert ev & L.EV_CHECK_QUORUM
        if ev & L.EV_STEPPED_DOWN:
            assert not g["led"] and ro.queue() == [] and ro.last_pending() == 0 and ro.term == g["cur_term"]
            assert quorum_acks(ro, P, asked) == [] and ro.ack(0, 0, RO.ACK_LAST_SELF) == []
        else:
            assert g["led"] and len(ro.queue()) == pending
            assert quorum_acks(ro, P, asked) == want
        kinds.add((bool(ev & L.EV_STEPPED_DOWN), pending == 0, pending == depth, bool(want)))
        for grp in (ro, untouched):  # the next term: a fresh queue either way, whatever the earlier reset did
            grp.set_term(g["cur_term"] + 1)
            grp.term_lo = grp.commit
            st, rs = grp.request(5000)
            assert st in (RO.QUEUED, RO.READY) and grp.queue() == ([(5000, grp.commit, 1 << RO.cfg_self(grp.cfg))] if st == RO.QUEUED else [])
            if st == RO.QUEUED:
                rs = quorum_acks(grp, P, [5000])
            assert rs in ([(5000, grp.commit)], [])
        assert ro.queue() == untouched.queue()
    for down in (True, False):  # steppers and stayers with empty, partial and full queues, with a releasable quorum
        assert {(down, True, False, False), (down, False, True, True)} <= kinds, (down, sorted(kinds))
        assert any(k[0] == down and not k[1] and not k[2] for k in kinds), (down, sorted(kinds))


@pytest.mark.parametrize("P", [3, 8])
def test_model_agrees_with_the_oracle(oracle, P):
    """The quorum half is ro_quorum_recently_active and the heartbeat commits are ro_heartbeat_commit, group by group over a random
    shard of the baseline's shapes (joint configurations, learners, slots without a Progress), two sweeps so that the second meets
    the bits the first one left."""
    import oracle_lib as O
    from test_quorum_model import G_ORACLE, random_shard
    _, st, cl = random_shard(500 + P, P)
    lib = O.lib()
    groups = [L.new_group(P, int(st["cfg"][g]), pflags=[int(b) for b in st["pflags"][g]], match=[int(st["match"][p][g]) for p in range(P)], commit=int(st["commit"][g]))
              for g in range(G_ORACLE)]
    for g, grp in enumerate(groups):
        assert L.heartbeat_commits(grp, P) == [lib.ro_heartbeat_commit(cl.h, g, p + 1) for p in range(P)], g
    for sweep in range(2):
        seen = set()
        for g, grp in enumerate(groups):
            got = L.quorum_recently_active(grp)
            assert got == lib.ro_quorum_recently_active(cl.h, g, (grp["cfg"] >> 16 & 7) + 1), (sweep, g)
            seen.add(got)
        assert seen == {True, False}
        cl.store_soa(st)
        present = (st["cfg"] >> 24) & 0xff
        for g in range(0, G_ORACLE, 7):
            for p in range(8):
                if present[g] >> p & 1:
                    assert (groups[g]["pflags"][p] ^ int(st["pflags"][g][p])) & L.PF_RECENT_ACTIVE == 0, (sweep, g, p)


def test_reference_scenarios_on_the_model():
    """test_leader_stepdown_when_quorum_active (harness/tests/integration_cases/test_raft.rs:1851), test_leader_stepdown_when_quorum_lost
    (:1869) and test_leader_transfer_timeout (:3519), on the model."""
    cfg3 = L.cfg_word((0, 1, 2), self_slot=0)
    # :1851 -- new_test_raft(1, [1, 2, 3], election 5, heartbeat 1), check_quorum; a MsgHeartbeatResponse of peer 2 before every tick
    # (handle_heartbeat_response, raft.rs:1792: pr.recent_active = true); for _ in 0..=election_timeout
    c = L.Config(5, 1, L.CHECK_QUORUM)
    g = L.new_group(3, cfg3)
    seen = []
    for _ in range(c.election_tick + 1):
        g["pflags"][1] |= L.PF_RECENT_ACTIVE
        seen.append(L.tick(c, g))
    assert g["led"] and seen == [L.EV_BEAT] * 4 + [L.EV_BEAT | L.EV_CHECK_QUORUM] + [L.EV_BEAT]
    # :1869 -- nobody answers: Follower after the election timeout
    g = L.new_group(3, cfg3)
    seen = [L.tick(c, g) for _ in range(c.election_tick + 1)]
    assert not g["led"] and seen == [L.EV_BEAT] * 4 + [L.EV_CHECK_QUORUM | L.EV_STEPPED_DOWN, 0] and (g["hb"], g["el"]) == (0, 0)
    # :3519 -- Network::new's default config (election 10, heartbeat 1, no check_quorum), the transferee (peer 3) isolated:
    # still there after heartbeat_timeout ticks, gone -- and still Leader -- after election_timeout ticks
    c = L.Config(10, 1, 0)
    g = L.new_group(3, L.cfg_word((0, 1, 2), self_slot=0, transferee=2))
    before = list(g["pflags"])
    for _ in range(c.heartbeat_tick):
        L.tick(c, g)
    assert g["cfg"] >> 20 & 0xF == 3
    seen = [L.tick(c, g) for _ in range(c.election_tick - c.heartbeat_tick)]
    assert g["led"] and g["cfg"] >> 20 & 0xF == 0 and seen[-1] == L.EV_BEAT | L.EV_TRANSFER_ABORTED and g["pflags"] == before


def test_sweep_coverage_from_the_model_alone():
    """The sweep contains every event bit, check quorum off at an election timeout, stopped groups, and every step-down and write
    refusal; a step-down and a beat never come together; without check quorum no flag byte moves."""
    events, shapes = set(), set()
    for c, P, g in L.sweep(21, SWEEP):
        m = L.copy_group(g)
        ev = L.tick(c, m)
        events.add(ev)
        assert not (ev & L.EV_STEPPED_DOWN and ev & L.EV_BEAT)
        assert not ev & L.EV_STEPPED_DOWN or (ev & L.EV_CHECK_QUORUM and not m["led"] and m["cfg"] >> 20 & 0xF == 0)
        if not c.check_quorum or not ev & L.EV_CHECK_QUORUM:
            assert m["pflags"] == g["pflags"]
        if not ev & (L.EV_STEPPED_DOWN | L.EV_TRANSFER_ABORTED):
            assert m["cfg"] == g["cfg"]
        shapes.add(("led", m["led"]))
        if g["led"] and g["tag"] == g["cur_term"] and g["el"] + 1 >= c.election_tick:
            shapes.add(("timeout", c.check_quorum, bool(g["cfg"] >> 20 & 0xF), bool(ev & L.EV_BEAT)))
    bits = {b for b in (1, 2, 4, 8, 16) if any(ev & b for ev in events)}
    assert bits == {1, 2, 4, 8, 16} and 0 in events and L.EV_BEAT | L.EV_CHECK_QUORUM | L.EV_TRANSFER_ABORTED in events
    assert {("led", True), ("led", False)} <= shapes and {("timeout", cq, tr, beat) for cq in (True, False) for tr in (True, False) for beat in (True, False)} <= shapes
    statuses = set()
    for node, lead in step_down_cases(22, 2000):
        statuses.add(L.step_down(node, lead)[0][0])
    assert statuses == {H.DONE, H.NOT_WON, H.FAULT}
    c = L.Config(10, 3)
    assert [L.cell_refused(L.Config(e[0], e[1]), 8, (0, 1, e[2], e[3], e[4], e[5]), set()) for e, _ in WRITE_EDGES] == [r for _, r in WRITE_EDGES]
    assert L.cell_refused(c, 8, (8, 1, 0, 0, 1, (0,) * 7), set()) and L.cell_refused(c, 8, (3, 1, 0, 0, 1, (0,) * 7), {3})
    assert [L.Config(*e[:3]).valid(e[3]) for e, _ in CONFIG_EDGES] == [ok for _, ok in CONFIG_EDGES]


STAMP_TERMS = (0, 1, 2, 1 << 31, (1 << 32) - 1, (1 << 63) - 1, 1 << 63, (1 << 64) - 2, (1 << 64) - 1)  # RG_COL_CUR_TERM at both ends and in the middle
STOP_EDGES = ((5 | 3 << 14, 4, 4), (5 | 3 << 14, 3, 4), (1 << 31 | 2, 4, 4), (1 << 31 | 2, 3, 4), (0, 0, 0))  # (cell, tag, RG_COL_CUR_TERM)


def run_checks(exe):
    lines = ["X %d %d %d" % e for e in STOP_EDGES]  # the clock cell a step-down leaves: STOPPED; counters 0 where the tag was stale
    got = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")[:-1]
    for line, (cell, tag, term) in zip(got, STOP_EDGES):
        g = {"hb": cell & 0x3FFF, "el": cell >> 14 & 0x3FFF, "led": not cell >> 31, "tag": tag}
        node = G.Node(GATE, 1)
        node.load(term, 7, 7, 0, G.FOLLOWER, 0, 0, True)
        node.self_id = 7
        lead = H.fresh_lead(3, 7 | 7 << 24)
        lead.update(cur_term=term, term_lo=1, term_hi=0)
        assert L.step_down(node, lead, g)[0][0] == H.DONE and g["tag"] == term
        assert line.split() == ["X", str(L.cell_word(g))], (line, g)
    got = subprocess.run([exe], input="".join("R %d\n" % t for t in STAMP_TERMS), stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")[:-1]
    assert len(got) == len(STAMP_TERMS)
    for line, t in zip(got, STAMP_TERMS):  # the ReadIndex queue's term cell after a step-down: never the term (rg_read_sync_term then empties the queue)
        w = line.split()
        assert w[0] == "R" and int(w[1]) == ~t & (1 << 64) - 1 != t and int(w[2]) == 1, (line, t)
        # ... nor the NEXT term, which the queue has to tell from its stamp after an election (the one exception: 2^63 - 1)
        assert (int(w[1]) == t + 1) == (t == (1 << 63) - 1), (line, t)
    lines = ["W %d %d %d %d %d %s" % (e[0], e[1], e[2], e[3], e[4], " ".join("%d" % x for x in e[5])) for e, _ in WRITE_EDGES]
    lines += ["C %d %d %d %d" % e for e, _ in CONFIG_EDGES]
    got = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")[:-1]
    for line, (e, refused) in zip(got, WRITE_EDGES):
        w = line.split()
        assert w[0] == "W" and (int(w[1]) != 0) == refused, (line, e)
        if not refused:  # the record packs and unpacks to itself
            assert [int(x) for x in w[2:]] == [e[3] | e[2] << 14 | (0 if e[4] else 1 << 31), e[2], e[3], e[4]], (line, e)
    for line, (e, ok) in zip(got[len(WRITE_EDGES):], CONFIG_EDGES):
        assert line.split()[0] == "C" and (int(line.split()[1]) == 0) == ok, (line, e)


def test_host_twin_matches_the_model(tmp_path):
    """The edge list and a seeded sweep of 12 000 group-ticks: the event byte, both cells, the cfg word, the flag row and the
    heartbeat commits; the step-down's answers and soft cells; the host checks of the enable and the write."""
    exe = build_twin(tmp_path, "lead_clock_twin", [])
    edges = edge_ticks()
    ev = run_ticks(exe, edges)
    assert len(ev) == len(edges) > 1000 and {e & L.EV_STEPPED_DOWN for e in ev} == {0, L.EV_STEPPED_DOWN}
    for seed in (21, 23):
        cases = named_sweep(seed, SWEEP)
        assert len(run_ticks(exe, cases)) == SWEEP
    assert set(run_step_downs(exe, step_down_cases(22, 2000))) == {H.DONE, H.NOT_WON, H.FAULT}
    run_checks(exe)


def test_host_twin_is_clean_under_asan_and_ubsan(tmp_path):
    """The same program, -fsanitize=address,undefined -fno-sanitize-recover=all, run directly (a stand-alone executable)."""
    exe = build_twin(tmp_path, "lead_clock_twin_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    run_ticks(exe, edge_ticks()[::3])
    assert len(run_ticks(exe, named_sweep(24, 1500))) == 1500
    run_step_downs(exe, step_down_cases(25, 500))
    run_checks(exe)


def test_kernels_carry_no_scratch():
    """tools/kernel_resources.py over ext_lead.hip: k_lead_clock and the step-down kernels of both index widths use no scratch and
    no LDS."""
    if not os.path.exists(shutil.which("hipcc") or "/opt/rocm/bin/hipcc"):
        pytest.fail("hipcc is needed (the engine is built with it)")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--src=raft_rs_amd/csrc/ext_lead.hip"], cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines()[1:]:
        m = re.match(r"(\S.*?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)$", line)
        if m:
            rows[m.group(1)] = (int(m.group(5)), int(m.group(6)))
    for name in ("k_lead_clock", "k_handoff_step_down_dense", "k_handoff_step_down_list"):
        mine = {k: v for k, v in rows.items() if k.startswith(name + "<")}
        assert sorted(mine) == [name + "<unsigned int>", name + "<unsigned long>"], (name, sorted(rows), out.stderr[-1000:])
        for k, (scratch, lds) in mine.items():
            print(k, scratch, lds)
            assert scratch == 0 and lds == 0, (k, scratch, lds)
    for name in ("k_lead_clock_write", "k_lead_clock_read", "k_lead_init", "k_lead_place"):
        assert rows[name] == (0, 0), (name, rows[name])


def test_every_new_name_is_declared_exported_and_bound(rg):
    """The extension header include/raftgroups_lead.h: every function it declares is exported (as rgx_*, nothing else with that
    prefix) and bound, in Python and in
    the generated bindings/raftgroups_lead.rs with the header's arity; raftgroups.h, its version and its count are what they were."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_bindings
    from raft_rs_amd import engine as E
    hdr = open(os.path.join(ROOT, "include", "raftgroups_lead.h"), encoding="utf-8").read()
    declared = set(re.findall(r"\b(rgx_\w+)\s*\([^()]*\)\s*;", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))  # every prototype of the header
    assert declared == set(NEW_NAMES)
    assert not {name for name, _, _ in gen_rust_bindings.parse(hdr)[3]}  # ... and it declares no rg_* function
    core = open(os.path.join(ROOT, "include", "raftgroups.h"), encoding="utf-8").read()
    assert not any(name in core for name in NEW_NAMES) and "rgx_" not in core and "#define RG_ABI_VERSION 12u" in core
    nm = subprocess.run(["nm", "-D", "--defined-only", rg.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert {l.split()[-1] for l in nm.splitlines() if l.split() and l.split()[-1].startswith("rgx_")} == declared
    lib = ctypes.CDLL(rg.LIB_PATH)
    for name in NEW_NAMES:
        assert name in declared and hasattr(lib, name) and name in E.SYMBOLS, name
    assert "eight `rgx_*` exports" in open(os.path.join(ROOT, "README.md")).read() and len(declared) == 8
    # the generated Rust module: up to date (tests/test_abi.py runs the generator's --check, which covers it), one declaration per
    # prototype of the header, the same number of arguments, every struct and constant of the header
    rs = open(os.path.join(ROOT, "bindings", "raftgroups_lead.rs")).read()
    assert rs == gen_rust_bindings.generate_lead()
    rust = {m.group(1): m.group(2) for m in re.finditer(r"pub fn (rgx_\w+)\((.*?)\)(?: -> [^;]+)?;", rs)}
    assert set(rust) == declared
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in declared:
        c_args = [x for x in re.search(r"\b" + name + r"\s*\(([^()]*)\)\s*;", plain, flags=re.S).group(1).split(",") if x.strip() and x.strip() != "void"]
        assert len(c_args) == len([x for x in rust[name].split(",") if x.strip()]), name
    for needle in ("pub struct RgLeadClockConfig", "pub struct RgLeadClockCell", "pub struct RgLeadClockOut", "pub const RG_LEAD_EV_NEW_TERM: u32 = 0x10;",
                   "pub const RG_LEAD_CLOCK_START_LED: u32 = 0x100;", "pub const RG_HANDOFF_NO_LEAD: u64 = u64::MAX;", "pub const RGX_LEAD_VERSION: u32 = 1;"):
        assert needle in rs, needle
    lib.rgx_lead_version.restype = ctypes.c_uint32
    assert lib.rgx_lead_version() == int(re.search(r"#define RGX_LEAD_VERSION (\d+)u", hdr).group(1)) == E.LEAD_VERSION
    for k, v in (("BEAT", E.LEAD_EV_BEAT), ("CHECK_QUORUM", E.LEAD_EV_CHECK_QUORUM), ("STEPPED_DOWN", E.LEAD_EV_STEPPED_DOWN),
                 ("TRANSFER_ABORTED", E.LEAD_EV_TRANSFER_ABORTED), ("NEW_TERM", E.LEAD_EV_NEW_TERM)):
        assert int(re.search(r"#define RG_LEAD_EV_%s (0x[0-9a-f]+)u" % k, hdr).group(1), 16) == v == getattr(L, "EV_" + k), k
    assert int(re.search(r"#define RG_LEAD_CLOCK_START_LED (0x[0-9a-f]+)u", hdr).group(1), 16) == E.LEAD_CLOCK_START_LED == L.START_LED
    assert "#define RG_HANDOFF_NO_LEAD (~0ULL)" in hdr and E.HANDOFF_NO_LEAD == L.NO_LEAD
    assert E.LEAD_CLOCK_CELL_DTYPE.names == ("group", "term", "election_elapsed", "heartbeat_elapsed", "led", "reserved")
    assert (ctypes.sizeof(E.LeadClockConfig), ctypes.sizeof(E.LeadClockOut), E.LEAD_CLOCK_CELL_DTYPE.itemsize) == (16, 48, 32)
    assert [f for f, _ in E.LeadClockOut._fields_] == list(E.LEAD_CLOCK_OUT_FIELDS) and E.ABI_VERSION == 12
    for method in ("lead_clock_enable", "lead_clock_write", "lead_clock_read", "lead_clock", "lead_clock_counts", "follow_step_down", "follow_step_down_device"):
        assert callable(getattr(E.Engine, method)), method
    assert np.dtype(E.LEAD_CLOCK_CELL_DTYPE).fields["reserved"][0].shape == (7,)


def test_api_refusals_are_host_checks():
    """What the calls refuse is decided on the host, before anything is staged or launched: the state checks, the group bounds, the
    cell rules and the duplicate rules stand in front of RG_ENTER; the unit includes the HIP-free header, which includes nothing
    but rg_handoff.h and the extension's public header."""
    src = open(os.path.join(ROOT, "raft_rs_amd", "csrc", "ext_lead.hip")).read()
    for fn, needles in (("rgx_lead_clock_enable", ("h->ld", "rg_lead_config_check")),
                        ("rgx_lead_clock_write", ("!h->ld", "w.group >= h->G", "rg_lead_cell_check", "seen.emplace")),
                        ("rgx_lead_clock_read", ("!h->ld", "host_groups[i] >= h->G")),
                        ("rgx_lead_clock", ("!h->ld", "!dev_out->events")),
                        # (the election layer, and the record walk with its bounds and duplicate rules: rg_handoff_host.h, which
                        # tests/test_handoff_host.py reads)
                        ("rgx_follow_step_down", ("rg_elect_enabled", "rg_walk_pairs")),
                        ("rgx_follow_step_down_device", ("rg_elect_enabled", "h->host_mirror", "rg_handoff_out_complete"))):
        body = src[src.index('extern "C" int %s(' % fn):]
        body = body[:body.index("} RG_ABI_GUARD")]
        enter = body.index("RG_ENTER(h)")
        for needle in needles:
            assert 0 <= body.find(needle) < enter, (fn, needle)
    hdr = open(os.path.join(ROOT, "raft_rs_amd", "csrc", "rg_lead.h")).read()
    assert re.findall(r"#include\s+(\S+)", hdr) == ['"rg_handoff.h"', '"../../include/raftgroups_lead.h"']
    # every int entry point of the unit is a function-try-block that ends in RG_ABI_GUARD, as in the abi_*.hip units
    heads = [l for l in src.split("\n") if l.startswith('extern "C" int ')]
    assert len(heads) == 6 and all(l.rstrip().endswith("try {") for l in heads) and src.count("\n} RG_ABI_GUARD") == 6
    assert "ext_lead.hip" in open(os.path.join(ROOT, "raft_rs_amd", "build.py")).read()
