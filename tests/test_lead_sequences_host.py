"""CPU only: the composer of tests/lead_sequence.py checked without a GPU.

(1) The composed model against a CONTINUOUS oracle: the same seeded sequences with a second executor, ONE O.Cluster that lives through
the whole sequence. Ticks, local events and the send stage run directly on it; conf changes go through
test_conf_change_host.oracle_route and transfers through the route of test_transfer_host.model_and_route (the checks are the model's,
what they lead to is the oracle's); the clock and the gate, which have no counterpart in the oracle, run as the model's and reach the
cluster through ro_group_set_transferee and the recent_active flags. The oracle has no call that edits a membership, so oracle_route
loads the edited columns into the living cluster and hands it back its windows; a restore loads the checkpoint's. After every step every
R.ALL_COLS column, every window, the clock cells and every item set are equal: the reload-per-tick executor of the truth loses nothing
the oracle keeps outside the SoA, and the four Python models compose.
(2) The coverage floors of every seed the GPU file uses, on the model alone -- among them a conf call and a transfer call in which all
256 lanes of a workgroup owe items, and a wave whose lanes all owe P - 1 --, and every documented refusal tried by one seed or another.
(3) Three mutations of the continuous executor, each caught within the committed seeds: the evidence that the sequences reach the
hand-offs at all."""
import ctypes
import time

import numpy as np
import pytest

import conf_model as CM
import handoff_rig as R
import lead_sequence as S
import transfer_model as TM
from test_conf_change_host import oracle_route

ALL = [(S.SEEDS[c], c[0], c[2], False) for c in S.CASES] + [(S.TWIN_SEED, S.TWIN_CASE[0], S.TWIN_CASE[2], True)]
MUTATIONS = ("transfer_keeps_election_elapsed", "added_peer_not_recent_active", "step_down_keeps_transferee")


class Continuous:
    """The second executor: one cluster from the first step to the last"""

    def __init__(self, O, tr, mutation=None):
        self.O, self.G, self.P, self.cap, self.mutation = O, tr.G, tr.P, tr.cap, mutation
        self.st, self.cells, self.ckpt = R.copy_state(tr.st), S.copy_cells(tr.cells), None
        self.cl = O.Cluster(self.G)
        self.cl.load_soa(self.st, term=S.TERM, max_inflight=self.cap)
        self.cl.set_own_inflights(self.cap > 0)

    def windows(self):
        win = {}
        if self.cap:
            S.export_windows(self.cl, win, self.st, self.cap)
        return win

    def sync(self):
        self.cl.store_soa(self.st)
        self.st["run_count"] = S.run_count_of(self.st)

    def led(self, g):
        c = self.cells[g]
        return c["tag"] != int(self.st["cur_term"][g]) or c["led"]

    def push_soft(self):
        """what the clock or the gate did to the columns, into the cluster: lead_transferee and Progress::recent_active"""
        L, h, cfg, pf = self.cl.L, self.cl.h, self.st["cfg"], self.st["pflags"]
        for g in range(self.G):
            L.ro_group_set_transferee(h, g, int(cfg[g]) >> 20 & 0xF)
            for s in range(self.P):
                if int(cfg[g]) >> 24 >> s & 1:
                    L.ro_group_progress(h, g, s + 1).contents.recent_active = bool(int(pf[g, s]) & CM.PF_RECENT_ACTIVE)

    def apply(self, op):
        """-> the items of the step, as the truth reports them"""
        items = getattr(self, "_" + op["kind"])(op)
        self.sync()
        return items

    def _tick(self, op):
        msgs = dict(op["msgs"])
        if op["terms"] is not None:
            self.sync()
            msgs["m_flags"] = S.gate_step(self.st, self.cells, msgs["m_flags"], op["terms"])[0]
            self.push_soft()
        gout = np.zeros(self.G, dtype=np.uint32)
        self.cl.tick_soa(msgs, gout)
        return S.coalesce(self.cl.send_stage_soa(gout, op["max_entries"], skip_bcast_commit=op["skip"]) if self.cap else ())

    def _clock(self, op):
        before = self.st["cfg"].copy()
        events, _, _ = S.clock_step(self.st, self.cells)
        if self.mutation == "step_down_keeps_transferee":
            for g in [g for g, ev in enumerate(events) if ev & S.L.EV_STEPPED_DOWN]:
                self.st["cfg"][g] |= before[g] & np.uint32(0xF << 20)
        self.push_soft()
        return {}

    def _conf(self, op):
        recs = op["recs"]
        win = self.windows()
        led = {g: self.led(g) for g, _ in recs}
        _, answers, _ = CM.apply_state(self.st, S.copy_windows(win) if self.cap else None, recs, self.cap, led=led, max_entries=op["max_entries"])
        flags = CM.PROBE if self.mutation == "added_peer_not_recent_active" else CM.PROBE | CM.PF_RECENT_ACTIVE
        self.st, sent, _ = oracle_route(self.O, self.st, recs, answers, self.cap, op["max_entries"], cl=self.cl, windows=win, added_pflags=flags)
        return S.coalesce(sent)

    def _transfer(self, op):
        recs = op["recs"]
        led = {g: self.led(g) for g, _ in recs}
        cells = {g: dict(self.cells[g]) for g, _ in recs}
        _, answers, _ = TM.apply_state(self.st, self.windows() if self.cap else None, recs, self.cap, led=led, cells=cells, max_entries=op["max_entries"])
        cl, sent = self.cl, []
        for (g, t), a in zip(recs, answers):
            if a["previous"]:
                cl.L.ro_group_set_transferee(cl.h, g, 0)
            if a["status"] != TM.STARTED:
                continue
            cl.L.ro_group_set_transferee(cl.h, g, t + 1)
            if self.cells[g]["tag"] == int(self.st["cur_term"][g]) and self.mutation != "transfer_keeps_election_elapsed":
                self.cells[g]["el"] = 0  # raft.rs:1876
            assert bool(a["events"] & TM.EV_TIMEOUT_NOW) == (cl.pr(g, t + 1).matched == cl.last_index(g)), (g, a)
            if a["events"] & TM.EV_APPEND and self.cap:
                ok, m = cl.maybe_send_append(g, t + 1, True, op["max_entries"])
                if ok:
                    sent.append((m.group, m.to, m.index, m.n_entries, m.kind, 0))
        return S.coalesce(np.array(sent, dtype=self.O.SEND_MSG_DTYPE))

    def _events(self, op):
        S.apply_events(self.cl, op["events"], self.G, self.P)
        return {}

    def _checkpoint(self, op):
        self.ckpt = (R.copy_state(self.st), self.windows(), S.copy_cells(self.cells))
        return {}

    def _restore(self, op):
        st, win, cells = self.ckpt
        self.st, self.cells = R.copy_state(st), S.copy_cells(cells)
        self.cl.load_soa(self.st, term=S.TERM, max_inflight=self.cap)
        self.cl.set_own_inflights(self.cap > 0)
        S.add_windows(self.cl, win, self.st)
        return {}


def first_mismatch(tr, cont, want, items):
    """what differs between the truth and the continuous executor after a step, or None"""
    d = S.first_diff(tr.st, cont.st, cols=R.ALL_COLS)
    if d:
        return ("column",) + d
    if tr.cap:
        win = cont.windows()
        cfg = tr.st["cfg"]
        for g in range(tr.G):
            for s in range(tr.P):
                if int(cfg[g]) >> 24 >> s & 1 and win.get((g, s), []) != tr.win.get((g, s), []):
                    return "window", g, s, tr.win.get((g, s), []), win.get((g, s), [])
    if tr.cells != cont.cells:
        g = next(g for g in range(tr.G) if tr.cells[g] != cont.cells[g])
        return "clock cell", g, None, tr.cells[g], cont.cells[g]
    d = S.diff_items(want.get("items", {}), items)
    return ("item",) + d if d else None


def run(O, seed, P, cap, twin, mutation=None):
    """-> (the truth at the end, the first mismatch as (step, op name, what) or None)"""
    tr, ch = S.Truth(seed, P, cap), S.Chooser(seed, P, cap, twin=twin)
    cont = Continuous(O, tr, mutation)
    for step in range(S.STEPS):
        op = ch.next(tr)
        want = tr.apply(op)
        bad = first_mismatch(tr, cont, want, cont.apply(op))
        if bad:
            return tr, (seed, step, op["name"], bad)
    return tr, None


@pytest.mark.parametrize("seed,P,cap,twin", ALL)
def test_the_composed_model_equals_a_continuous_oracle_and_meets_its_floors(oracle, seed, P, cap, twin):
    """Every committed seed: after every step every column, every window, every clock cell and the item set of the truth equal the
    cluster's that was never rebuilt between two ticks; and the floors of the sequence hold on the model alone."""
    t0 = time.time()
    tr, bad = run(oracle, seed, P, cap, twin)
    assert bad is None, bad
    print("seed %d P %d cap %d twin %s: %.1f s: %s" % (seed, P, cap, twin, time.time() - t0, tr.cov.line()))
    S.check_floors(tr.cov, cap)


def test_the_same_seed_gives_the_same_sequence_with_nothing_beside_it():
    """The chooser reads the truth alone: two runs of a seed draw the same ops, the same records and the same message columns"""
    def digest(seed, P, cap):
        out = []
        for step, op, want, tr in S.sequence(seed, P, cap, steps=12):
            parts = [op["name"], repr(op.get("bad")), repr(op.get("recs")), repr(op.get("events")), repr(op.get("item_cap"))]
            if op["kind"] == "tick":
                parts += [op["msgs"][k].tobytes() for k in ("m_index", "m_commit", "m_hint", "m_rs", "m_flags")] + [None if op["terms"] is None else op["terms"].tobytes()]
            out.append(tuple(parts))
        return out
    assert digest(3, 5, 8) == digest(3, 5, 8)
    assert digest(3, 5, 8) != digest(4, 5, 8)


def test_the_committed_seeds_try_every_forbidden_call():
    """Each of the documented refusals is tried by at least one of the committed seeds (every seed tries at least two: a floor)"""
    tried = set()
    for seed, P, cap, twin in ALL:
        for step, op, want, tr in S.sequence(seed, P, cap, twin=twin):
            pass
        tried |= set(tr.cov.bad)
    assert tried == set(S.BAD_CALLS), sorted(set(S.BAD_CALLS) - tried)


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_each_mutation_of_the_continuous_executor_is_caught(oracle, mutation):
    """the transfer does not zero election_elapsed / apply_conf leaves RECENT_ACTIVE clear on an added peer / the clock's step-down
    keeps the TRANSFEREE bits: the comparison fails within the committed seeds, at the step that makes the slip"""
    caught = []
    for seed, P, cap, twin in ALL[:3]:
        _, bad = run(oracle, seed, P, cap, twin, mutation)
        if bad:
            caught.append(bad)
    print(mutation, caught)
    want = {"transfer_keeps_election_elapsed": ("transfer", "clock cell"), "added_peer_not_recent_active": ("conf", "column"),
            "step_down_keeps_transferee": ("clock", "column")}[mutation]
    assert len(caught) == 3 and all(c[2].startswith(want[0]) and c[3][0] == want[1] for c in caught), caught
    assert mutation != "added_peer_not_recent_active" or all(c[3][1] == "pflags" for c in caught)
    assert mutation != "step_down_keeps_transferee" or all(c[3][1] == "cfg" for c in caught)


@pytest.mark.parametrize("P,seed", S.MIRROR_CASES)
def test_the_read_mirror_seeds_meet_their_floors_and_produce_packed_launches(oracle, P, seed):
    """The seeds of the read-mirror sequences (tick_runs: runs of 2-4 plain ticks), on the model alone: the floors of every
    sequence, and what readmirror.after predicts for the engine beside it -- packed launches, i.e. ticks that read the plane."""
    import readmirror as RM
    tr, ch = S.Truth(seed, P, 0), S.Chooser(seed, P, 0, tick_runs=True)
    classes, runs, dropped_valid, valid = [], [], 0, False
    while not ch.done():
        op = ch.next(tr)
        tr.apply(op)
        step = S.mirror_classes(op, first=not classes)
        dropped_valid += valid and step[0] == "drop"  # a call that has to drop a plane a tick left valid
        classes += step
        valid = RM.launch_counts(classes)[2]
        if op["kind"] == "tick" and not op.get("follows"):
            runs.append(1)
        elif op.get("follows"):
            runs[-1] += 1
    S.check_floors(tr.cov, 0)
    build, packed, valid = RM.launch_counts(classes)
    assert (build, packed) == S.MIRROR_LAUNCHES[(P, seed)] and packed >= 15 and build + packed < 32, (build, packed)
    assert {2, 3, 4} >= {r for r in runs if r > 1} and max(runs) >= 3, runs
    assert dropped_valid >= 5, dropped_valid
