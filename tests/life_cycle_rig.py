"""What the GPU tests of a group's life cycle share (tests/test_step_down_gpu.py, tests/test_second_term_gpu.py,
tests/test_step_down_corners_gpu.py): the promoted rig with the leader's clock behind it, the two clock calls to the step-down,
lead_clock_model over every group of a rig's leader engine, the model's arena after a step-down, and the device columns of a
vote round and of an election call's answers."""
import numpy as np

import gate_model as G
import handoff_model as H
import handoff_rig as R
import lead_clock_model as L
from test_follow_elect_gpu import U8_COLS, U64_COLS
from test_handoff_gpu import GATE, OUT_SENT, Rig, dev

CLOCK = L.Config(2, 1, L.CHECK_QUORUM)


def promoted_rig(rg, ix64=False):
    """The 3-slot rig with the model's promotable cases promoted (dense) and the leader's clock enabled behind it: every led group
    starts at 0 / 0 with the tag of its current term."""
    rig = Rig(rg, 3, ix64=ix64)
    cases = H.gpu_cases(3)
    rig.load_lead(R.state_with(rig.G, 3, rig.eng.stride, cases))
    rig.load_arena(cases)
    _, answers = R.model_state(R.state_with(rig.G, 3, rig.eng.stride, cases), cases)
    rig.promote(cases, True, answers, vouch=True)
    rig.eng.lead_clock_enable(CLOCK.election_tick, CLOCK.heartbeat_tick, CLOCK.flags | L.START_LED)
    return rig, cases, [c for c in cases if c.expect == H.DONE]


def tick_until_down(rig):
    """Two clock calls: a promoted group (Progress reset, nobody recent_active but itself) loses its quorum at the first election
    timeout; the quiet base groups (every peer recent_active) pass their first check. -> the device event column"""
    import torch
    events = torch.zeros(rig.eng.stride, dtype=torch.uint8, device="cuda")
    assert rig.eng.lead_clock(events)[2] == 0
    counts = rig.eng.lead_clock(events)
    return events, counts


def node_of(g, soft, cells):
    n = G.Node(GATE, g)
    n.load(*soft)
    n.self_id = cells[0]
    return n


def expect_arena(before, lead_state, pairs):
    """The model's arena after stepping down `pairs` [(follow group, lead group)] -> (arena list, answers)"""
    want, answers = list(before), []
    for g, Lg in pairs:
        canon, soft, cells = before[g]
        node = node_of(g, soft, cells)
        a, c = L.step_down(node, R.get_lead(lead_state, Lg))
        answers.append(a)
        if a[0] == H.DONE:
            want[g] = (c, node.soft(), cells)
    return want, answers


class ClockModel:
    """lead_clock_model over every group of a rig's leader engine: the columns the clock reads are taken from the engine (ticks and
    promotions write them), the clock cells are the model's own."""

    def __init__(self, rig, c):
        self.rig, self.c = rig, c
        self.groups = [L.new_group(rig.P, 0, led=False) for _ in range(rig.G)]
        self.adopt(first=True)

    def adopt(self, first=False):
        st = self.rig.read_lead()
        for i, g in enumerate(self.groups):
            d = R.get_lead(st, i)
            g.update(cfg=d["cfg"], cur_term=d["cur_term"], commit=d["commit"], match=d["match"], pflags=d["pflags"] + [0] * (8 - self.rig.P))
            if first:
                g["tag"] = g["cur_term"]
        return st

    def tick(self):
        return [L.tick(self.c, g) for g in self.groups]

    def check(self, events, want):
        ev = events.cpu().numpy()
        assert [int(x) for x in ev[:self.rig.G]] == want, [(i, int(ev[i]), w) for i, w in enumerate(want) if int(ev[i]) != w][:5]
        got = self.rig.eng.lead_clock_read(np.arange(self.rig.G, dtype=np.uint64))
        for i, (r, g) in enumerate(zip(got, self.groups)):
            assert (int(r["term"]), int(r["election_elapsed"]), int(r["heartbeat_elapsed"]), int(r["led"])) == (g["tag"], g["el"], g["hb"], int(g["led"])), (i, r, g)
        st = self.rig.read_lead()
        assert [int(x) for x in st["cfg"]] == [g["cfg"] for g in self.groups]
        assert [[int(b) for b in row[:self.rig.P]] for row in st["pflags"]] == [g["pflags"][:self.rig.P] for g in self.groups]


def vote_round(S, groups, kind, term):
    """The device columns of one round of vote responses: slot 0 grants `kind` at `term` to every group of `groups`."""
    cols = {k: np.zeros(S, np.uint8) for k in ("kind", "slot", "reject")}
    cols.update({k: np.zeros(S, np.uint64) for k in ("term", "commit", "commit_term")})
    for g in groups:
        cols["kind"][g], cols["slot"][g], cols["term"][g] = kind, 0, term
    return {k: dev(v) for k, v in cols.items()}


def elect_out(size):
    """The output columns of an election call, sentinels in the status bytes."""
    import torch
    o = {k: torch.full((size,), OUT_SENT, dtype=torch.uint8, device="cuda") for k in U8_COLS}
    o.update({k: torch.zeros(size, dtype=torch.int64, device="cuda") for k in U64_COLS})
    return o
