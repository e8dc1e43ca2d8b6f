"""GPU: the entry points behave as tests/test_read_mirror_entry_points.py classifies them. For every `keep` or `drop` entry that an
engine with the read mirror can reach: a packed tick, the call with small valid arguments, rgr_mirror_stats.valid as classified,
the next tick a build or a packed launch as classified, every column equal to a RG_CFGF_NO_READ_MIRROR twin that got the same
calls, and the tick behind the call equal to the oracle reloaded from the engine's columns (as tests/test_mirror_gpu.py does for
its seven calls). A `drop` call is then tried once more in a form the library refuses, with the flag pinned per case
(Pair.refuse): 1 where the refusal comes from the checks in front of RG_ENTER (nothing entered, nothing written), 0 where the
call had entered -- and no column changes either way. Publication every third tick: the riding event goes out on a packed
launch."""
import numpy as np
import pytest

import fuzz
import oracle_lib as O
from test_read_mirror_entry_points import TABLE

pytestmark = pytest.mark.gpu
G, P, TERM = 193, 5, 4
STATE_COLS = ("match", "next", "pr_commit", "pend_snap", "pend_rs", "pflags", "commit", "term_lo", "term_hi", "cfg", "out")


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


class Pair:
    """A mirror-on engine and its mirror-less twin on the headline stream (BASELINE config 2, five slots, no size classes), the
    host mirror of RawNode::step registered where a case needs it, and the oracle."""

    def __init__(self, rg, host_mirror=False, max_inflight=0):
        self.rg, self.E = rg, rg.engine
        self.on = rg.Engine(G, P, flags=rg.CFGF.NO_SIZE_CLASSES, max_inflight=max_inflight)
        self.off = rg.Engine(G, P, flags=rg.CFGF.NO_SIZE_CLASSES | rg.CFGF.NO_READ_MIRROR, max_inflight=max_inflight)
        self.engines = (self.on, self.off)
        for e in self.engines:
            e.workload_init(rg.WL_MAJORITY)
            if host_mirror:
                for g in range(G):
                    e.set_peers(g, list(range(1, P + 1)), TERM)
        self.msgs, self.gout, self.t = rg.MsgBuffers(G, P, self.on.stride), np.zeros(G, dtype=np.uint32), 0
        self.keep = []  # device buffers the asynchronous calls read
        self.resync()

    def close(self):
        for e in self.engines:
            e.sync()
            e.close()

    def both(self, call):
        return [call(e) for e in self.engines]

    def stats(self):
        s = self.on.mirror_stats()
        return s["build_launches"], s["packed_launches"], s["valid"]

    def resync(self):
        """the engines agree cell for cell; the oracle is reloaded from their columns (rg_read_column keeps the mirror)"""
        a, b = self.on.read_state(), self.off.read_state()
        diffs = fuzz.diff_states(a, b, G, P, present_only=False)
        assert not diffs, diffs[:5]
        assert (a["out"] == b["out"]).all()
        self.st = a
        self.cl = O.Cluster(G)
        self.cl.load_soa(self.st, term=TERM - 1)
        return a

    def tick(self, check=True):
        """one tick of the generated stream on both engines and the oracle, compared (check=False: by a later check())"""
        self.cl.store_soa(self.st)
        self.E.workload_gen_host(self.st, self.msgs, self.rg.WL_MAJORITY, self.t)
        self.t += 1
        for e in self.engines:
            e.tick(self.msgs)
        self.cl.tick_soa(self.msgs.as_dict(), self.gout)
        self.cl.store_soa(self.st)
        if check:
            self.check()

    def check(self):
        for e in self.engines:
            got = e.read_state()
            diffs = fuzz.diff_states(self.st, got, G, P)
            assert not diffs, (self.t, diffs[:5])
            assert (got["out"] == self.gout).all(), self.t
        s = self.off.mirror_stats()
        assert (s["build_launches"], s["packed_launches"]) == (0, 0)

    def packed_tick(self):
        """ticks until the last launch read the plane (two at the most)"""
        for _ in range(2):
            before = self.stats()
            self.tick()
            now = self.stats()
            if now[1] == before[1] + 1:
                assert now[2] == 1
                return
        raise AssertionError("no packed launch: %s" % (self.stats(),))

    def follower(self, g):
        w = int(self.st["cfg"][g])
        return next(s for s in range(P) if s != ((w >> 16) & 7) and (w >> (24 + s)) & 1)

    def exercise(self, name, entries, call, fail=None, refused="before"):
        """entries: the exported names the case goes through (all of one class). fail: the same call in a form the library
        refuses, made behind another packed tick (refuse())."""
        classes = {TABLE[n] for n in entries}
        assert len(classes) == 1 and classes <= {"keep", "drop"}, (name, classes)
        cls = classes.pop()
        self.packed_tick()
        b0, p0, _ = self.stats()
        got = self.both(call)
        assert same(got[0], got[1]), (name, "the two engines answered differently")
        assert self.stats()[2] == (1 if cls == "keep" else 0), (name, cls, self.stats())
        self.resync()
        self.tick()
        assert self.stats()[:2] == ((b0, p0 + 1) if cls == "keep" else (b0 + 1, p0)), (name, cls, (b0, p0), self.stats())
        if fail is not None:
            self.refuse(name, fail, refused)

    def refuse(self, name, fail, refused="before"):
        """A call the library refuses, behind a packed tick. refused = "before": the refusal comes from the checks in front of
        RG_ENTER -- nothing has been entered, nothing written, and the flag is still 1; "after": the call had entered when it
        failed, and a failed entry leaves the mirror dropped: 0. Either way no column changes, and the next tick is a packed or
        a build launch accordingly. A change of the order of check and entry, in either direction, fails here."""
        self.packed_tick()
        before = self.on.read_state()
        b0, p0, _ = self.stats()
        raised = []
        for e in self.engines:
            try:
                fail(e)
                raised.append(False)
            except self.rg.EngineError:
                raised.append(True)
        valid = self.stats()[2]
        self.pin(name, raised, valid, refused)
        after = self.resync()
        assert all((before[k] == after[k]).all() for k in STATE_COLS), (name, "a refused call changed the columns")
        self.tick()
        assert self.stats()[:2] == ((b0 + 1, p0) if valid == 0 else (b0, p0 + 1)), (name, valid, self.stats())

    def pin(self, name, raised, valid, refused):
        assert all(raised), (name, "the call was not refused", raised)
        assert valid == {"before": 1, "after": 0}[refused], (name, "refused %s RG_ENTER, rgr_mirror_stats.valid = %d" % (refused, valid))


def same(a, b):
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.tobytes() == b.tobytes()
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if hasattr(a, "cpu"):
        return same(a.cpu().numpy(), b.cpu().numpy())
    return a == b


# ---- leader control: conf change, transfer, clock, term gate, local events -----------------------------------------------------
def test_leader_control_calls(rg):
    import torch
    import conf_model as CM
    pr = Pair(rg)
    E, stride = pr.E, pr.on.stride
    full = (1 << P) - 1

    def conf_recs(recs):
        a = np.zeros(len(recs), dtype=E.CONF_REC_DTYPE)
        for k, (g, W) in enumerate(recs):
            a[k]["group"], a[k]["cfg"] = g, W
        return a

    def xfer_recs(recs):
        a = np.zeros(len(recs), dtype=E.TRANSFER_REC_DTYPE)
        for k, (g, s) in enumerate(recs):
            a[k]["group"], a[k]["slot"] = g, s
        return a

    # the sparse conf change: the follower of group 3 becomes a learner (the same word again is a valid call that changes nothing)
    def conf_sparse(e):
        w = int(pr.st["cfg"][3])
        inc = (w & 0xFF) & ~(1 << pr.follower(3))
        return e.apply_conf(conf_recs([(3, CM.word(inc, 0, full))]))[0]

    pr.exercise("rgc_apply_conf", ["rgc_apply_conf"], conf_sparse, fail=lambda e: e.apply_conf(conf_recs([(G, CM.word(1))])))

    def conf_dense(e):
        sel, cfg = np.zeros(G, np.uint8), np.zeros(G, np.uint32)
        for g in (5, 64, 192):
            sel[g], cfg[g] = 1, CM.word(full, 0, full)
        cols = [dev(sel), dev(cfg)] + [torch.zeros(G, dtype=torch.uint8, device="cuda") for _ in range(2)]
        pr.keep.append(cols)
        e.apply_conf_device(cols[0], cols[1], cols[2], cols[3])
        e.sync()
        return cols[2], cols[3]

    pr.exercise("rgc_apply_conf_device", ["rgc_apply_conf_device"], conf_dense, fail=lambda e: e.apply_conf_device(dev(np.zeros(G, np.uint8)), dev(np.zeros(G, np.uint32)), None))
    # the transfer, the events-only road of an engine without device Inflights
    pr.exercise("rgm_transfer_leader", ["rgm_transfer_leader"], lambda e: e.transfer_leader(xfer_recs([(7, pr.follower(7))]))[0],
                fail=lambda e: e.transfer_leader(xfer_recs([(7, P)])))

    def xfer_dense(e):
        to = np.zeros(G, np.uint8)
        for g in (9, 65, 191):
            to[g] = pr.follower(g) + 1
        cols = [dev(to)] + [torch.zeros(G, dtype=torch.uint8, device="cuda") for _ in range(2)]
        pr.keep.append(cols)
        e.transfer_leader_device(cols[0], cols[1], cols[2])
        e.sync()
        return cols[1], cols[2]

    pr.exercise("rgm_transfer_leader_device", ["rgm_transfer_leader_device"], xfer_dense, fail=lambda e: e.transfer_leader_device(dev(np.zeros(G, np.uint8)), None))
    # the clock: enable, write, read, one Raft::tick of every group (check-quorum clears RECENT_ACTIVE: the flag rows change)
    pr.exercise("rgx_lead_clock_enable", ["rgx_lead_clock_enable"], lambda e: e.lead_clock_enable(4, 1, E.GATE_CHECK_QUORUM | E.LEAD_CLOCK_START_LED),
                fail=lambda e: e.lead_clock_enable(4, 1, E.GATE_CHECK_QUORUM))
    everyone = np.arange(G, dtype=np.uint64)

    def clock(e):
        ev = torch.zeros(stride, dtype=torch.uint8, device="cuda")
        pr.keep.append(ev)
        counts = e.lead_clock(ev)
        return counts, ev

    pr.exercise("rgx_lead_clock", ["rgx_lead_clock"], clock, fail=lambda e: e.lead_clock(None))
    pr.exercise("rgx_lead_clock_read", ["rgx_lead_clock_read"], lambda e: e.lead_clock_read(everyone))

    def clock_write(e):
        cell = e.lead_clock_read(everyone[:1])
        cell[0]["election_elapsed"] = 1
        e.lead_clock_write(cell)

    bad_cell = pr.on.lead_clock_read(everyone[:1])  # (read here: inside the refused call the read itself would drop the mirror)
    bad_cell[0]["election_elapsed"] = 4

    pr.exercise("rgx_lead_clock_write", ["rgx_lead_clock_write"], clock_write, fail=lambda e: e.lead_clock_write(bad_cell))
    # the term gate in front of a tick: every record of the current term (nothing is dropped, nobody deposed)
    cur = pr.on.read_column(rg.COL.CUR_TERM)

    def gate(e):
        flags = dev(np.ascontiguousarray(pr.msgs.m_flags).reshape(-1).copy())
        terms = np.zeros((P, stride), dtype=np.uint64)
        terms[:, :G] = cur[None, :G]
        self_slot = (pr.st["cfg"] >> 16) & 7
        terms[self_slot, np.arange(G)] = 0
        cols = [flags, dev(terms), torch.zeros(stride, dtype=torch.uint8, device="cuda"), torch.zeros(stride, dtype=torch.int64, device="cuda")]
        pr.keep.append(cols)
        return e.lead_gate_device(cols[0], cols[1], cols[2], cols[3])

    pr.exercise("rgt_lead_gate_device", ["rgt_lead_gate_device"], gate, fail=lambda e: e.lead_gate_device(None, None, None, None))
    # local events, both forms
    pr.exercise("rg_progress_events", ["rg_progress_events"], lambda e: e.progress_events([(g, pr.follower(g), E.EV_UNREACHABLE) for g in range(0, G, 3)]),
                fail=lambda e: e._check(e.L.rg_progress_events(e.h, None, 1)))
    slot1 = np.zeros(G, np.uint8)
    slot1[::5] = 2
    pr.exercise("rg_progress_event_dense", ["rg_progress_event_dense"], lambda e: e.progress_event_dense(E.EV_UNREACHABLE, slot1),
                fail=lambda e: e.progress_event_dense(9, slot1))
    pr.close()


# ---- the follower arena and the hand-off ---------------------------------------------------------------------------------------
def test_handoff_and_follower_calls(rg):
    import torch
    pr = Pair(rg)
    E = pr.E
    n_follow = 8
    pr.exercise("rg_follow_enable", ["rg_follow_enable"], lambda e: e.follow_enable(n_follow), fail=lambda e: e.follow_enable(n_follow))
    pr.exercise("rg_follow_gate_enable", ["rg_follow_gate_enable"], lambda e: e.follow_gate_enable(5, flags=E.GATE_CHECK_QUORUM), fail=lambda e: e.follow_gate_enable(5, flags=E.GATE_CHECK_QUORUM))
    pr.exercise("rg_follow_elect_enable", ["rg_follow_elect_enable"], lambda e: e.follow_elect_enable(), fail=lambda e: e.follow_elect_enable())
    pr.both(lambda e: e.lead_clock_enable(4, 1, E.GATE_CHECK_QUORUM | E.LEAD_CLOCK_START_LED))
    fstride = pr.on.follow_stride()
    some = np.arange(n_follow, dtype=np.uint64)
    # the reads of the arena gather on the engine's stream: they enter like any other call
    pr.exercise("arena reads", ["rg_follow_read", "rg_follow_soft_read", "rg_follow_elect_read"],
                lambda e: (e.follow_read(some), e.follow_soft_read(some), e.follow_elect_read(some)), fail=lambda e: e.follow_read(np.array([n_follow], dtype=np.uint64)))
    pr.exercise("arena getters", ["rg_follow_stride", "rg_follow_clock_counts"], lambda e: (e.follow_stride(), bool(e.follow_clock_counts())))

    # ---- the follower's own steps: they write the arena, never a leader column, and enter like any other call
    states = pr.on.follow_read(some)
    softs = pr.on.follow_soft_read(some)

    def z(dtype, n=None):
        t = torch.zeros(fstride if n is None else n, dtype=dtype, device="cuda")
        pr.keep.append(t)
        return t

    def beyond(a):
        b = a[:1].copy()
        b[0]["group"] = n_follow
        return b

    def fmsgs(**kw):
        m = {"flags": z(torch.uint8), "index": z(torch.int64), "log_term": z(torch.int64), "commit": z(torch.int64), "ent_term": z(torch.int64),
             "n_entries": z(torch.int32)}
        m.update(kw)
        return m

    def fout():
        o = {k: z(torch.int64) for k in ("index", "commit", "conflict", "reject_hint", "log_term")}
        o["status"] = z(torch.uint8)
        return o

    def elect_out():
        return {k: z(torch.uint8 if i < 6 else torch.int64) for i, k in enumerate(E.ELECT_OUT_COLUMNS)}

    pr.exercise("rg_follow_write", ["rg_follow_write"], lambda e: e.follow_write(states), fail=lambda e: e.follow_write(beyond(states)))
    pr.exercise("rg_follow_soft_write", ["rg_follow_soft_write"], lambda e: e.follow_soft_write(softs), fail=lambda e: e.follow_soft_write(beyond(softs)))
    cells = np.zeros(1, dtype=E.FOLLOW_ELECT_DTYPE)
    cells[0]["group"], cells[0]["self_id"], cells[0]["conf"] = 6, 1, E.elect_conf_make(0b111, 0, 0)
    pr.exercise("rg_follow_elect_write", ["rg_follow_elect_write"], lambda e: e.follow_elect_write(cells), fail=lambda e: e.follow_elect_write(beyond(cells)))
    hb = np.zeros(2, dtype=E.FOLLOW_MSG_DTYPE)
    hb["group"], hb["flags"] = [0, 1], E.FOLLOW_MSG_HEARTBEAT
    pr.exercise("rg_follow_step", ["rg_follow_step"], lambda e: e.follow_step(hb), fail=lambda e: e.follow_step(beyond(hb)))
    hdrs = np.zeros(2, dtype=E.FOLLOW_HDR_DTYPE)
    hdrs["term"], hdrs["from"] = 1, 2
    no_term = hdrs.copy()
    no_term["term"] = 0
    pr.exercise("rg_follow_step_gated", ["rg_follow_step_gated"], lambda e: e.follow_step_gated(hb, hdrs), fail=lambda e: e.follow_step_gated(hb, no_term))

    def step_dense(e):
        o = fout()
        e.follow_step_device(fmsgs(), o)
        e.sync()
        return o["status"]

    pr.exercise("rg_follow_step_device", ["rg_follow_step_device"], step_dense, fail=lambda e: e.follow_step_device(fmsgs(), {**fout(), "status": None}))

    def gated_dense(e, gate=True):
        o, g = fout(), z(torch.uint8)
        e.follow_step_gated_device(fmsgs(), z(torch.int64), z(torch.int64), o, g if gate else None, z(torch.uint8), z(torch.int64))
        e.sync()
        return o["status"], g

    pr.exercise("rg_follow_step_gated_device", ["rg_follow_step_gated_device"], gated_dense, fail=lambda e: gated_dense(e, gate=False))
    pr.exercise("rg_follow_clock", ["rg_follow_clock"], lambda e: e.follow_clock(z(torch.int64, 8), 8), fail=lambda e: e.follow_clock(None, 8))
    hup = np.zeros(1, dtype=E.FOLLOW_CAMPAIGN_REQ_DTYPE)
    hup[0]["group"] = 6
    pr.exercise("rg_follow_campaign", ["rg_follow_campaign"], lambda e: e.follow_campaign(hup), fail=lambda e: e.follow_campaign(beyond(hup)))

    def campaign_dense(e, n=True):
        o = elect_out()
        e.follow_campaign_device(z(torch.int64, 8), z(torch.int64, 1) if n else None, 8, o)  # (a count word of 0: no group campaigns)
        e.sync()
        return o["status"]

    pr.exercise("rg_follow_campaign_device", ["rg_follow_campaign_device"], campaign_dense, fail=lambda e: campaign_dense(e, n=False))
    vr = np.zeros(1, dtype=E.FOLLOW_VOTE_REC_DTYPE)
    vr[0]["group"], vr[0]["term"], vr[0]["from_slot"], vr[0]["kind"] = 6, 1, 1, E.FOLLOW_MSG_VOTE
    no_kind = vr.copy()
    no_kind[0]["kind"] = 0
    pr.exercise("rg_follow_vote_resps", ["rg_follow_vote_resps"], lambda e: e.follow_vote_resps(vr), fail=lambda e: e.follow_vote_resps(no_kind))

    def vote_cols(slot=True):
        m = {k: z(torch.uint8 if i < 3 else torch.int64) for i, k in enumerate(E.VOTE_COLUMNS)}
        if not slot:
            m["slot"] = None
        return m

    def resps_dense(e, slot=True):
        o = elect_out()
        e.follow_vote_resps_device(vote_cols(slot), o)
        e.sync()
        return o["status"]

    pr.exercise("rg_follow_vote_resps_device", ["rg_follow_vote_resps_device"], resps_dense, fail=lambda e: resps_dense(e, slot=False))

    def rec(f, lead):
        a = np.zeros(1, dtype=E.HANDOFF_REC_DTYPE)
        a[0]["follow_group"], a[0]["lead_group"] = f, lead
        return a

    def out_cols():
        o = {"status": torch.zeros(fstride, dtype=torch.uint8, device="cuda"), "term": torch.zeros(fstride, dtype=torch.int64, device="cuda"),
             "last_index": torch.zeros(fstride, dtype=torch.int64, device="cuda")}
        pr.keep.append(o)
        return o

    def answers(o):
        return o["status"], o["term"], o["last_index"]

    none = np.full(fstride, E.HANDOFF_NO_LEAD, np.uint64)
    # a promotion of a group that has not won its election is answered, not applied; the call enters all the same
    pr.exercise("rg_follow_promote", ["rg_follow_promote"], lambda e: e.follow_promote(rec(0, 0)), fail=lambda e: e.follow_promote(rec(n_follow, 0)))

    def promote_dense(e):
        o = out_cols()
        cols = [dev(np.zeros(fstride, np.uint8)), dev(none)]
        pr.keep.append(cols)
        e.follow_promote_device(cols[0], cols[1], o)
        e.sync()
        return answers(o)

    pr.exercise("rg_follow_promote_device", ["rg_follow_promote_device"], promote_dense, fail=lambda e: e.follow_promote_device(dev(np.zeros(fstride, np.uint8)), None, out_cols()))
    pr.exercise("rg_follow_demote", ["rg_follow_demote"], lambda e: e.follow_demote(rec(1, 11)), fail=lambda e: e.follow_demote(rec(1, G)))

    def demote_dense(e):
        o = out_cols()
        select, lead = np.zeros(fstride, np.uint8), none.copy()
        select[2], lead[2] = 1, 12
        cols = [dev(select), dev(lead)]
        pr.keep.append(cols)
        e.follow_demote_device(cols[0], cols[1], o)
        e.sync()
        return answers(o)

    pr.exercise("rg_follow_demote_device", ["rg_follow_demote_device"], demote_dense, fail=lambda e: e.follow_demote_device(dev(np.zeros(fstride, np.uint8)), None, out_cols()))
    # step-down and deposition of led groups into the arena (the lead side stops being led: clock cells, not columns)
    pr.exercise("rgx_follow_step_down", ["rgx_follow_step_down"], lambda e: e.follow_step_down(rec(3, 13)), fail=lambda e: e.follow_step_down(rec(3, G)))

    def step_down_dense(e):
        o = out_cols()
        cols = [torch.zeros(pr.on.stride, dtype=torch.uint8, device="cuda"), dev(none)]
        pr.keep.append(cols)
        e.follow_step_down_device(cols[0], cols[1], o)
        e.sync()
        return answers(o)

    pr.exercise("rgx_follow_step_down_device", ["rgx_follow_step_down_device"], step_down_dense, fail=lambda e: e.follow_step_down_device(None, None, out_cols()))

    def depose(e, lead=14):
        a = np.zeros(1, dtype=E.DEPOSE_REC_DTYPE)
        a[0]["follow_group"], a[0]["lead_group"], a[0]["term"] = 4, lead, TERM + 3
        return e.follow_depose(a)

    pr.exercise("rgt_follow_depose", ["rgt_follow_depose"], depose, fail=lambda e: depose(e, G))

    def depose_dense(e):
        o = out_cols()
        cols = [torch.zeros(pr.on.stride, dtype=torch.uint8, device="cuda"), torch.zeros(pr.on.stride, dtype=torch.int64, device="cuda"), dev(none)]
        pr.keep.append(cols)
        e.follow_depose_device(cols[0], cols[1], cols[2], o)
        e.sync()
        return answers(o)

    pr.exercise("rgt_follow_depose_device", ["rgt_follow_depose_device"], depose_dense, fail=lambda e: e.follow_depose_device(None, None, None, out_cols()))
    # the vote step: a request of a higher term for a followed group whose lead group this store leads (it is deposed); an empty
    # batch returns in front of RG_ENTER and so is no `drop` call
    def vote(e, kind=E.FOLLOW_MSG_VOTE):
        a = np.zeros(1, dtype=E.VOTE_REC_DTYPE)
        a[0]["follow_group"], a[0]["lead_group"], a[0]["term"], a[0]["from"], a[0]["kind"] = 5, 15, TERM + 5, 2, kind
        a[0]["index"], a[0]["log_term"] = int(pr.st["term_hi"][15]) + 1, TERM + 1
        return e.follow_vote(a)

    pr.exercise("rgv_follow_vote", ["rgv_follow_vote"], vote, fail=lambda e: vote(e, E.FOLLOW_MSG_APPEND))

    # the dense vote step: one request of a higher term, for followed group 7, whose lead group 16 this store leads
    def vote_dense(e, term=True):
        flags, t, frm, index, lt = (np.zeros(fstride, d) for d in (np.uint8, np.uint64, np.uint64, np.uint64, np.uint64))
        lead = none.copy()
        flags[7], t[7], frm[7], index[7], lt[7], lead[7] = E.FOLLOW_MSG_VOTE, TERM + 6, 2, int(pr.st["term_hi"][16]) + 1, TERM + 1, 16
        cols = [dev(x) for x in (flags, t, frm, index, lt, lead)]
        pr.keep.append(cols)
        o = {"status": z(torch.uint8), "gate": z(torch.uint8), "events": z(torch.uint8), "term": z(torch.int64), "commit": z(torch.int64), "log_term": z(torch.int64)}
        counts = e.follow_vote_device(fmsgs(flags=cols[0], index=cols[3], log_term=cols[4]), cols[1] if term else None, cols[2], o, lead=cols[5])
        return counts, o["status"], o["gate"], o["events"]

    pr.exercise("rgv_follow_vote_device", ["rgv_follow_vote_device"], vote_dense, fail=lambda e: vote_dense(e, term=False))

    # the deposition by a new leader's record, in front of the gated step: a heartbeat of a higher term for followed group 0 = led group 17
    def scan_dense(e, with_lead=True):
        flags, t, lead = np.zeros(fstride, np.uint8), np.zeros(fstride, np.uint64), none.copy()
        flags[0], t[0], lead[0] = E.FOLLOW_MSG_HEARTBEAT, TERM + 7, 17
        cols = [dev(x) for x in (flags, t, lead)]
        pr.keep.append(cols)
        o = out_cols()
        e.follow_depose_scan_device(cols[0], cols[1], cols[2] if with_lead else None, o)
        e.sync()
        return answers(o)

    pr.exercise("rgt_follow_depose_scan_device", ["rgt_follow_depose_scan_device"], scan_dense, fail=lambda e: scan_dense(e, with_lead=False))
    pr.close()


# ---- whole-engine calls: censuses, hints, placement, checkpoint, the stream ------------------------------------------------------
def test_whole_engine_calls(rg):
    import torch
    pr = Pair(rg)
    E = pr.E
    # (rg_restore without a checkpoint, rg_flush and the reports without a host mirror: refused states)
    pr.refuse("rg_restore", lambda e: e.restore())
    pr.refuse("rg_flush", lambda e: e.flush())
    pr.refuse("rg_report_unreachable", lambda e: e.report_unreachable(0, 1))
    pr.refuse("rg_report_snapshot", lambda e: e.report_snapshot(0, 1, True))
    pr.exercise("rg_maximal_committed_index", ["rg_maximal_committed_index"], lambda e: e.maximal_committed_index(),
                fail=lambda e: e._check(e.L.rg_maximal_committed_index(e.h, None, None)))
    pr.exercise("rg_heartbeat_commits", ["rg_heartbeat_commits"], lambda e: e.heartbeat_commits()[:, :G],
                fail=lambda e: e._check(e.L.rg_heartbeat_commits(e.h, None, None)))
    pr.exercise("rg_quorum_recently_active", ["rg_quorum_recently_active"], lambda e: e.quorum_recently_active())
    yes, no = np.full(G, 0b00011, np.uint8), np.full(G, 0b00100, np.uint8)
    pr.exercise("votes", ["rg_vote_result", "rg_tally_votes"], lambda e: (e.vote_result(yes, no), e.tally_votes(yes, no)))
    pr.exercise("rg_host_hints", ["rg_host_hints"], lambda e: e.host_hints())
    # (an empty batch returns in front of RG_ENTER; one record: maybe_decr_to of a follower, applied or found stale)
    pr.exercise("rg_resolve_host_hints", ["rg_resolve_host_hints"],
                lambda e: e.resolve_host_hints([(6, int(pr.st["next"][pr.follower(6), 6]) - 1, int(pr.st["match"][pr.follower(6), 6]), pr.follower(6), 0)]),
                fail=lambda e: e.resolve_host_hints([(G, 1, 1, 0, 0)]))
    # a group that does not exist is found by rg_read_groups' kernel, i.e. AFTER the call has entered: the one refusal here that
    # comes behind RG_ENTER ("a failed entry leaves the mirror dropped"); a NULL array is refused in front of it
    pr.exercise("rg_read_groups", ["rg_read_groups"], lambda e: e.read_groups(np.arange(G, dtype=np.uint64)), fail=lambda e: e.read_groups(np.array([G], dtype=np.uint64)),
                refused="after")
    pr.refuse("rg_read_groups, no array", lambda e: e._check(e.L.rg_read_groups(e.h, None, 1, None)))
    pr.exercise("rg_size_classes", ["rg_size_classes"], lambda e: e.size_classes(), fail=lambda e: e._check(e.L.rg_size_classes(e.h, None, 4, None)))
    # (rg_recompute, rg_checkpoint and rg_set_stream take the engine alone or accept any handle: no argument or state of an engine
    # without device Inflights makes them fail, so they have no refused form)
    pr.exercise("rg_recompute", ["rg_recompute"], lambda e: e.recompute())
    pr.exercise("rg_workload_init", ["rg_workload_init"], lambda e: e.workload_init(rg.WL_MAJORITY), fail=lambda e: e.workload_init(99))
    pr.exercise("checkpoint and restore", ["rg_checkpoint", "rg_restore"], lambda e: (e.checkpoint(), e.restore()))
    pr.exercise("rg_write_cells", ["rg_write_cells"], lambda e: e.write_cells([{"group": 2, "slot": pr.follower(2), "pr_commit": 0}]),
                fail=lambda e: e._check(e.L.rg_write_cells(e.h, None, 1)))  # (a cell of a group beyond the shard is skipped on the device, not refused)
    pr.exercise("rg_set_config", ["rg_set_config"], lambda e: e.set_config(0, int(pr.st["cfg"][0])), fail=lambda e: e.set_config(G, int(pr.st["cfg"][0])))
    pr.exercise("rg_load_column", ["rg_load_column"], lambda e: e.load_column(rg.COL.MATCH, pr.st["match"]),
                fail=lambda e: e._check(e.L.rg_load_column(e.h, rg.COL.MATCH, pr.st["match"].ctypes.data, 8)))
    perm = np.arange(G, dtype=np.uint64)
    perm[[1, 130]] = perm[[130, 1]]
    bad_perm = np.zeros(G, dtype=np.uint64)
    pr.exercise("rg_permute_groups", ["rg_permute_groups"], lambda e: e.permute_groups(perm), fail=lambda e: e.permute_groups(bad_perm))
    # place_by_size_class: rg_plan_placement on the host (no engine), rg_read_column, rg_permute_groups
    pr.exercise("place_by_size_class", ["rg_permute_groups"], lambda e: e.place_by_size_class()[0])
    # the read-only calls and the getters keep the plane
    flags_dev = dev(np.ascontiguousarray(pr.msgs.m_flags).reshape(-1).copy())
    pr.exercise("read-only calls", ["rg_results", "rg_result_counts", "rg_sync", "rg_get_device_info", "rg_msg_stats", "rg_read_column", "rgr_mirror_stats", "rg_column_bytes",
                                    "rg_stride", "rg_fused_ticks_done", "rg_mailbox_stats", "rgt_lead_gate_counts", "rgv_follow_vote_counts", "rgx_lead_clock_counts"],
                lambda e: (e.results(), e.result_counts(), e.sync(), e.device_info()["last_tick_kernel"], e.msg_stats(flags_dev.data_ptr()), e.read_column(rg.COL.MATCH),
                           e.mirror_stats()["present"] >= 0, e.L.rg_column_bytes(e.h, rg.COL.MATCH), e.stride, e.fused_ticks_done(), e.mailbox_stats(),
                           bool(e.lead_gate_counts()), bool(e.follow_vote_counts()), bool(e.lead_clock_counts())))
    cols = [torch.empty((P, pr.on.stride), dtype=torch.int64, device="cuda") for _ in range(4)] + [torch.empty((G, 8), dtype=torch.uint8, device="cuda")]
    pr.exercise("rg_workload_gen", ["rg_workload_gen"], lambda e: (e.workload_gen(rg.WL_MAJORITY, 3, *[c.data_ptr() for c in cols]), e.sync()))
    # a stream of the caller's: the ticks behind it run there
    side = torch.cuda.Stream()
    pr.exercise("rg_set_stream", ["rg_set_stream"], lambda e: (e.sync(), e.set_stream(side.cuda_stream)))
    pr.close()  # (before `side` goes)


# ---- ReadIndex -------------------------------------------------------------------------------------------------------------------
def test_read_index_calls(rg):
    import torch
    pr = Pair(rg)
    pr.exercise("rg_read_index_enable", ["rg_read_index_enable"], lambda e: e.read_index_enable(4), fail=lambda e: e.read_index_enable(4))
    pr.exercise("rg_read_index", ["rg_read_index"], lambda e: e.read_index([(g, 100 + g) for g in range(0, G, 7)]), fail=lambda e: e.read_index([(G, 1)]))
    pr.exercise("rg_read_acks", ["rg_read_acks"], lambda e: e.read_acks([(0, 100, pr.follower(0), 0)]), fail=lambda e: e.read_acks([(G, 100, 0, 0)]))

    def acks_dense(e):
        ctx = torch.zeros((P, e.stride), dtype=torch.int64, device="cuda")
        pr.keep.append(ctx)
        e.read_acks_device(ctx.data_ptr())
        e.sync()

    pr.exercise("rg_read_acks_device", ["rg_read_acks_device"], acks_dense, fail=lambda e: e.read_acks_device(None))
    pr.exercise("read queues", ["rg_read_states", "rg_read_last_pending", "rg_read_pending_counts"], lambda e: (e.read_states(), e.read_last_pending(), e.read_pending_counts()))
    pr.refuse("rg_read_states", lambda e: e._check(e.L.rg_read_states(e.h, None, 4, None)))
    pr.refuse("rg_read_last_pending", lambda e: e._check(e.L.rg_read_last_pending(e.h, None, None)))
    pr.refuse("rg_read_pending_counts", lambda e: e._check(e.L.rg_read_pending_counts(e.h, None)))
    pr.close()


# ---- the sparse roads: ingest, the one-trip tick, the flush of the host mirror, the mailbox, the fused launch --------------------
def wire(rg, recs):
    a = np.zeros(len(recs), dtype=rg.engine.WIRE_DTYPE)
    for k, (g, s, index, commit) in enumerate(recs):
        a[k]["group"], a[k]["slot"], a[k]["index"], a[k]["commit"], a[k]["flags"] = g, s, index, commit, fuzz.MF_VALID
    return a


def test_sparse_road_calls(rg):
    import torch
    pr = Pair(rg, host_mirror=True)

    def ack(g):
        s = pr.follower(g)
        return g, s, int(min(int(pr.st["term_hi"][g]), int(pr.st["match"][s, g]) + 1)), int(pr.st["commit"][g])

    # (the sparse tick leaves results of its own: the next dense tick's result words are compared all the same)
    pr.exercise("rg_ingest + rg_tick_ingested", ["rg_ingest", "rg_tick_ingested", "rg_ingested_results", "rg_ingested_duplicates"],
                lambda e: (e.ingest(wire(rg, [ack(4), ack(70)])), e.tick_ingested(), e.ingested_results(), e.ingested_duplicates()),
                fail=lambda e: e._check(e.L.rg_ingest(e.h, None, 3, None)))
    pr.exercise("rg_ingest_tick", ["rg_ingest_tick"], lambda e: e.ingest_tick(wire(rg, [ack(5), ack(129)])), fail=lambda e: e._check(e.L.rg_ingest_tick(e.h, None, 3, None, None)))

    def ingest_device(e):
        recs = torch.from_numpy(wire(rg, [ack(6)]).view(np.uint8)).cuda()
        pr.keep.append(recs)
        e.ingest_device(recs.data_ptr(), 1)
        return e.tick_ingested()

    pr.exercise("rg_ingest_device", ["rg_ingest_device", "rg_tick_ingested"], ingest_device, fail=lambda e: e.ingest_device(None, 1))

    # the host mirror: staging keeps the plane (nothing reaches the device before the flush) ...
    def stage(e, g):
        _, s, index, commit = ack(g)
        e.step(g, s + 1, TERM, index, commit=commit)

    def stage_bytes(e, g):
        _, s, index, commit = ack(g)
        e.step_bytes(g, rg.engine.encode_message({"msg_type": 4, "from": s + 1, "to": 1, "term": TERM, "index": index, "commit": commit}))  # MsgAppendResponse

    pr.exercise("staging calls", ["rg_step", "rg_step_bytes", "rg_set_peers", "rg_mark_sent"],
                lambda e: (e.set_peers(0, list(range(1, P + 1)), TERM), e.mark_sent(8, pr.follower(8) + 1), stage(e, 8), stage_bytes(e, 20)))
    # ... and the flush drops it: one record (the small flush) -- the record staged above
    pr.exercise("rg_flush, the staged records", ["rg_flush"], lambda e: e.flush())

    def local(e):
        g = 9
        me = (int(pr.st["cfg"][g]) >> 16) & 7
        hi = int(pr.st["term_hi"][g])
        e.local_append(g, hi + 1)
        e.local_persisted(g, hi + 1)
        e.step_heartbeat_response(g, pr.follower(g) + 1, TERM, commit=int(pr.st["commit"][g]))
        e.flush()
        return me

    pr.exercise("local_append, local_persisted, heartbeat response + flush", ["rg_flush"], local)
    cur = pr.on.read_column(rg.COL.CUR_TERM)

    def elect(e):
        e.local_become_leader(10, int(cur[10]) + 1)
        e.flush()

    pr.exercise("local_become_leader + flush", ["rg_flush"], elect)
    # more than RG_ROUNDTRIP_MAX (16 384) records would take the three-call road; at 193 groups x 5 slots a flush can hold 965
    # distinct cells, and rg_ingest_tick with 16 385 records of which all but a few are duplicates is what reaches that road here
    many = wire(rg, [ack(11)] * 16385)
    pr.exercise("rg_ingest_tick, three-call road", ["rg_ingest_tick"], lambda e: e.ingest_tick(many)[0])
    pr.exercise("rg_report_unreachable, rg_report_snapshot", ["rg_report_unreachable", "rg_report_snapshot"],
                lambda e: (e.report_unreachable(12, pr.follower(12) + 1), e.report_snapshot(13, pr.follower(13) + 1, True)),
                fail=lambda e: e.report_unreachable(G, 1))
    # the resident mailbox: the dense tick takes k_tick_lane while it runs (no mirror launch at all), one flush is served, and the
    # tick behind rg_mailbox_stop builds
    pr.packed_tick()
    b0, p0, _ = pr.stats()
    served = []
    for e in pr.engines:
        e.mailbox_start()
        for g in (14, 16, 18):  # (the first small flush launches the resident workgroup, the ones behind it are served)
            stage(e, g)
            e.flush()
        served.append(e.mailbox_stats()[0])
    assert min(served) >= 1, served
    assert pr.stats() == (b0, p0, 0)
    pr.resync()
    pr.tick()  # a dense tick while the mailbox is on: k_tick_lane, neither a build nor a packed launch
    assert pr.stats() == (b0, p0, 0)
    pr.both(lambda e: e.mailbox_stop())
    assert pr.stats() == (b0, p0, 0)
    pr.resync()
    pr.tick()
    assert pr.stats() == (b0 + 1, p0, 1)
    pr.close()


def test_fused_launch(rg):
    """rg_tick_device_fused: two ticks in one launch (k_tick_fused writes the columns, never the plane): the tick behind it builds"""
    import torch
    pr = Pair(rg)
    pr.packed_tick()
    b0, p0, _ = pr.stats()
    ticks, want = [], []
    for _ in range(2):
        pr.cl.store_soa(pr.st)
        pr.E.workload_gen_host(pr.st, pr.msgs, rg.WL_MAJORITY, pr.t)
        pr.t += 1
        pr.cl.tick_soa(pr.msgs.as_dict(), pr.gout)
        want.append(pr.gout.copy())
        ticks.append([dev(getattr(pr.msgs, k).copy()) for k in ("m_index", "m_commit", "m_hint", "m_rs", "m_flags")])
    pr.cl.store_soa(pr.st)
    for e in pr.engines:
        out_t = torch.zeros((2, G), dtype=torch.int32, device="cuda")
        assert e.tick_device_fused([[c.data_ptr() for c in t] for t in ticks], out_t.data_ptr()) == 2
        e.sync()
        assert (out_t.cpu().numpy().view(np.uint32) == np.array(want)).all()
    assert pr.stats() == (b0, p0, 0)
    for e in pr.engines:
        assert not fuzz.diff_states(pr.st, e.read_state(), G, P)
    pr.resync()
    pr.tick()
    assert pr.stats() == (b0 + 1, p0, 1)
    pr.refuse("rg_tick_device_fused", lambda e: e.tick_device_fused([], None))
    pr.close()


def test_handing_out_a_cached_column_switches_the_mirror_off(rg):
    """rg_column_ptr, the one `off` entry: a column the plane does not cache keeps it, a cached one ends it for good"""
    assert TABLE["rg_column_ptr"] == "off"
    pr = Pair(rg)
    pr.packed_tick()
    b0, p0, _ = pr.stats()
    pr.both(lambda e: e.column_ptr(rg.COL.NEXT))
    assert pr.stats() == (b0, p0, 1) and pr.on.mirror_stats()["off"] == 0
    pr.tick()
    assert pr.stats() == (b0, p0 + 1, 1)
    for col in (rg.COL.MATCH, rg.COL.PR_COMMIT, rg.COL.COMMIT):
        pr.both(lambda e: e.column_ptr(col))
        assert pr.stats() == (b0, p0 + 1, 0) and pr.on.mirror_stats()["off"] == 1
    pr.tick()
    pr.tick()
    assert pr.stats() == (b0, p0 + 1, 0)
    pr.close()


def test_engines_with_device_inflights_have_no_mirror(rg):
    """The `needs_inflights` entries are refused on an engine created with max_inflight == 0 (tried: the send stage and the
    Inflights dump), and the engines they run on have no plane: present == 0, no mirror launch ever."""
    assert sum(1 for c in TABLE.values() if c == "needs_inflights") >= 15
    eng = rg.Engine(G, P, flags=rg.CFGF.NO_SIZE_CLASSES, max_inflight=8)
    eng.workload_init(rg.WL_MAJORITY)
    msgs = rg.MsgBuffers(G, P, eng.stride)
    st = eng.read_state()
    rg.engine.workload_gen_host(st, msgs, rg.WL_MAJORITY, 0)
    eng.tick(msgs)
    eng.send_appends()
    eng.sync()
    s = eng.mirror_stats()
    assert (s["present"], s["plane_bytes"], s["build_launches"], s["packed_launches"], s["valid"]) == (0, 0, 0, 0, 0), s
    eng.close()
    plain = rg.Engine(G, P, flags=rg.CFGF.NO_SIZE_CLASSES)
    plain.workload_init(rg.WL_MAJORITY)
    for call in (plain.send_appends, plain.read_inflights, plain.send_items, lambda: plain.log_sizes_enable(8)):
        with pytest.raises(rg.EngineError):
            call()
    plain.close()


# ---- publication -----------------------------------------------------------------------------------------------------------------
def test_publication_every_third_tick_rides_on_a_packed_launch(rg):
    """World size 1, a host transport standing in for the all-gather (a copy of the one slice), ring_ticks 4: three ticks per
    rg_publish_commit, four publications. rg_publish_commit enters through RG_ENTER, so every cycle is one build and two packed
    launches, and the event rg_publish_commit waits for went out on the dispatch packet of the cycle's LAST tick: a packed
    launch (events_on_tick_packets grows by one per cycle). Replica and columns equal the mirror-less twin's after every
    publication."""
    import torch

    class Dev:
        def __init__(self, ptr, nbytes):
            self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (int(ptr), False), "version": 2}

    def allgather(dev_send, dev_recv, nbytes, hip_stream):
        torch.cuda.synchronize()
        torch.as_tensor(Dev(dev_recv, nbytes), device="cuda").copy_(torch.as_tensor(Dev(dev_send, nbytes), device="cuda"))
        torch.cuda.synchronize()
        return 0

    pr = Pair(rg)
    pr.both(lambda e: e.comm_init(0, 1, transport=allgather, ring_ticks=4))
    b0, p0, _ = pr.stats()
    for cycle in range(4):
        rode0 = pr.both(lambda e: e.publish_stats()["events_on_tick_packets"])
        b1, p1, _ = pr.stats()
        for k in range(3):  # (any entry point forgets the riding event, a read included: nothing between the last tick and the call)
            pr.tick(check=k < 2)
            if k == 0:  # the communicator's bookkeeping keeps the plane: the tick behind it is packed
                pr.both(lambda e: (e.comm_info(), e.publish_stats(), e.published_commit_ptr()))
        assert pr.stats() == (b1 + 1, p1 + 2, 1), (cycle, pr.stats())
        pr.both(lambda e: e.publish_commit())
        assert pr.stats()[2] == 0
        pr.check()
        rep = pr.both(lambda e: e.published_commit(0))
        a = pr.resync()
        assert (rep[0] == rep[1]).all() and (rep[0] == a["commit"]).all(), cycle
        rode = [x - y for x, y in zip(pr.both(lambda e: e.publish_stats()["events_on_tick_packets"]), rode0)]
        assert rode == [1, 1], (cycle, rode)
    pr.packed_tick()
    pr.both(lambda e: e.publish_sync())  # (rg_publish_sync on its own: it enters too)
    assert pr.stats()[2] == 0
    pr.packed_tick()
    b0, p0, _ = pr.stats()
    pr.both(lambda e: e.comm_destroy())
    assert pr.stats() == (b0, p0, 1)
    pr.tick()
    assert pr.stats() == (b0, p0 + 1, 1)
    pr.close()


def test_in_process_publication_keeps_the_mirror(rg):
    """rg_comm_init_all / rg_publish_commit_all (the engines of one process as the ranks of one publication, here the mirror
    engine and its twin): neither enters through RG_ENTER and neither writes a cached column, so the ticks around them stay
    packed; both replicas hold both ranks' commit indices."""
    pr = Pair(rg)
    E = pr.E
    assert TABLE["rg_comm_init_all"] == TABLE["rg_publish_commit_all"] == "keep"
    pr.packed_tick()
    b0, p0, _ = pr.stats()
    E.comm_init_all(list(pr.engines), ring_ticks=4)
    assert pr.stats() == (b0, p0, 1)
    pr.tick()
    assert pr.stats() == (b0, p0 + 1, 1)
    E.publish_commit_all(list(pr.engines))
    assert pr.stats() == (b0, p0 + 1, 1)
    pr.tick(check=False)
    assert pr.stats() == (b0, p0 + 2, 1)
    E.publish_commit_all(list(pr.engines))
    pr.check()
    reps = pr.both(lambda e: e.published_commit())  # (rg_published_commit waits through rg_publish_sync: a `drop` entry)
    assert pr.stats()[2] == 0
    commit = pr.resync()["commit"]
    for rep in reps:
        assert rep.shape == (2, G) and (rep[0] == commit).all() and (rep[1] == commit).all()
    pr.both(lambda e: e.comm_destroy())
    pr.close()


# the keep / drop entries the cases above go through without naming them in an exercise() list, and where
ALSO_CALLED = {"rg_tick": "Pair.tick", "rg_tick_device": "tests/test_read_mirror_edges_gpu.py (the streamed cases, the escape watch)",
               "rg_local_append": "test_sparse_road_calls", "rg_local_persisted": "test_sparse_road_calls", "rg_step_heartbeat_response": "test_sparse_road_calls",
               "rg_local_become_leader": "test_sparse_road_calls", "rg_mailbox_start": "test_sparse_road_calls", "rg_mailbox_stop": "test_sparse_road_calls",
               "rg_comm_init": "the publication test", "rg_publish_commit": "the publication test", "rg_publish_sync": "the publication test",
               "rg_published_commit": "the publication test", "rg_comm_info_get": "the publication test", "rg_publish_stats_get": "the publication test",
               "rg_published_commit_ptr": "the publication test", "rg_comm_destroy": "the publication test"}


def test_every_keep_and_drop_entry_is_called_in_this_file():
    """A new entry point classified keep or drop has to get its call here as well"""
    import re
    text = open(__file__).read()
    named = set(re.findall(r'"(rg\w?_\w+)"', text.split("ALSO_CALLED = ")[0])) | set(ALSO_CALLED)
    missing = sorted(n for n, c in TABLE.items() if c in ("keep", "drop") and n not in named)
    assert not missing, missing
