"""GPU: random sequences of the leader's control calls -- ticks with their send stage in one launch and in two, gated ticks,
re-elections, the clock, the batched conf change and the batched leader transfer in their dense and sparse forms, local events,
checkpoint / restore -- on an engine of 700 groups (two full 256-thread workgroups and a partial third) against the ONE model state of
tests/lead_sequence.py, which is never refreshed from the engine. After every step, exactly: every column of READ_COLS (RG_COL_OUT
included), every window, every clock cell, the call's answers, its item set, the reported total and the canaries behind every buffer.
A wrong cell written by step n is the engine's input of step n + 1 and the model's of none.

tests/test_lead_sequences_host.py holds the model against an oracle that lives through the whole sequence, asserts the coverage floors
of the seeds used here and shows that three slips at the hand-offs are caught. No test provokes a device fault: every forbidden call
(about one step in fifteen) is refused on the host, every bad dense cell is an answer."""
import os

import numpy as np
import pytest

import conf_model as CM
import lead_sequence as S
import oracle_lib as O
import sendstage
import transfer_model as TM

pytestmark = pytest.mark.gpu

LOAD_COLS = O.STATE_COLS + O.TERM_TABLE_COLS + ("out",)
CANARY, EV_SENT, U64_SENT = 0x7E, 0xEE, 0xA5A5A5A5A5A5A5A5
MSG_COLS = ("m_index", "m_commit", "m_hint", "m_rs", "m_flags")


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


class HostMsgs:
    """the five message columns of a tick in host memory: no m_logterm column"""

    def __init__(self, msgs):
        for k in MSG_COLS:
            setattr(self, k, np.ascontiguousarray(msgs[k]))


class Runner:
    """One engine beside the truth. form: None = every call in the form its op names; "dense" / "sparse" = that form wherever an op has
    two (a tick: one launch / two launches) -- the twins."""

    def __init__(self, rg, tr, ix64, form=None, flags=None):
        """flags: more RG_CFGF_* bits for the engine (the read-mirror cases: NO_SIZE_CLASSES, NO_READ_MIRROR)"""
        import torch
        self.rg, self.E, self.torch, self.tr, self.form = rg, rg.engine, torch, tr, form
        self.G, self.P, self.cap = tr.G, tr.P, tr.cap
        E = self.E
        if flags is not None:
            flags |= E.CFGF.IX64 if ix64 else 0
        self.eng = eng = rg.Engine(self.G, self.P, flags=(E.CFGF.IX64 if ix64 else None) if flags is None else flags, max_inflight=self.cap)
        assert eng.stride == tr.stride
        self.stride = eng.stride
        for k in LOAD_COLS:
            eng.load_column(E.COL.NAMES.index(k), tr.st[k])
        if self.cap:
            eng.load_inflights(np.zeros((self.P, self.stride), dtype=np.uint32), np.zeros((self.G, self.P, self.cap), dtype=np.uint64))
        eng.lead_clock_enable(S.CLOCK.election_tick, S.CLOCK.heartbeat_tick, E.GATE_CHECK_QUORUM | E.LEAD_CLOCK_START_LED)
        self.everyone = np.arange(self.G, dtype=np.uint64)
        self.where = None

    def close(self):
        self.eng.sync()
        self.eng.close()

    def fail(self, what, *detail):
        seed, step, name, form = self.where
        raise AssertionError("seed %d step %d op %s form %s: %s %s" % (seed, step, name, form, what, detail))

    def code(self, call):
        try:
            call()
        except self.rg.EngineError as e:
            return e.code
        return 0

    # ---- what is read back ----
    def read(self):
        st = {"n_groups": self.G, "n_slots": self.P, "stride": self.stride}
        for k in S.READ_COLS:
            st[k] = self.eng.read_column(self.E.COL.NAMES.index(k))
        return st

    def windows(self):
        """(count u32 [P][G], entries u64 [G][P][cap], oldest first) of every window, from the Inflights dump"""
        meta, ring = self.eng.read_inflights()
        m = meta[:, :self.G].astype(np.int64)
        start, count = m & 0xFFFF, m >> 16
        start = np.where(start == sendstage.INS_COMPACT, 0, start)
        idx = (start.T[:, :, None] + np.arange(self.cap)[None, None, :]) % self.cap  # [G][P][cap]
        entries = np.take_along_axis(ring, idx, axis=2)
        entries[np.arange(self.cap)[None, None, :] >= count.T[:, :, None]] = 0
        return count.astype(np.uint32), entries

    def image(self):
        """the engine as bytes: rg_read_groups of every group, the Inflights dump, the clock cells"""
        return (self.eng.read_groups(self.everyone).tobytes(), [a.tobytes() for a in self.eng.read_inflights()] if self.cap else None,
                self.eng.lead_clock_read(self.everyone).tobytes())

    def check_state(self, columns_only=False):
        """columns_only: rg_read_column alone, which keeps the dense tick's read mirror (the clock cells are read through an entry
        point that drops it) -- between the ticks of a run (lead_sequence.Chooser tick_runs)"""
        tr = self.tr
        d = S.first_diff(tr.st, self.read())
        if d:
            self.fail("column", *d)
        if columns_only:
            return
        if self.cap:
            d = S.first_window_diff(tr.win, tr.st, self.cap, *self.windows())
            if d:
                self.fail("window", *d)
        cells = self.eng.lead_clock_read(self.everyone)
        got = np.stack([cells["term"].astype(np.int64), cells["election_elapsed"].astype(np.int64), cells["heartbeat_elapsed"].astype(np.int64), cells["led"].astype(np.int64)], axis=1)
        want = np.array([[c["tag"], c["el"], c["hb"], int(c["led"])] for c in tr.cells], dtype=np.int64)
        bad = np.nonzero((got != want).any(axis=1))[0]
        if len(bad) or cells["reserved"].any() or (cells["group"] != self.everyone).any():
            g = int(bad[0]) if len(bad) else -1
            self.fail("clock cell (term, election_elapsed, heartbeat_elapsed, led)", g, None, want[g].tolist(), got[g].tolist())

    # ---- the forbidden calls ----
    def bad_call(self, bad):
        E, eng, g, P = self.E, self.eng, bad["group"], self.P
        conf = lambda recs, **kw: (lambda: eng.apply_conf(self.conf_recs(recs), **kw))  # noqa: E731
        xfer = lambda recs, **kw: (lambda: eng.transfer_leader(self.transfer_recs(recs), **kw))  # noqa: E731
        W = CM.word(1)
        cell = np.zeros(1, dtype=E.LEAD_CLOCK_CELL_DTYPE)
        cell[0]["group"], cell[0]["term"], cell[0]["election_elapsed"], cell[0]["led"] = g, S.TERM, S.CLOCK.election_tick, 1
        call = {"conf_owed": conf([(g, W)]), "transfer_owed": xfer([(g, 0)]), "conf_twice": conf([(g, W), (g, W)]), "conf_beyond": conf([(self.G, W)]),
                "conf_malformed": conf([(g, 1 << 24)]), "conf_flags": conf([(g, W)], flags=4), "conf_bytes": conf([(g, W)], flags=2),
                "transfer_slot": xfer([(g, P)]), "transfer_twice": xfer([(g, 0), (g, 0)]), "transfer_flags": xfer([(g, 0)], flags=1),
                "transfer_bytes": xfer([(g, 0)], flags=2),
                "clock_enable_again": lambda: eng.lead_clock_enable(S.CLOCK.election_tick, S.CLOCK.heartbeat_tick, E.GATE_CHECK_QUORUM),
                "clock_write_elapsed": lambda: eng.lead_clock_write(cell)}[bad["call"]]
        before = (self.image(), self.read())
        got = self.code(call)
        if got != E.ERR[S.BAD_CALLS[bad["call"]]]:
            self.fail("the forbidden call " + bad["call"], "wanted", S.BAD_CALLS[bad["call"]], "got", got)
        if before[0] != self.image() or S.first_diff(before[1], self.read()):
            self.fail("the refused call " + bad["call"] + " changed the engine")

    # ---- the ops ----
    def apply(self, seed, step, op, want):
        form = self.form or {"tick": "one launch" if op.get("launches") == 1 else "two launches", "conf": "dense" if op.get("dense") else "sparse",
                             "transfer": "dense" if op.get("dense") else "sparse", "events": op.get("form")}.get(op["kind"], "-")
        self.where = (seed, step, op["name"], form)
        if op["bad"] and op["bad"]["when"] == "before":
            self.bad_call(op["bad"])
        getattr(self, "_" + op["kind"])(op, want, form in ("dense", "one launch"))
        self.check_state(columns_only=bool(op.get("columns_only")))

    def check_gate(self, want, got_rows, in_rows, flags, events, new_term, down, counts, alias):
        G = self.G
        if counts != want["counts"]:
            self.fail("gate counts", want["counts"], counts)
        ev = events.cpu().numpy()
        bad = np.nonzero(ev[:G] != np.array(want["events"], dtype=np.uint8))[0]
        if len(bad):
            self.fail("gate event", int(bad[0]), None, want["events"][bad[0]], int(ev[bad[0]]))
        rows = got_rows.cpu().numpy()
        bad = np.argwhere(rows[:G * 8].reshape(G, 8) != want["rows"])
        if len(bad):
            self.fail("gate row", int(bad[0][0]), int(bad[0][1]), int(want["rows"][tuple(bad[0])]), int(rows[:G * 8].reshape(G, 8)[tuple(bad[0])]))
        assert (ev[G:] == EV_SENT).all() and (rows[G * 8:] == EV_SENT).all(), self.where
        if not alias:
            assert (in_rows.cpu().numpy()[:G * 8].reshape(G, 8) == flags).all(), self.where  # the input rows are read only
        nt = new_term.cpu().numpy().view(np.uint64)
        wanted = np.array([U64_SENT if t is None else t for t in want["new_term"]], dtype=np.uint64)
        bad = np.nonzero(nt[:G] != wanted)[0]
        if len(bad) or (nt[G:] != U64_SENT).any():
            self.fail("gate new_term", int(bad[0]) if len(bad) else -1)
        deposed = {g for g, e in enumerate(want["events"]) if e & 0x80}
        lst = [int(x) for x in down.cpu().numpy().view(np.uint64)]
        if set(lst[:len(deposed)]) != deposed or any(x != U64_SENT for x in lst[len(deposed):]):
            self.fail("gate list of deposed groups", sorted(deposed)[:5], lst[:5])

    def _tick(self, op, want, one):
        torch, eng, G, cap = self.torch, self.eng, self.G, self.cap
        m, me, skip = op["msgs"], op["max_entries"], op["skip"]
        owed = op["bad"] if op["bad"] and op["bad"]["when"] == "owed" else None
        keep = None
        if op["terms"] is None and (cap or one):
            host = HostMsgs(m)
            if cap and one:
                eng.tick_send(host, me, skip_bcast_commit=skip)
            else:
                eng.tick(host)
        else:  # device buffers: a gated tick, and the second tick form of an engine without device Inflights
            keep = [dev(m[k]) for k in MSG_COLS[:4]]
            flags = torch.full((G * 8 + 64,), EV_SENT, dtype=torch.uint8, device="cuda")
            flags[:G * 8] = dev(m["m_flags"].reshape(-1))
            rows = flags
            if op["terms"] is not None:
                rows = flags if one else torch.full((G * 8 + 64,), EV_SENT, dtype=torch.uint8, device="cuda")  # one launch: in place
                events = torch.full((self.stride + 8,), EV_SENT, dtype=torch.uint8, device="cuda")
                new_term = torch.full((self.stride + 8,), U64_SENT - (1 << 64), dtype=torch.int64, device="cuda")
                down = torch.full((G + 4,), U64_SENT - (1 << 64), dtype=torch.int64, device="cuda")
                terms = dev(op["terms"])
                torch.cuda.synchronize()
                counts = eng.lead_gate_device(flags, terms, events, new_term, None if one else rows, down, G)
                eng.sync()
                self.check_gate(want["gate"], rows, flags, m["m_flags"], events, new_term, down, counts, one)
                keep += [terms, events, new_term, down]
            torch.cuda.synchronize()
            ptrs = [t.data_ptr() for t in keep[:4]] + [rows.data_ptr()]
            if cap and one:
                eng.tick_device_send(*ptrs, max_entries_per_msg=me, skip_bcast_commit=skip)
            else:
                eng.tick_device(*ptrs)
            eng.sync()
            keep += [flags, rows]
        if cap and not one:
            if owed:
                self.bad_call(owed)
            eng.send_appends(me, skip_bcast_commit=skip)
        eng.sync()
        del keep
        if cap:
            d = S.diff_items(want["items"], sendstage.items_dict(eng.send_items()))
            if d:
                self.fail("send item", d[0][0], d[0][1], d[1], d[2])

    def _clock(self, op, want, _):
        torch, eng, G, P = self.torch, self.eng, self.G, self.P
        beats, downs = [g for g, e in enumerate(want["events"]) if e & 1], [g for g, e in enumerate(want["events"]) if e & 4]
        beat_cap, down_cap = (G if op["beat_cap"] is None else op["beat_cap"]), (G if op["down_cap"] is None else op["down_cap"])
        events = torch.full((self.stride,), EV_SENT, dtype=torch.uint8, device="cuda")
        beat = torch.full((beat_cap + 3,), U64_SENT - (1 << 64), dtype=torch.int64, device="cuda")
        down = torch.full((down_cap + 3,), U64_SENT - (1 << 64), dtype=torch.int64, device="cuda")
        hbc = torch.full((P, self.stride), U64_SENT - (1 << 64), dtype=torch.int64, device="cuda") if op["hb"] else None
        torch.cuda.synchronize()
        counts = eng.lead_clock(events, beat if beat_cap else None, beat_cap, down if down_cap else None, down_cap, hbc)
        if counts != want["counts"]:
            self.fail("clock counts (beats, check-quorum runs, step-downs, transfers aborted)", want["counts"], counts)
        ev = events.cpu().numpy()
        bad = np.nonzero(ev[:G] != np.array(want["events"], dtype=np.uint8))[0]
        if len(bad) or (ev[G:] != EV_SENT).any():
            g = int(bad[0]) if len(bad) else -1
            self.fail("clock event", g, None, want["events"][g], int(ev[g]))
        for name, buf, cap, full in (("beat", beat, beat_cap, beats), ("down", down, down_cap, downs)):
            lst = [int(x) for x in buf.cpu().numpy().view(np.uint64)]
            k = min(cap, len(full))
            if len(set(lst[:k])) != k or not set(lst[:k]) <= set(full) or any(x != U64_SENT for x in lst[k:]) or (cap >= len(full) and set(lst[:k]) != set(full)):
                self.fail("clock list " + name, full[:5], lst[:5])
        if op["hb"]:  # written only under EV_BEAT
            h = hbc.cpu().numpy().view(np.uint64)
            wanted = np.full((P, self.stride), U64_SENT, dtype=np.uint64)
            for g, row in want["hb"].items():
                wanted[:, g] = row
            bad = np.argwhere(h != wanted)
            if len(bad):
                s, g = (int(v) for v in bad[0])
                self.fail("hb_commit", g, s, int(wanted[s, g]), int(h[s, g]))

    def conf_recs(self, recs):
        a = np.zeros(len(recs), dtype=self.E.CONF_REC_DTYPE)
        for k, (g, W) in enumerate(recs):
            a[k]["group"], a[k]["cfg"] = g, W
        return a

    def transfer_recs(self, recs):
        a = np.zeros(len(recs), dtype=self.E.TRANSFER_REC_DTYPE)
        for k, (g, t) in enumerate(recs):
            a[k]["group"], a[k]["slot"] = g, t
        return a

    def check_answers(self, recs, answers, got, fields):
        for k, ((g, _), a) in enumerate(zip(recs, answers)):
            for f in fields:
                if int(got[f][k]) != a[f] & S.U64:
                    self.fail("answer " + f, g, None, a[f], int(got[f][k]))

    def check_items(self, op, want, items, total):
        if total != want["total"]:
            self.fail("item total", want["total"], total)
        if len(items) != min(total, op["item_cap"]):
            self.fail("items written", min(total, op["item_cap"]), len(items))
        got = sendstage.items_dict(items)  # (asserts that no peer appears twice)
        d = S.diff_items(want["items"], got, strict=True, subset=len(items) < total)
        if d:
            self.fail("item", d[0][0], d[0][1], d[1], d[2])

    def dense_call(self, op, want, sel_col, extra_cols, call, fields):
        """the dense form of the conf change / the transfer: canaries behind G and behind item_cap, the cells of unselected groups"""
        torch, G, cap = self.torch, self.G, self.cap
        recs, room = op["recs"], op["item_cap"] if cap else 0
        out = {"status": torch.full((G + 64,), CANARY, dtype=torch.uint8, device="cuda"), "events": torch.full((G + 64,), CANARY, dtype=torch.uint8, device="cuda")}
        if "commit" in fields:
            out["commit"] = torch.full((G + 64,), -1, dtype=torch.int64, device="cuda")
        buf = torch.full(((room + 2) * 32,), CANARY, dtype=torch.uint8, device="cuda") if cap else None  # two items of canary behind item_cap
        count = torch.full((2,), 0x55555555, dtype=torch.int32, device="cuda") if cap else None
        cols = [dev(c) for c in (sel_col,) + extra_cols]
        torch.cuda.synchronize()
        call(cols, out, buf if room else None, room, count)
        self.eng.sync()
        got = {k: v.cpu().numpy() for k, v in out.items()}
        if "commit" in got:
            got["commit"] = got["commit"].view(np.uint64)
        picked = np.zeros(G, dtype=bool)
        picked[[g for g, _ in recs]] = True
        for k, v in got.items():
            untouched = 0 if k == "status" else S.U64 if k == "commit" else CANARY  # (status: NONE for an unselected group)
            bad = np.nonzero((v[:G] != untouched) & ~picked)[0]
            if len(bad) or (v[G:] != (S.U64 if k == "commit" else CANARY)).any():
                self.fail("dense " + k + " cell of an unselected group, or the canary behind G", int(bad[0]) if len(bad) else -1)
        idx = [g for g, _ in recs]
        self.check_answers(recs, want["answers"], {k: v[idx] for k, v in got.items()}, fields)
        if not cap:
            return
        words = count.cpu().numpy().view(np.uint32)
        raw = buf.cpu().numpy()
        total = int(words[0])
        k = min(total, room)
        if int(words[1]) != 0x55555555 or (raw[k * 32:] != CANARY).any():
            self.fail("a write behind the count word or behind the items written", total, room)
        self.check_items(op, want, raw[:k * 32].view(self.E.SEND_ITEM_DTYPE).copy(), total)

    def _conf(self, op, want, dense):
        eng, recs = self.eng, op["recs"]
        if dense:
            sel, cfg = np.zeros(self.G, np.uint8), np.full(self.G, 0xA5A5A5A5, np.uint32)  # (an unselected word is never read: it is malformed)
            for g, W in recs:
                sel[g], cfg[g] = 1 + g % 255, W
            self.dense_call(op, want, sel, (cfg,), lambda c, o, buf, room, count: eng.apply_conf_device(c[0], c[1], o["status"], o["events"], o["commit"], buf, room, count,
                                                                                                      op["max_entries"], 0), ("status", "events", "commit"))
            return
        resp, items, total = eng.apply_conf(self.conf_recs(recs), op["max_entries"], 0, op["item_cap"] if self.cap else None)
        self.check_answers(recs, want["answers"], resp, ("commit", "last_index", "cfg", "out", "n_items", "status", "events", "added", "removed"))
        if self.cap:
            self.check_items(op, want, items, total)

    def _transfer(self, op, want, dense):
        eng, recs = self.eng, op["recs"]
        if dense:
            to = np.zeros(self.G, np.uint8)
            for g, t in recs:
                to[g] = t + 1
            self.dense_call(op, want, to, (), lambda c, o, buf, room, count: eng.transfer_leader_device(c[0], o["status"], o["events"], buf, room, count, op["max_entries"], 0),
                            ("status", "events"))
            return
        resp, items, total = eng.transfer_leader(self.transfer_recs(recs), op["max_entries"], 0, op["item_cap"] if self.cap else None)
        if resp["reserved"].any() or resp["reserved2"].any():
            self.fail("a reserved field of a transfer response is not 0")
        self.check_answers(recs, want["answers"], resp, ("last_index", "matched", "cfg", "n_items", "status", "events", "previous"))
        if self.cap:
            self.check_items(op, want, items, total)

    def _events(self, op, want, dense):
        if dense and "slot1" in op:
            self.eng.progress_event_dense(op["ev_kind"], op["slot1"])
        else:
            self.eng.progress_events(op["events"])

    def _checkpoint(self, op, want, _):
        self.eng.checkpoint()

    def _restore(self, op, want, _):
        self.eng.restore()


_CASES = [(S.SEEDS[c],) + c for c in S.CASES] + [(300 + i, (3, 5, 8)[i % 3], bool(i % 2), (1, 4, 8, 0)[i % 4]) for i in range(int(os.environ.get("RG_SOAK_SEEDS", "0")))]


# (RG_SOAK_SEEDS=n adds n more seeded cases: an ad hoc soak; their coverage floors are not asserted)
@pytest.mark.parametrize("seed,P,ix64,cap", _CASES)
def test_random_sequences_of_leader_control_calls_match_the_model(rg, seed, P, ix64, cap):
    """Forty steps on 700 groups; slot counts 3, 5 and 8, max_inflight 0 (no items, the events-only road of the transfer, no stage),
    1, 4 and 8, 32- and 64-bit cell offsets (RG_CFGF_IX64 forces the 64-bit instantiations at this size)."""
    tr, ch = S.Truth(seed, P, cap), S.Chooser(seed, P, cap)
    run = Runner(rg, tr, ix64)
    try:
        run.where = (seed, -1, "load", "-")
        run.check_state()
        for step in range(S.STEPS):
            op = ch.next(tr)
            want = tr.apply(op)
            run.apply(seed, step, op, want)
    finally:
        run.close()


def test_dense_and_sparse_twins_stay_byte_equal(rg):
    """One seed on two engines: the first takes the dense form wherever an op has two (a tick and its stage: one launch), the second
    the sparse form (two launches). After every step both equal the model, and each other byte for byte: rg_read_groups of every
    group, the Inflights dump, the clock cells."""
    (P, ix64, cap), seed = S.TWIN_CASE, S.TWIN_SEED
    tr, ch = S.Truth(seed, P, cap), S.Chooser(seed, P, cap, twin=True)
    a, b = Runner(rg, tr, ix64, "dense"), Runner(rg, tr, ix64, "sparse")
    try:
        for step in range(S.STEPS):
            op = ch.next(tr)
            want = tr.apply(op)
            for run in (a, b):
                run.apply(seed, step, op, want)
            ia, ib = a.image(), b.image()
            for what, x, y in zip(("rg_read_groups", "the Inflights dump", "the clock cells"), ia, ib):
                assert x == y, "seed %d step %d op %s: %s of the dense and the sparse twin differ" % (seed, step, op["name"], what)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("P,seed", S.MIRROR_CASES)
def test_sequences_with_packed_launches_match_the_model_and_a_mirror_less_twin(rg, P, seed):
    """max_inflight 0, 32-bit offsets, no size classes: the engines whose dense tick is k_tick_mirror. One engine with the read
    mirror, one created with RG_CFGF_NO_READ_MIRROR, the same model, never refreshed from either. The chooser emits runs of 2-4
    plain ticks behind which only columns are read, so ticks find their plane valid -- and so does the call behind a run, which
    has to drop it. After every step both engines equal the
    model; after every step with a full check their images are byte-equal; and rgr_mirror_stats is what readmirror.after predicts
    from the op sequence alone -- build and packed launches and the flag, after every step."""
    import readmirror as RM
    E = rg.engine
    tr, ch = S.Truth(seed, P, 0), S.Chooser(seed, P, 0, tick_runs=True)
    on = Runner(rg, tr, False, flags=E.CFGF.NO_SIZE_CLASSES)
    off = Runner(rg, tr, False, flags=E.CFGF.NO_SIZE_CLASSES | E.CFGF.NO_READ_MIRROR)
    try:
        assert on.eng.mirror_stats()["present"] == 1 and off.eng.mirror_stats()["present"] == 0
        for run in (on, off):
            run.where = (seed, -1, "load", "-")
            run.check_state()
        build = packed = step = 0
        valid = False
        while not ch.done():
            op = ch.next(tr)
            want = tr.apply(op)
            for run in (on, off):
                run.apply(seed, step, op, want)
            build, packed, valid = RM.launch_counts(S.mirror_classes(op, first=step == 0), valid, build, packed)
            s = on.eng.mirror_stats()
            assert (s["build_launches"], s["packed_launches"], s["valid"], s["off"]) == (build, packed, int(valid), 0), (seed, step, op["name"], s, build, packed, valid)
            s = off.eng.mirror_stats()
            assert (s["build_launches"], s["packed_launches"], s["valid"]) == (0, 0, 0), s
            if op["kind"] == "tick":
                info = on.eng.device_info()
                assert info["last_tick_kernel"] == rg.KERNEL.NAMES[rg.KERNEL.LANE] and info["last_tick_offset_bits"] == 32, info
            if not op.get("columns_only"):  # (the images are read through entry points that drop the mirror: not behind a plain tick)
                for what, x, y in zip(("rg_read_groups", "the Inflights dump", "the clock cells"), on.image(), off.image()):
                    assert x == y, "seed %d step %d op %s: %s of the mirror engine and its twin differ" % (seed, step, op["name"], what)
            step += 1
        assert (build, packed) == S.MIRROR_LAUNCHES[(P, seed)], (build, packed)
        S.check_floors(tr.cov, 0)
    finally:
        on.close()
        off.close()
