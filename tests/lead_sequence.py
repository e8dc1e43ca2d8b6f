"""Random SEQUENCES of the leader's control calls and their model: ONE state of the truth carried through a whole sequence, never
refreshed from an engine.

The six leader-side steps that live on the device -- the clock (rgx_lead_clock), the term gate (rgt_lead_gate_device), the tick with
its send stage, the batched conf change (rgc_apply_conf*), the batched leader transfer (rgm_transfer_leader*) and the local events --
each have a literal model (tests/lead_clock_model.py, term_gate_model.py, conf_model.py, transfer_model.py, the C oracle). Here they
are composed:

    Truth     handoff_rig's SoA dict (R.ALL_COLS + out + host_hint), the window dict {(group, slot): [entries oldest first]}, one clock
              cell {"tag", "hb", "el", "led"} per group, and a checkpoint copy of all three. Truth.apply(op) moves it by the models
              alone and returns what the call has to answer.
    Chooser   a seeded generator that picks the next op FROM THE TRUTH'S STATE ALONE: the same seed gives the same sequence whether
              an engine, the continuous oracle of tests/test_lead_sequences_host.py, or nothing at all runs beside it.
    Coverage  what a sequence reached, counted on the model: the floors of check_floors are conditions on the committed seeds.

Density. A conf change or a transfer selects a few groups, about 40 % of all groups, or every group of workgroups 0 and 1 and none of
workgroup 2; item_cap is exact, one short, cut inside the second workgroup's share, or 0. The generator is weighted so that the item
lists get as long as they can: the groups without a Progress of their own lie in workgroup 2, and every group of workgroups 0 and 1
has one peer that is owed a message (shape_workgroups); step 0 is a dense transfer in which every lane of workgroup 1 owes its item,
step 1 a dense conf change in which every lane of workgroup 0 owes items and every lane of its wave 0 all P - 1 (the word leaves the
leader the only voter and gives every slot a Progress: the commit index moves and bcast_append follows); later a transfer names, six
times in ten, a lagging voter that is not paused, and one conf word in eight is that leader-alone word again.

A tick's truth is the C oracle: a FRESH O.Cluster loaded from the truth's state (windows re-added with ro_ins_add), ro_tick_soa,
ro_send_stage_soa, ro_store_soa back into the truth. tests/test_lead_sequences_host.py shows that this reload-per-tick executor loses
nothing that an oracle which lives through the whole sequence keeps outside the SoA.

What is compared and what is not. Every scalar column of every group; the per-slot columns and the flag bytes of every slot that has
a Progress (RG_CFG_PRESENT of the truth's cfg word AFTER the step: the cells of a slot without one are without meaning until
apply_conf adds it again, which rewrites all of them -- include/raftgroups_conf.h); the window of every Progress in Replicate (the
reference keeps the Inflights of the others empty, the engine clears them lazily when the send stage next looks at the peer:
tests/sendstage.py compare_rings)."""
import ctypes

import numpy as np

import conf_model as CM
import fuzz
import handoff_rig as R
import lead_clock_model as L
import oracle_lib as O
import sendstage
import term_gate_model as T
import transfer_model as TM

TERM, G_DEFAULT, STEPS, BLOCK = 5, 700, 40, 256
CLOCK = L.Config(4, 1, L.CHECK_QUORUM | L.START_LED)
READ_COLS = R.ALL_COLS + ("out", "host_hint")
SLOT_COLS = ("match", "next", "pr_commit", "pend_snap", "pend_rs", "gid")
U64 = (1 << 64) - 1
MF_BECOME_LEADER, OUT_TIMEOUT_NOW = 0x02, 0x4
# (P, ix64, max_inflight) of the GPU file, and the seed each of them runs (chosen on the CPU so that check_floors holds)
CASES = [(3, False, 1), (3, True, 8), (5, False, 8), (5, True, 1), (8, False, 4), (5, False, 0)]
SEEDS = {(3, False, 1): 2, (3, True, 8): 2, (5, False, 8): 3, (5, True, 1): 2, (8, False, 4): 1, (5, False, 0): 1}
TWIN_CASE, TWIN_SEED = (5, False, 8), 2
# (P, seed) of the read-mirror sequences (tests/test_lead_sequences_gpu.py): max_inflight 0, 32-bit offsets, no size classes, the
# chooser with tick_runs -- runs of 2-4 consecutive plain ticks, so that the dense tick finds its plane valid (packed launches)
# Seeds with fewer than RG_MIRROR_WINDOW = 32 mirror launches in all: the engine's escape watch never takes a look. (It would switch
# the mirror off on this stream, rightly: half of fuzz.random_msgs' acks carry Message.commit = commit + 1, a committed_index ABOVE
# the commit index, which the packed word cannot hold, so most waves store an escape.)
MIRROR_CASES = [(3, 1), (5, 5)]
MIRROR_LAUNCHES = {(3, 1): (11, 19), (5, 5): (10, 20)}  # (build, packed) launches of the mirror-on engine: floors of the seeds

DECK = (["tick_one"] * 3 + ["tick_two"] * 3 + ["gated_one"] * 2 + ["gated_two"] * 2 + ["reelect"] * 3 + ["clock"] * 9 + ["conf_dense"] * 3 +
        ["conf_sparse"] * 2 + ["transfer_dense"] * 3 + ["transfer_sparse"] * 2 + ["events_records"] * 2 + ["events_dense"] * 2 +
        ["checkpoint"] * 2 + ["restore"] * 2)
assert len(DECK) == STEPS
OP_NAMES = sorted(set(DECK))
TRANSFER_STATUSES = {TM.STARTED, TM.SELF, TM.IN_PROGRESS, TM.LEARNER, TM.NO_PROGRESS, TM.NOT_LED, TM.FAULT}
CONF_STATUSES = {CM.DONE, CM.DEMOTED, CM.NOT_LED, CM.HOST, CM.FAULT}
# the calls a state forbids: name -> the documented error (include/raftgroups_conf.h, _transfer.h, _lead.h: "State rules")
BAD_CALLS = {"conf_owed": "STATE", "transfer_owed": "STATE", "conf_twice": "INVALID_ARG", "conf_beyond": "INVALID_ARG", "conf_malformed": "INVALID_ARG",
             "conf_flags": "INVALID_ARG", "conf_bytes": "STATE", "transfer_slot": "INVALID_ARG", "transfer_twice": "INVALID_ARG", "transfer_flags": "INVALID_ARG",
             "transfer_bytes": "STATE", "clock_enable_again": "STATE", "clock_write_elapsed": "INVALID_ARG"}


def copy_windows(win):
    return None if win is None else {k: list(v) for k, v in win.items()}


def copy_cells(cells):
    return [dict(c) for c in cells]


def run_count_of(st):
    return (st["run_first"][:, :st["n_groups"]] != 0).sum(axis=0).astype(np.uint8)


def initial_state(rng, G, P, cap):
    """The state test_random_api_sequences_with_the_send_stage starts from, about a tenth of the groups without a Progress of their
    own slot, a few joint, about a tenth with a transferee; the cells of slots without a Progress are zero and the flag bytes are
    what the oracle stores for what it was given (the engine derives its own bits of a loaded row the same way).

    WHERE the random draws land is weighted so that whole workgroups can owe items (shape_workgroups): the groups without a Progress
    of their own all lie in workgroup 2."""
    st = O.add_term_table(O.alloc_state(G, P))
    st["cfg"][:] = fuzz.random_cfg(rng, G, P, joint_frac=0.06, transfer_frac=0.1)
    fuzz.random_state(rng, st, small_values=True)
    empty = np.arange(G) < BLOCK
    st["term_lo"][empty] = np.minimum(st["term_lo"][empty], st["term_hi"][empty])  # (workgroup 0: an entry of the leader's term to commit)
    fuzz.random_term_table(rng, st, TERM)
    sendstage.mark_pending_conf(rng, st)
    cfg = st["cfg"].astype(np.int64)
    lose = (rng.random(G) < 0.1 * G / max(G - 2 * BLOCK, 1)) & (np.arange(G) >= 2 * BLOCK)
    cfg[lose] &= ~(1 << (24 + (cfg[lose] >> 16 & 7)))
    st["cfg"][:] = cfg.astype(np.uint32)
    shape_workgroups(st)
    cfg = st["cfg"].astype(np.int64)
    for s in range(P):
        absent = (cfg >> (24 + s) & 1) == 0
        for k in SLOT_COLS:
            st[k][s, :G][absent] = 0
        st["pflags"][absent, s] = 0
    cl = O.Cluster(G)
    cl.load_soa(st, term=TERM, max_inflight=cap)
    cl.set_own_inflights(bool(cap))
    cl.store_soa(st)
    st["run_count"] = run_count_of(st)
    st["out"] = np.zeros(G, dtype=np.uint32)
    st["host_hint"] = np.zeros(G, dtype=np.uint8)
    return st


def shape_workgroups(st):
    """Every group of workgroups 0 and 1 gets one peer a call owes a message whatever else the draw gave it -- the slot behind the
    leader's: a voter with a Progress, in Replicate, recently active, one entry behind, not the transferee. In workgroup 0 the
    leader has persisted its whole log and the commit index is behind it (a word that leaves the leader the only voter then
    commits, and bcast_append follows); in its wave 0 every peer is in Replicate and recently active with nothing pending, so
    that every lane of the wave owes all P - 1 of them."""
    G, P = st["n_groups"], st["n_slots"]
    for g in range(min(G, 2 * BLOCK)):
        cfg, hi = int(st["cfg"][g]), int(st["term_hi"][g])
        me = cfg >> 16 & 7
        t = (me + 1) % P
        cfg |= 1 << t | 1 << (24 + t) | 1 << (24 + me)
        if cfg >> 20 & 0xF == t + 1:
            cfg &= ~(0xF << 20)
        st["cfg"][g] = cfg
        st["match"][t, g], st["next"][t, g], st["pend_snap"][t, g], st["pend_rs"][t, g] = hi - 1, hi, 0, 0
        st["pflags"][g, t] = O.REPLICATE | CM.PF_RECENT_ACTIVE
        if g < BLOCK:
            st["match"][me, g], st["next"][me, g] = hi, hi + 1
            st["commit"][g] = min(int(st["commit"][g]), hi - 1)
        if g < 64:
            for s in range(P):
                if s != me:
                    st["pflags"][g, s], st["pend_snap"][s, g], st["pend_rs"][s, g] = O.REPLICATE | CM.PF_RECENT_ACTIVE, 0, 0
        for s in range(P):
            st["pr_commit"][s, g] = min(int(st["commit"][g]), int(st["match"][s, g]))


def add_windows(cl, win, st):
    """ro_ins_add of every entry of every window of a slot that has a Progress, oldest first"""
    for (g, s), entries in win.items():
        if entries and int(st["cfg"][g]) >> 24 >> s & 1:
            ins = ctypes.byref(cl.L.ro_group_progress(cl.h, g, s + 1).contents.ins)
            for e in entries:
                cl.L.ro_ins_add(ins, e)


def export_windows(cl, win, st, cap):
    """every window of the cluster into the dict (a slot without a Progress keeps what the dict held: it is without meaning)"""
    G, P = st["n_groups"], st["n_slots"]
    counts, first, _ = cl.ins_export(P, st["stride"], k=cap)
    for g, s in list(win):
        if int(st["cfg"][g]) >> 24 >> s & 1:
            del win[(g, s)]
    ss, gg = np.nonzero(counts[:, :G])
    for s, g in zip(ss.tolist(), gg.tolist()):
        win[(g, s)] = [int(x) for x in first[g, s, :counts[s, g]]]


def coalesce(sent):
    """the oracle's messages as the engine's items; a snapshot item is compared by kind and prev_index only (its last_index carries
    the requested index: tests/sendstage.py compare_items)"""
    return {k: (v[0], v[1] & U64, v[2] & U64, v[3]) for k, v in sendstage.coalesce_oracle(sent).items()}


def same_item(a, b, strict=False):
    """strict: a call's own items (conf change, transfer), whose model is exact; else a stage's, where a snapshot item is compared by
    kind and prev_index only"""
    if a is None or b is None:
        return a is b
    if not strict and a[0] == O.SEND_SNAPSHOT and b[0] == O.SEND_SNAPSHOT:
        return a[1] & U64 == b[1] & U64
    return (a[0], a[1] & U64, a[2] & U64, a[3]) == (b[0], b[1] & U64, b[2] & U64, b[3])


def diff_items(want, got, strict=False, subset=False):
    """the first (group, slot) at which two item dicts differ, or None; subset: `got` is a list cut by item_cap -- every item of it
    has to be one of `want`"""
    for k in sorted(set(got) if subset else set(want) | set(got)):
        if not same_item(want.get(k), got.get(k), strict):
            return k, want.get(k), got.get(k)
    return None


def first_diff(want, got, cols=READ_COLS):
    """(column, group, slot, wanted, got) of the first cell in which `got` differs from the truth's state `want`, or None; per-slot
    cells only where the truth's cfg word has a Progress"""
    G, P = want["n_groups"], want["n_slots"]
    present = (want["cfg"].astype(np.int64) >> 24) & 0xFF
    mask = np.stack([(present >> s & 1).astype(bool) for s in range(P)])  # [P][G]
    for k in cols:
        x, y = want[k], got[k]
        if k in SLOT_COLS:
            bad = np.argwhere((x[:P, :G] != y[:P, :G]) & mask)
            if len(bad):
                s, g = (int(v) for v in bad[0])
                return k, g, s, int(x[s, g]), int(y[s, g])
        elif k == "pflags":
            bad = np.argwhere((x[:G, :P] != y[:G, :P]) & mask.T)
            if len(bad):
                g, s = (int(v) for v in bad[0])
                return k, g, s, int(x[g, s]), int(y[g, s])
        elif k in ("run_first", "run_term"):
            bad = np.argwhere(x[:, :G] != y[:, :G])
            if len(bad):
                r, g = (int(v) for v in bad[0])
                return k, g, r, int(x[r, g]), int(y[r, g])
        else:
            bad = np.nonzero(x[:G] != y[:G])[0]
            if len(bad):
                g = int(bad[0])
                return k, g, None, int(x[g]), int(y[g])
    return None


def replicate_mask(st):
    """[P][G]: the slots whose window is compared: a Progress in Replicate"""
    G, P = st["n_groups"], st["n_slots"]
    present = (st["cfg"].astype(np.int64) >> 24) & 0xFF
    return np.stack([(present >> s & 1).astype(bool) & ((st["pflags"][:G, s] & 3) == O.REPLICATE) for s in range(P)])


def window_arrays(win, st, cap):
    """the window dict as (count u32 [P][G], entries u64 [G][P][cap])"""
    G, P = st["n_groups"], st["n_slots"]
    count, entries = np.zeros((P, G), dtype=np.uint32), np.zeros((G, P, max(cap, 1)), dtype=np.uint64)
    for (g, s), e in win.items():
        if e:
            count[s, g] = len(e)
            entries[g, s, :len(e)] = e
    return count, entries


def first_window_diff(win, st, cap, got_count, got_entries):
    """(group, slot, wanted, got) of the first Replicate window that differs, or None; got_* as window_arrays gives them"""
    mask = replicate_mask(st)
    count, entries = window_arrays(win, st, cap)
    bad = (count != got_count) & mask
    live = np.arange(max(cap, 1))[None, None, :] < count.T[:, :, None]  # [G][P][cap]
    bad |= ((entries != got_entries) & live).any(axis=2).T & mask
    where = np.argwhere(bad)
    if not len(where):
        return None
    s, g = (int(v) for v in where[0])
    return g, s, entries[g, s, :count[s, g]].tolist(), got_entries[g, s, :got_count[s, g]].tolist()


def gate_step(st, cells, flags, terms):
    """term_gate_model.gate of every group over the SoA dict and the clock cells, both updated in place -> (filtered rows u8 [G][8],
    events, new_term or None per group, the three counts)"""
    G, P, cfg, cur = st["n_groups"], st["n_slots"], st["cfg"], st["cur_term"]
    rows, events, new_terms, counts = flags.copy(), [], [], [0, 0, 0]
    fl, tl = flags.tolist(), terms[:, :G].T.tolist()
    for g in range(G):
        c = cells[g]
        d = {"tag": c["tag"], "hb": c["hb"], "el": c["el"], "led": c["led"], "cur_term": int(cur[g]), "cfg": int(cfg[g])}
        row, ev, nt, stale, not_led = T.gate(d, fl[g], tl[g] + [0] * (8 - P), P)
        rows[g] = row
        events.append(ev)
        new_terms.append(nt)
        counts[0] += bool(ev & T.EV_DEPOSED)
        counts[1] += stale
        counts[2] += not_led
        c.update(tag=d["tag"], hb=d["hb"], el=d["el"], led=d["led"])
        cfg[g] = d["cfg"]
    return rows, events, new_terms, tuple(counts)


def clock_step(st, cells):
    """lead_clock_model.tick of every group over the SoA dict and the clock cells, both updated in place -> (events, {group:
    heartbeat commits} of the groups that beat, the four counts)"""
    G, P = st["n_groups"], st["n_slots"]
    cfg, cur, commit = st["cfg"], st["cur_term"], st["commit"]
    pf, match = st["pflags"].tolist(), st["match"][:P, :G].T.tolist()
    events, hb = [], {}
    for g in range(G):
        c = cells[g]
        d = {"tag": c["tag"], "hb": c["hb"], "el": c["el"], "led": c["led"], "cur_term": int(cur[g]), "cfg": int(cfg[g]), "pflags": pf[g], "match": match[g],
             "commit": int(commit[g])}
        ev = L.tick(CLOCK, d)
        events.append(ev)
        if ev & L.EV_BEAT:
            hb[g] = L.heartbeat_commits(d, P)
        c.update(tag=d["tag"], hb=d["hb"], el=d["el"], led=d["led"])
        cfg[g] = d["cfg"]
        st["pflags"][g, :] = d["pflags"]
    counts = tuple(sum(1 for e in events if e & b) for b in (L.EV_BEAT, L.EV_CHECK_QUORUM, L.EV_STEPPED_DOWN, L.EV_TRANSFER_ABORTED))
    return events, hb, counts


class Coverage:
    """What one sequence reached, on the model alone"""

    def __init__(self):
        self.ops = {k: 0 for k in OP_NAMES}
        self.transfer_status, self.conf_status, self.bad = set(), set(), {}
        self.n = {k: 0 for k in ("timeout_now_behind_transfer", "aborted_clock", "aborted_gate", "aborted_conf", "stepped_down", "deposed", "new_term_reelected",
                                 "restore_undoes_conf", "workgroup_selected", "workgroup_every_wave_owes", "lane_owes_all_peers", "max_lanes_owing", "cap_short_one",
                                 "cap_inside_second", "cap_zero", "cap_exact", "items", "stale_records", "not_led_records", "beats", "elected", "full_workgroup_conf",
                                 "full_workgroup_transfer", "wave_owes_all_peers")}

    def line(self):
        return "ops %s transfer %s conf %s bad %s %s" % (self.ops, sorted(self.transfer_status), sorted(self.conf_status), self.bad, self.n)


def check_floors(cov, cap):
    """The floors of a sequence: conditions on the model alone, for every committed seed. A whole workgroup owes items: in one conf
    call and in one transfer call all 256 lanes of a workgroup owe at least one item, and in one call every lane of a wave owes
    all P - 1."""
    low = {k: v for k, v in cov.ops.items() if v < 2}
    assert not low, ("every op kind runs at least twice in both of its forms", low)
    assert cov.transfer_status >= TRANSFER_STATUSES, sorted(TRANSFER_STATUSES - cov.transfer_status)
    assert cov.conf_status >= CONF_STATUSES, sorted(CONF_STATUSES - cov.conf_status)
    once = ["timeout_now_behind_transfer", "aborted_clock", "aborted_gate", "aborted_conf", "stepped_down", "deposed", "new_term_reelected", "restore_undoes_conf",
            "workgroup_selected"]
    if cap:
        once += ["workgroup_every_wave_owes", "full_workgroup_conf", "full_workgroup_transfer", "wave_owes_all_peers", "cap_short_one", "cap_inside_second"]
    missing = [k for k in once if cov.n[k] < 1]
    assert not missing, missing
    assert not cap or cov.n["items"] >= 3000, cov.n["items"]
    assert not cap or cov.n["max_lanes_owing"] == BLOCK, cov.n["max_lanes_owing"]
    assert sum(cov.bad.values()) >= 2, ("at least two forbidden calls are tried", cov.bad)


class Truth:
    def __init__(self, seed, P, cap, G=G_DEFAULT):
        self.seed, self.P, self.cap, self.G = seed, P, cap, G
        self.st = initial_state(np.random.default_rng(7100 + seed), G, P, cap)
        self.stride = self.st["stride"]
        self.win = {} if cap else None
        self.cells = [{"tag": TERM, "hb": 0, "el": 0, "led": True} for _ in range(G)]  # (what the enable call leaves, START_LED)
        self.ckpt = None
        self.cov = Coverage()
        self.conf_since_ckpt = False
        self.transferred, self.reelected = set(), set()  # groups a transfer op started a transfer in / a reelect op elected

    # ---- the pieces ----
    def oracle(self):
        """a fresh cluster that holds the truth's state, windows included"""
        cl = O.Cluster(self.G)
        cl.load_soa(self.st, term=TERM, max_inflight=self.cap)
        if self.cap:
            cl.set_own_inflights(True)
            add_windows(cl, self.win, self.st)
        return cl

    def take(self, cl):
        cl.store_soa(self.st)
        self.st["run_count"] = run_count_of(self.st)
        if self.cap:
            export_windows(cl, self.win, self.st, self.cap)

    def led(self, g):
        c = self.cells[g]
        return c["tag"] != int(self.st["cur_term"][g]) or c["led"]

    def stopped_groups(self):
        """the groups a re-election can elect: stopped under the current term, with a Progress of their own"""
        cfg, cur = self.st["cfg"], self.st["cur_term"]
        return [g for g in range(self.G) if not self.led(g) and int(cfg[g]) >> 24 >> (int(cfg[g]) >> 16 & 7) & 1 and int(cur[g]) < TERM + 200]

    def forget_transfers(self):
        cfg = self.st["cfg"]
        self.transferred = {g for g in self.transferred if int(cfg[g]) >> 20 & 0xF}

    def gate(self, flags, terms):
        rows, events, new_terms, counts = gate_step(self.st, self.cells, flags, terms)
        self.cov.n["deposed"] += counts[0]
        self.cov.n["aborted_gate"] += sum(1 for ev in events if ev & T.EV_DEPOSED and ev & T.EV_TRANSFER_ABORTED)
        self.cov.n["stale_records"] += counts[1]
        self.cov.n["not_led_records"] += counts[2]
        return rows, events, new_terms, counts

    # ---- the ops ----
    def apply(self, op):
        self.cov.ops[op["name"]] += 1
        if op.get("bad"):
            self.cov.bad[op["bad"]["call"]] = self.cov.bad.get(op["bad"]["call"], 0) + 1
        want = getattr(self, "_" + op["kind"])(op)
        self.forget_transfers()
        return want

    def _tick(self, op):
        msgs, want = dict(op["msgs"]), {"gate": None}
        if op["terms"] is not None:
            rows, events, new_terms, counts = self.gate(msgs["m_flags"], op["terms"])
            msgs["m_flags"] = rows
            want["gate"] = {"rows": rows, "events": events, "new_term": new_terms, "counts": counts}
        cl = self.oracle()
        gout = np.zeros(self.G, dtype=np.uint32)
        cl.tick_soa(msgs, gout)
        sent = cl.send_stage_soa(gout, op["max_entries"], skip_bcast_commit=op["skip"]) if self.cap else ()
        self.take(cl)
        self.st["out"][:] = gout
        want["out"], want["items"] = gout, coalesce(sent)
        self.cov.n["items"] += len(want["items"])
        self.cov.n["timeout_now_behind_transfer"] += sum(1 for g in self.transferred if int(gout[g]) & OUT_TIMEOUT_NOW)
        elected = [g for g in op["elected"] if int(gout[g]) & 0x10]
        self.cov.n["elected"] += len(elected)
        self.reelected |= set(elected)
        return want

    def _clock(self, op):
        events, hb, counts = clock_step(self.st, self.cells)
        for g in [g for g in self.reelected if events[g] & L.EV_NEW_TERM]:
            self.cov.n["new_term_reelected"] += 1
            self.reelected.discard(g)
        self.cov.n["beats"] += counts[0]
        self.cov.n["stepped_down"] += counts[2]
        self.cov.n["aborted_clock"] += counts[3]
        return {"events": events, "hb": hb, "counts": counts}

    def _items_of_call(self, op, items):
        """item_cap of the call from its draw, and what the call's density reached"""
        n, total = self.cov.n, len(items)
        per_group = {}
        for g, s in items:
            per_group[g] = per_group.get(g, 0) + 1
        n0, n1 = sum(v for g, v in per_group.items() if g < BLOCK), sum(v for g, v in per_group.items() if BLOCK <= g < 2 * BLOCK)
        op["item_cap"] = {"exact": total, "short1": max(total - 1, 0), "mid2": n0 + n1 // 2, "zero": 0}[op["cap_mode"]]
        n["items"] += total
        n["cap_exact"] += op["cap_mode"] == "exact"
        n["cap_zero"] += op["cap_mode"] == "zero" and total > 0
        n["cap_short_one"] += op["cap_mode"] == "short1" and total > 0
        n["cap_inside_second"] += op["cap_mode"] == "mid2" and n1 >= 2 and n0 < op["item_cap"] < n0 + n1
        if op["density"] == "workgroups":
            n["workgroup_selected"] += 1
            waves = {g // 64 for g in per_group if g < 2 * BLOCK}
            n["workgroup_every_wave_owes"] += len(waves) == 2 * BLOCK // 64
            n["max_lanes_owing"] = max(n["max_lanes_owing"], sum(1 for g in per_group if g < BLOCK), sum(1 for g in per_group if BLOCK <= g < 2 * BLOCK))
        n["lane_owes_all_peers"] += any(v == self.P - 1 for v in per_group.values())
        full = any(all(g in per_group for g in range(b, b + BLOCK)) for b in (0, BLOCK))
        n["full_workgroup_" + op["kind"]] += full
        n["wave_owes_all_peers"] += any(all(per_group.get(g) == self.P - 1 for g in range(w, w + 64)) for w in range(0, 2 * BLOCK, 64))

    def _conf(self, op):
        led = {g: self.led(g) for g, _ in op["recs"]}
        self.st, answers, items = CM.apply_state(self.st, self.win, op["recs"], self.cap, led=led, max_entries=op["max_entries"])
        items = {k: (v[0], v[1] & U64, v[2] & U64, v[3]) for k, v in items.items()}
        self._items_of_call(op, items)
        self.cov.conf_status |= {a["status"] for a in answers}
        self.cov.n["aborted_conf"] += sum(1 for a in answers if a["events"] & CM.EV_TRANSFER_ABORTED)
        self.conf_since_ckpt |= any(a["status"] in (CM.DONE, CM.DEMOTED) for a in answers)
        return {"answers": answers, "items": items, "total": len(items)}

    def _transfer(self, op):
        led = {g: self.led(g) for g, _ in op["recs"]}
        cells = {g: self.cells[g] for g, _ in op["recs"]}
        self.st, answers, items = TM.apply_state(self.st, self.win, op["recs"], self.cap, led=led, cells=cells, max_entries=op["max_entries"])
        items = {k: (v[0], v[1] & U64, v[2] & U64, v[3]) for k, v in items.items()}
        self._items_of_call(op, items)
        self.cov.transfer_status |= {a["status"] for a in answers}
        self.transferred |= {g for (g, _), a in zip(op["recs"], answers) if a["status"] == TM.STARTED}
        return {"answers": answers, "items": items, "total": len(items)}

    def _events(self, op):
        cl = self.oracle()
        apply_events(cl, op["events"], self.G, self.P)
        self.take(cl)
        return {}

    def _checkpoint(self, op):
        self.ckpt = (R.copy_state(self.st), copy_windows(self.win), copy_cells(self.cells), set(self.transferred), set(self.reelected))
        self.conf_since_ckpt = False
        return {}

    def _restore(self, op):
        st, win, cells, transferred, reelected = self.ckpt
        self.st, self.win, self.cells, self.transferred, self.reelected = R.copy_state(st), copy_windows(win), copy_cells(cells), set(transferred), set(reelected)
        self.cov.n["restore_undoes_conf"] += self.conf_since_ckpt
        self.conf_since_ckpt = False
        return {}


def apply_events(cl, events, G, P):
    """RawNode::report_unreachable / report_snapshot as tests/test_api_sequences_gpu.py local_messages hands them to the oracle"""
    for g, s, kind in events:
        if g >= G or s >= P:
            continue
        if kind == 1:
            cl.L.ro_handle_unreachable(cl.h, g, s + 1)
        else:
            cl.L.ro_handle_snapshot_status(cl.h, g, s + 1, kind == 3)


class Chooser:
    """The next op from the truth's state alone. A shuffled deck holds every op kind in both of its forms often enough; an op whose
    precondition the state does not meet yet waits for a later step. twin: only inputs BOTH forms of a call take (no malformed word,
    no slot at or beyond P), for the test that runs the dense and the sparse forms side by side."""

    def __init__(self, seed, P, cap, G=G_DEFAULT, twin=False, tick_runs=False):
        """tick_runs: every plain tick of the deck is followed by 1-3 more plain ticks (op["follows"] on them), and every ungated
        tick carries op["columns_only"]: whoever runs beside the truth reads nothing but columns behind it, so the next op -- a
        tick of the run, or whatever call the deck holds next -- finds the engine as the tick left it. The default draws exactly
        what it always drew."""
        self.rng = np.random.default_rng(9100 + seed)
        self.P, self.cap, self.G, self.twin = P, cap, G, twin
        self.tick_runs, self.run_left = tick_runs, 0
        self.deck = [DECK[i] for i in self.rng.permutation(len(DECK))]
        # the first two steps, while every group is still led, over workgroups 0 and 1 as shape_workgroups prepared them: a dense
        # transfer in which every lane of workgroup 1 owes its item (workgroup 0 names its own leader: SELF, nothing moves), then a
        # dense conf change in which every lane of workgroup 0 owes items and every lane of its wave 0 all P - 1 of them
        for k, name in enumerate(("transfer_dense", "conf_dense")):
            self.deck.remove(name)
            self.deck.insert(k, name)
        self.step = 0
        self.bad_order = [c for c in sorted(BAD_CALLS) if not c.endswith("owed")]
        self.bad_order = self.bad_order[4 * seed % len(self.bad_order):] + self.bad_order[:4 * seed % len(self.bad_order)]

    def ready(self, name, tr):
        if name == "restore":
            return tr.ckpt is not None and tr.conf_since_ckpt
        if name == "reelect":
            return "clock" in self.deck and len(tr.stopped_groups()) > 0
        return True

    def done(self):
        return not self.deck and not self.run_left

    def next(self, tr):
        if self.run_left:  # (tick_runs: the rest of a run of plain ticks)
            self.run_left -= 1
            op = self._tick(tr, "tick_one" if self.rng.random() < 0.5 else "tick_two")
            op.update(name="tick_one" if op["launches"] == 1 else "tick_two", bad=None, follows=True, columns_only=True)
            self.step += 1
            return op
        name = next((n for n in self.deck if self.ready(n, tr)), None)
        if name is None:  # (nothing is ready: the first op in the form the state allows)
            name = self.deck[0]
            self.deck.pop(0)
            kind = {"restore": "restore" if tr.ckpt is not None else "checkpoint", "reelect": "reelect"}[name]
        else:
            self.deck.remove(name)
            kind = name
        op = getattr(self, "_" + kind.split("_")[0])(tr, kind)
        if name == "restore" and op["kind"] == "checkpoint":  # (counted as what ran)
            name = "checkpoint"
        if name == "reelect" and not op["elected"]:
            name = "tick_one" if op["launches"] == 1 else "tick_two"
        op["name"] = name
        op["bad"] = self.bad_call(tr, op)
        if self.tick_runs and op["kind"] == "tick" and op["terms"] is None:
            self.run_left = int(self.rng.integers(1, 4))
            op["columns_only"] = True
        self.step += 1
        return op

    # ---- ticks ----
    def msgs(self, tr):
        m = O.alloc_msgs(self.G, self.P)
        del m["m_logterm"]
        fuzz.random_msgs(self.rng, tr.st, m, sent_p=0.0 if self.cap else 0.5, heartbeat_p=0.2)
        if self.cap:
            sendstage.prepare_msgs(m)
        return m

    def _tick(self, tr, kind, terms=None, msgs=None, elected=()):
        return {"kind": "tick", "launches": 1 if kind.endswith("one") else 2, "msgs": msgs or self.msgs(tr), "terms": terms, "max_entries": int(self.rng.integers(0, 4)),
                "skip": bool(self.rng.integers(0, 2)), "elected": list(elected)}

    def _gated(self, tr, kind):
        """a m_term column around RG_COL_CUR_TERM: 0, equal, lower, and for about 3 % of the groups higher; the own slot's events
        carry 0 by contract (include/raftgroups_term.h)"""
        rng, G, P = self.rng, self.G, self.P
        msgs = self.msgs(tr)
        cur = tr.st["cur_term"]
        self_slot = (tr.st["cfg"] >> 16 & 7).astype(np.int64)
        terms = np.full((P, tr.stride), 0xDEAD, dtype=np.uint64)
        higher = rng.random(G) < 0.03
        for s in range(P):
            pick = rng.random(G)
            t = np.where(pick < 0.15, 0, np.where(pick < 0.85, cur, cur - 1)).astype(np.uint64)
            t = np.where(higher, cur + rng.integers(1, 4, size=G).astype(np.uint64), t)
            terms[s, :G] = np.where(self_slot == s, 0, t)
        return self._tick(tr, kind, terms=terms, msgs=msgs)

    def _reelect(self, tr, kind):
        """RG_MF_BECOME_LEADER alone on the own slot of about half of the stopped groups, m_hint = RG_COL_CUR_TERM + 1"""
        rng = self.rng
        msgs = self.msgs(tr)
        stopped = tr.stopped_groups()
        elected = [g for g in stopped if rng.random() < 0.5] or stopped[:1]
        for g in elected:
            s = int(tr.st["cfg"][g]) >> 16 & 7
            msgs["m_flags"][g, :] = 0
            msgs["m_flags"][g, s] = MF_BECOME_LEADER
            msgs["m_hint"][s, g] = int(tr.st["cur_term"][g]) + 1
        return self._tick(tr, "reelect_one" if rng.random() < 0.5 else "reelect_two", msgs=msgs, elected=elected)

    def _clock(self, tr, kind):
        r = self.rng.random()
        caps = (None, None) if r < 0.6 else (int(self.rng.integers(0, 4)), int(self.rng.integers(0, 4)))
        return {"kind": "clock", "beat_cap": caps[0], "down_cap": caps[1], "hb": bool(self.rng.random() < 0.8)}

    # ---- conf change and transfer ----
    def selection(self):
        rng, G = self.rng, self.G
        density = ("few", "forty", "workgroups")[int(rng.choice(3, p=[0.25, 0.3, 0.45]))]
        if self.step < 2:
            density = "workgroups"
        if density == "few":
            groups = np.sort(rng.choice(G, size=int(rng.integers(3, 25)), replace=False))
        elif density == "forty":
            groups = np.nonzero(rng.random(G) < 0.4)[0]
        else:  # every group of workgroups 0 and 1, none of workgroup 2: its lanes all leave at the first barrier
            groups = np.arange(2 * BLOCK)
        return density, [int(g) for g in groups]

    def word(self, old, dense):
        """a conf word as tests/test_conf_change_host.py sweep_cases draws it -- the present set kept in three cases of ten, the
        leader's own slot kept a voter with a Progress more often than chance would -- and in the dense form only, a malformed one"""
        rng, P = self.rng, self.P
        full = (1 << P) - 1
        oldp, self_slot = old >> 24 & 0xFF, old >> 16 & 7
        r = rng.random()
        bad_ok = dense and not self.twin
        if r < 0.08 and bad_ok:
            return int(rng.integers(0, 1 << 32))
        if 0.3 <= r < 0.42:  # the leader alone votes, everyone has a Progress: where its own matched index is ahead the commit index
            return CM.word(1 << self_slot & full or 1, 0, full)  # moves, and bcast_append owes every peer a message
        keep = (1 << self_slot) & full if rng.random() < 0.7 else 0
        Wp = oldp if r < 0.3 and oldp else int(rng.integers(1, full + 1)) | keep
        Wi = (int(rng.integers(1, full + 1)) | keep) & Wp or Wp & -Wp
        Wo = int(rng.integers(0, full + 1)) & Wp if rng.random() < 0.4 else 0
        W = CM.word(Wi, Wo, Wp)
        if r > 0.97 and bad_ok:
            W |= 1 << int(rng.integers(8, 16)) if P < 8 else 1 << 17
        return W

    def cap_mode(self):
        return ("exact", "short1", "mid2", "zero")[int(self.rng.choice(4, p=[0.3, 0.3, 0.3, 0.1]))] if self.cap else "exact"

    def _conf(self, tr, kind):
        dense = kind.endswith("dense")
        density, groups = self.selection()
        recs = [(g, self.word(int(tr.st["cfg"][g]), dense)) for g in groups]
        if self.step == 1:  # workgroup 0: the leader alone votes, everyone has a Progress
            recs = [(g, CM.word(1 << (int(tr.st["cfg"][g]) >> 16 & 7), 0, (1 << self.P) - 1) if g < BLOCK else W) for g, W in recs]
        return {"kind": "conf", "dense": dense, "recs": recs, "density": density, "cap_mode": self.cap_mode(), "max_entries": int(self.rng.integers(0, 4))}

    def owed_peers(self, tr, g):
        """the voters of a group, other than its leader and its transferee, that lag and are not paused"""
        st, P = tr.st, self.P
        cfg, hi = int(st["cfg"][g]), int(st["term_hi"][g])
        out = []
        for s in range(P):
            pb = int(st["pflags"][g, s])
            if not cfg >> 24 >> s & 1 or not (cfg | cfg >> 8) >> s & 1 or s == cfg >> 16 & 7 or s + 1 == cfg >> 20 & 0xF or int(st["match"][s, g]) == hi:
                continue
            if (pb & 3 == O.PROBE and not pb & CM.PF_PAUSED) or (pb & 3 == O.REPLICATE and self.cap and len(tr.win.get((g, s), ())) < self.cap):
                out.append(s)
        return out

    def _transfer(self, tr, kind):
        rng, P = self.rng, self.P
        dense = kind.endswith("dense")
        density, groups = self.selection()
        wide = dense and not self.twin
        recs = [(g, 254 if wide and rng.random() < 0.02 else int(rng.integers(0, P + 1 if wide else P))) for g in groups]
        for k, (g, _) in enumerate(recs):  # six times in ten, where there is one: a peer the call owes a message
            owed = self.owed_peers(tr, g) if rng.random() < 0.6 else ()
            if len(owed):
                recs[k] = (g, owed[int(rng.integers(0, len(owed)))])
            if self.step == 0:  # workgroup 0: the leader itself; workgroup 1: the slot behind the leader's
                me = int(tr.st["cfg"][g]) >> 16 & 7
                recs[k] = (g, me if g < BLOCK else (me + 1) % P)
        return {"kind": "transfer", "dense": dense, "recs": recs, "density": density, "cap_mode": self.cap_mode(), "max_entries": int(self.rng.integers(0, 4))}

    # ---- the rest ----
    def _events(self, tr, kind):
        rng, G, P = self.rng, self.G, self.P
        if kind.endswith("records"):
            return {"kind": "events", "form": "records", "events": fuzz.random_progress_events(rng, G, P, int(rng.integers(1, 60)))}
        ev_kind = int(rng.integers(1, 4))
        slot1 = np.where(rng.random(G) < 0.1, rng.integers(1, P + 1, size=G), 0).astype(np.uint8)
        return {"kind": "events", "form": "dense", "ev_kind": ev_kind, "slot1": slot1, "events": [(int(g), int(slot1[g]) - 1, ev_kind) for g in np.nonzero(slot1)[0]]}

    def _checkpoint(self, tr, kind):
        return {"kind": "checkpoint"}

    def _restore(self, tr, kind):
        return {"kind": "restore"}

    def bad_call(self, tr, op):
        """About one step in fifteen: a call the state forbids, tried BEFORE the step's own call -- or, inside a two-launch tick of an
        engine with device Inflights, between the tick and its send stage, which is then owed"""
        rng = self.rng
        r = rng.random()
        if op["kind"] == "tick" and op["launches"] == 2 and self.cap and r < 0.3:
            return {"call": ("conf_owed", "transfer_owed")[int(rng.integers(0, 2))], "when": "owed", "group": int(rng.integers(0, self.G))}
        if r >= 1 / 15:
            return None
        self.bad_order.append(self.bad_order.pop(0))  # (in turn, from a start the seed sets: no call is drawn twice before all were)
        return {"call": self.bad_order[-1], "when": "before", "group": int(rng.integers(0, self.G))}


def mirror_classes(op, first=False):
    """What one step of tests/test_lead_sequences_gpu.py's Runner does to the dense tick's read mirror, as call classes of
    readmirror.after, in order: the load and the first check drop it; a forbidden call is tried between two reads of the whole
    engine (rg_read_groups: drop); a gated tick enters through rgt_lead_gate_device first; every other op but the tick drops;
    the check behind a step reads the clock cells (drop) unless the op says columns only (an ungated tick under tick_runs: keep)."""
    classes = ["drop"] if first else []
    if op["bad"]:
        classes.append("drop")
    if op["kind"] == "tick":
        if op["terms"] is not None:
            classes.append("drop")
        classes.append("tick")
    else:
        classes.append("drop")
    classes.append("keep" if op.get("columns_only") else "drop")
    return classes


def sequence(seed, P, cap, G=G_DEFAULT, twin=False, steps=STEPS):
    """(step, op, want, truth) of a whole sequence, the truth moved by the models alone; what runs beside it runs inside the loop body
    of the caller, AFTER the truth has moved (the op then carries the call's item_cap)"""
    tr, ch = Truth(seed, P, cap, G), Chooser(seed, P, cap, G, twin)
    for step in range(steps):
        op = ch.next(tr)
        yield step, op, tr.apply(op), tr
