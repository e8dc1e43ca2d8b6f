"""GPU: the wire-record path (rg_ingest / rg_ingest_device -> rg_tick_ingested, and rg_ingest_tick) at its kernel and road
edges, bit-exact against the oracle (O.Cluster.tick_soa on the same events): record counts around one workgroup and around
every threshold of rg_ingest_tick's road selection, duplicates at scale with exact accounting (identical copies, and two
DIFFERENT records racing for a cell, judged by tests/ingestcheck.py), the list append under contention, malformed records,
touched fractions up to every cell of every group, cells reused across windows, what may happen between rg_ingest and
rg_tick_ingested, rg_ingested_results with short arrays, and the contract of the duplicate counts.

Which road a size takes follows from the constants in tests/ingestcheck.py (tests/test_ingestcheck.py ties them to the kernels'
headers), never from observation. The resident mailbox is not started anywhere in this file."""
import numpy as np
import pytest

import fuzz
import ingestcheck as IC
import oracle_lib as O

pytestmark = pytest.mark.gpu
TERM = 6
MF_VALID, MF_REJECT, MF_HAS_RS, MF_HAS_LOGTERM = fuzz.MF_VALID, fuzz.MF_REJECT, fuzz.MF_HAS_RS, 0x80

_BASE = {}


def copy_state(st):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}


def base_state(G, P, seed, gc=False):
    """A random cfg column and state (with a term-run table; with group commit: gids and the flag in 60 % of the cfg words, no
    table -- as test_group_commit_streams_match_oracle has it). Built once per shape, handed out as copies."""
    key = (G, P, seed, gc)
    if key not in _BASE:
        rng = np.random.default_rng(seed)
        st = O.alloc_state(G, P) if gc else O.add_term_table(O.alloc_state(G, P))
        st["cfg"][:] = fuzz.random_cfg(rng, G, P, group_commit_frac=0.6 if gc else 0.0)
        fuzz.random_state(rng, st, small_values=True, with_gids=gc)
        if not gc:
            fuzz.random_term_table(rng, st, TERM)
        _BASE[key] = st
    return copy_state(_BASE[key])


class Harness:
    """Engines and the oracle on one state; every window: new_msgs() -> (cut the events down) -> feed the engines ->
    oracle_tick() -> check(eng) / check_results(eng)."""

    def __init__(self, rg, G, P, seed, n_engines=2, gc=False, st=None):
        from raft_rs_amd.engine import WIRE_DTYPE
        assert WIRE_DTYPE == IC.WIRE_DTYPE
        self.rg, self.G, self.P, self.gc = rg, G, P, gc
        self.rng = np.random.default_rng(seed + 1)
        self.st = st if st is not None else base_state(G, P, seed, gc)
        self.engs = [rg.Engine(G, P) for _ in range(n_engines)]
        for e in self.engs:
            e.load_state(self.st)
        self.cl = self.cluster(self.st)
        self.msgs = O.alloc_msgs(G, P)
        self.gout = np.zeros(G, dtype=np.uint32)

    def cluster(self, st):
        cl = O.Cluster(self.G)
        cl.load_soa(st, term=TERM)
        return cl

    def new_msgs(self, groups=None, msgs=None):
        """Random events against the oracle's current state (log-term rejects included when there is a term table)."""
        msgs = self.msgs if msgs is None else msgs
        self.cl.store_soa(self.st)
        fuzz.random_msgs(self.rng, self.st, msgs, logterm_max=0 if self.gc else TERM)
        if groups is not None:
            IC.keep_groups(msgs, groups)
        return msgs

    def oracle_tick(self, msgs=None):
        self.gout[:] = 0
        self.cl.tick_soa(self.msgs if msgs is None else msgs, self.gout)
        self.cl.store_soa(self.st)

    def check(self, eng, what):
        got = eng.read_state()
        diffs = fuzz.diff_states(self.st, got, self.G, self.P)
        assert not diffs, (what, diffs[:5])
        bad = np.nonzero(got["out"] != self.gout)[0]
        assert bad.size == 0, (what, "RG_COL_OUT", bad[:5], got["out"][bad[:5]], self.gout[bad[:5]])

    def check_results(self, eng, what, msgs=None):
        """The result triples, sorted by group: the groups with events, each ONCE, with the oracle's commit and result word."""
        msgs = self.msgs if msgs is None else msgs
        with_events = np.nonzero(msgs["m_flags"].any(axis=1))[0]
        groups, commit, out = eng.ingested_results()
        order = np.argsort(groups, kind="stable")
        assert len(groups) == len(with_events), (what, len(groups), len(with_events))
        assert (groups[order] == with_events).all(), what
        assert (commit[order] == self.st["commit"][with_events]).all(), what
        assert (out[order] == self.gout[with_events]).all(), what
        return len(with_events)

    def close(self):
        for e in self.engs:
            e.close()


def split_odd(n):
    """An odd split point of a batch of n records (n itself for a batch of one)."""
    return min(n, (n // 2) | 1)


def to_device(recs):
    import torch
    return torch.from_numpy(recs.view(np.uint8).copy()).cuda()


def feed_both(h, recs, n_groups, what, drops=0):
    """The same window on engine 0 with rg_ingest_tick and on engine 1 with rg_ingest split at an odd boundary +
    rg_tick_ingested; then the oracle; states, result triples, group counts and drops of both."""
    a, b = h.engs
    assert a.ingest_tick(recs) == (n_groups, drops), what
    k = split_odd(len(recs))
    got = b.ingest(recs[:k]) + (b.ingest(recs[k:]) if k < len(recs) else 0)
    assert got == drops, what
    assert b.tick_ingested() == n_groups, what
    h.oracle_tick()
    for name, e in (("rg_ingest_tick", a), ("rg_ingest + rg_tick_ingested", b)):
        h.check(e, (what, name))
        assert h.check_results(e, (what, name)) == n_groups


# ---- 2. record-count and road edges ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True])
def test_record_count_edges_on_every_road(rg, reverse):
    """Batches of EXACTLY 1, 255, 256, 257, 511, 512, 513, 1024, 1025, 4096, 4097, 16384, 16385 and 3 G records: one launch,
    zero-copy with several workgroups, the round trip through device staging, the three-call road. In an order that makes
    the record staging (device and pinned) and the packed result buffers grow in the middle of the run, and backwards."""
    G, P = 8192, 5
    counts = [1, 257, 16385, 255, 4097, 3 * G, 256, 511, 1025, 16384, 512, 4096, 513, 1024]  # small, huge, small, ...
    assert sorted(counts) == IC.edge_counts(G)
    h = Harness(rg, G, P, seed=1201)
    for n in counts[::-1] if reverse else counts:
        msgs = h.new_msgs()
        touched = IC.fit_record_count(msgs, h.rng.permutation(G), n, P)
        recs = IC.records(msgs, touched, P, rng=h.rng)
        assert len(recs) == n
        feed_both(h, recs, len(touched), f"{n} records")
    h.close()


def test_zero_copy_road_with_many_workgroups_and_a_device_side_window(rg):
    """G = 1000: the window never exceeds RG_ZEROCOPY_MAX, so 300, 2000 and 8000 records (every cell of every group) all take
    the zero-copy road, where a k_ingest of up to 32 workgroups also zeroes the previous sparse tick's result words -- each
    batch follows a sparse tick of another touched set. Then rg_ingest_tick with 200 records closes a window in which
    rg_ingest_device has already listed 600 groups: the one-launch kernel ticks more groups than it has lanes."""
    G, P = 1000, 8
    assert G <= IC.RG_ZEROCOPY_MAX and G * P <= IC.RG_ROUNDTRIP_MAX
    h = Harness(rg, G, P, seed=1202)
    for n in (300, 2000, 8000):
        assert n > IC.RG_INGEST_BLOCK
        before = np.sort(h.rng.choice(G, size=150, replace=False))
        msgs = h.new_msgs(before)
        feed_both(h, IC.records(msgs, before, P, rng=h.rng), int(msgs["m_flags"].any(axis=1).sum()), f"before {n}")
        assert np.count_nonzero(h.gout), "the preceding tick left no result word to zero"
        msgs = h.new_msgs()
        touched = IC.fit_record_count(msgs, h.rng.permutation(G), n, P)
        feed_both(h, IC.records(msgs, touched, P, rng=h.rng), len(touched), f"{n} records")
        untouched = np.ones(G, dtype=bool)
        untouched[touched] = False
        for e in h.engs:
            assert not e.read_column(rg.COL.OUT)[untouched].any(), f"{n} records: stale result words outside the touched set"
    a, b = h.engs
    msgs = h.new_msgs()
    perm = h.rng.permutation(G)
    first, rest = perm[:600], perm[600:]
    small = copy_state(msgs)
    IC.keep_groups(msgs, first)
    dev_recs = IC.records(msgs, first, P, rng=h.rng)
    listed = int(msgs["m_flags"].any(axis=1).sum())
    assert listed > 2 * IC.RG_INGEST_BLOCK
    host_groups = IC.fit_record_count(small, rest, 200, P)
    host_recs = IC.records(small, host_groups, P, rng=h.rng)
    assert len(host_recs) == 200 <= IC.RG_INGEST_BLOCK
    dev = to_device(dev_recs)
    for e in (a, b):
        e.ingest_device(dev.data_ptr(), len(dev_recs))
    assert a.ingest_tick(host_recs) == (listed + len(host_groups), 0)
    assert b.ingest(host_recs) == 0 and b.tick_ingested() == listed + len(host_groups)
    a.sync(), b.sync()
    del dev
    msgs["m_flags"][host_groups] = small["m_flags"][host_groups]
    for k in ("m_index", "m_commit", "m_hint", "m_rs", "m_logterm"):
        msgs[k][:, host_groups] = small[k][:, host_groups]
    h.oracle_tick()
    for e in (a, b):
        h.check(e, "device-side window")
        h.check_results(e, "device-side window")
    h.close()


# ---- 3. duplicates at scale, exact accounting --------------------------------------------------------------------------------
def with_copies(recs):
    """Every record 1 + (group mod 4) times. The second copy follows its original directly (the same workgroup, mostly the same
    wave); third and fourth copies come behind ALL first and second ones, the groups that have them first in the array, so
    that they are at least RG_INGEST_BLOCK records away from their original. Returns (records, is_copy)."""
    k = 1 + recs["group"] % 4
    first = np.concatenate([recs[k >= 3], recs[k < 3]])
    kf = 1 + first["group"] % 4
    rep = np.where(kf >= 2, 2, 1)
    sec = np.repeat(first, rep)
    is_copy = np.ones(len(sec), dtype=bool)
    is_copy[np.cumsum(rep) - rep] = False
    third, fourth = first[kf >= 3], first[kf == 4]
    near = int(rep[kf < 3].sum())
    assert near >= IC.RG_INGEST_BLOCK and len(third) and len(fourth), "no room between an original and its far copies"
    pos = np.nonzero(is_copy)[0]
    assert ((pos // IC.RG_INGEST_BLOCK) == ((pos - 1) // IC.RG_INGEST_BLOCK)).any(), "no copy shares a workgroup with its original"
    out = np.concatenate([sec, third, fourth])
    return out, np.concatenate([is_copy, np.ones(len(third) + len(fourth), dtype=bool)])


@pytest.mark.parametrize("P", [8, 3])
def test_exact_copies_are_dropped_and_counted_exactly(rg, P):
    """1500 touched groups, every record 1 + (g mod 4) times: drops == records - distinct cells, the state is the oracle's with
    one event per cell, every group is listed once. In one call; with the copies in a second rg_ingest; with the copies, or
    the originals, or everything, coming through rg_ingest_device -- rg_ingest counts its OWN call's drops,
    rg_ingested_duplicates and rg_ingest_tick those of the window."""
    G = 4096
    h = Harness(rg, G, P, seed=1300 + P)
    a, b = h.engs
    empty = np.zeros(0, dtype=IC.WIRE_DTYPE)
    for window in range(3):
        touched = np.sort(h.rng.choice(G, size=1500, replace=False))
        msgs = h.new_msgs(touched)
        recs = IC.records(msgs, touched, P, rng=h.rng)
        allrecs, is_copy = with_copies(recs)
        orig, copies = allrecs[~is_copy], allrecs[is_copy]
        drops = len(allrecs) - len(recs)
        assert len(orig) == len(recs) and drops == len(copies) > len(recs) // 2
        n_groups = int(msgs["m_flags"].any(axis=1).sum())
        if window == 0:    # everything in one call
            assert a.ingest_tick(allrecs) == (n_groups, drops)
            assert b.ingest(allrecs) == drops and b.ingested_duplicates() == drops
            assert b.tick_ingested() == n_groups
        elif window == 1:  # the copies in a second rg_ingest; the originals from device memory and the copies from the host
            assert a.ingest(orig) == 0 and a.ingested_duplicates() == 0
            assert a.ingest(copies) == drops and a.ingested_duplicates() == drops
            assert a.tick_ingested() == n_groups
            dev = to_device(orig)
            b.ingest_device(dev.data_ptr(), len(orig))
            assert b.ingest(copies) == drops and b.ingested_duplicates() == drops
            assert b.tick_ingested() == n_groups
            del dev
        else:              # the copies from device memory; everything from device memory, closed by an EMPTY rg_ingest_tick
            dev = to_device(copies)
            assert a.ingest(orig) == 0
            a.ingest_device(dev.data_ptr(), len(copies))
            a.sync()
            assert a.ingested_duplicates() == drops
            assert a.ingest(empty) == 0 and a.ingested_duplicates() == drops
            assert a.tick_ingested() == n_groups
            dev_all = to_device(allrecs)
            b.ingest_device(dev_all.data_ptr(), len(allrecs))
            assert b.ingest_tick(empty) == (n_groups, drops)
            del dev, dev_all
        for e in (a, b):
            assert e.ingested_duplicates() == 0, "the next window starts at zero"
        h.oracle_tick()
        for e in (a, b):
            h.check(e, (P, window))
            assert h.check_results(e, (P, window)) == n_groups
    h.close()


def probing_cells(st, rng, n, P):
    """n groups with a slot that is not the leader's own and has a Progress; that Progress is put into Probe, two entries behind
    the log's end. Returns (groups, slots)."""
    G = st["n_groups"]
    self_slot = ((st["cfg"] >> 16) & 7).astype(np.int64)
    present = (st["cfg"] >> 24) & 0xff
    slots = np.full(G, -1, dtype=np.int64)
    for p in range(P):
        ok = (((present >> p) & 1) == 1) & (self_slot != p) & (slots < 0)
        slots[ok] = p
    groups = np.sort(rng.choice(np.nonzero(slots >= 0)[0], size=n, replace=False))
    s = slots[groups]
    assert (st["term_hi"][groups] >= 5).all()
    m = st["term_hi"][groups] - 2
    st["match"][s, groups] = m
    st["next"][s, groups] = m + 1
    st["pr_commit"][s, groups] = np.minimum(st["commit"][groups], m)
    st["pend_snap"][s, groups] = 0
    st["pend_rs"][s, groups] = 0
    st["pflags"][groups, s] = 0  # Probe, not paused, not recently active
    return groups, s


def set_cells(msgs, st, groups, s, kind):
    """kind "accept": MsgAppendResponse at match + 1 with every other field zero. kind "reject": a reject of next - 1 with a
    hint, a third of them with request_snapshot, half with the follower's log term."""
    g = groups
    for k in ("m_hint", "m_rs", "m_logterm"):
        msgs[k][s, g] = 0
    if kind == "accept":
        idx = np.minimum(st["match"][s, g] + 1, st["term_hi"][g])
        msgs["m_index"][s, g] = idx
        msgs["m_commit"][s, g] = np.minimum(st["commit"][g], idx)
        msgs["m_flags"][g, s] = MF_VALID
    else:
        nx = st["next"][s, g]
        idx = np.where(nx > 0, nx - 1, 0).astype(np.uint64)
        has_rs, has_lt = g % 3 == 0, g % 2 == 0
        msgs["m_index"][s, g] = idx
        msgs["m_commit"][s, g] = 0
        msgs["m_hint"][s, g] = np.where(idx > 0, idx - 1, 0)
        msgs["m_rs"][s, g] = np.where(has_rs, 5 + g % 20, 0)
        msgs["m_logterm"][s, g] = np.where(has_lt, 1 + g % TERM, 0)
        msgs["m_flags"][g, s] = MF_VALID | MF_REJECT | has_rs * MF_HAS_RS | has_lt * MF_HAS_LOGTERM


@pytest.mark.parametrize("one_call", [True, False], ids=["rg_ingest_tick", "rg_ingest+rg_tick_ingested"])
@pytest.mark.parametrize("P", [8, 3])
def test_two_different_records_for_one_cell_one_wins_whole(rg, P, one_call):
    """One cell in each of 1000 groups gets an accept (A) AND a reject with hint / request_snapshot / log term (B) of a probing
    peer in the same window, half of the pairs inside one wave, half in different workgroups, either record first. Which one
    wins is not specified; every group must equal the oracle's "all A" or its "all B" on every column and its result word
    (ingestcheck.judge), exactly one record of each pair is counted as dropped, and the run goes on from the state the
    oracle reaches with the records the engine applied."""
    G = 4096
    st0 = base_state(G, P, seed=1310 + P)
    rng = np.random.default_rng(77 + P)
    pairs, s = probing_cells(st0, rng, 1000, P)
    h = Harness(rg, G, P, seed=1310 + P, n_engines=1, st=st0)
    eng = h.engs[0]
    others = np.setdiff1d(rng.choice(G, size=1500, replace=False), pairs)
    msgs_a = h.new_msgs(np.concatenate([pairs, others]))
    set_cells(msgs_a, h.st, pairs, s, "accept")
    msgs_b = copy_state(msgs_a)
    set_cells(msgs_b, h.st, pairs, s, "reject")
    # the oracle's two answers, and the condition on the inputs: they differ in EVERY judged group
    answers = []
    for m in (msgs_a, msgs_b):
        st, gout = copy_state(h.st), np.zeros(G, dtype=np.uint32)
        cl = h.cluster(st)
        cl.tick_soa(m, gout)
        cl.store_soa(st)
        st["out"] = gout
        answers.append(st)
    IC.assert_distinguishable(answers[0], answers[1], pairs, P)
    # wire order: [pairs inside a wave: X Y X Y ...] [first records of the other pairs] [everything else] [their second records]
    is_pair = np.zeros((G, 8), dtype=bool)
    is_pair[pairs, s] = True
    rec_a = IC.records(msgs_a, np.concatenate([pairs, others]), P, rng=rng)
    cell_a = is_pair[rec_a["group"].astype(np.int64), rec_a["slot"].astype(np.int64)]
    rest, rec_a = rec_a[~cell_a], rec_a[cell_a]
    rec_b = IC.records(msgs_b, pairs, P, order="slot_adjacent")
    rec_b = rec_b[is_pair[rec_b["group"].astype(np.int64), rec_b["slot"].astype(np.int64)]]
    rec_a = rec_a[np.argsort(rec_a["group"], kind="stable")]
    assert len(rec_a) == len(rec_b) == 1000 and (rec_a["group"] == rec_b["group"]).all() and (rec_a["slot"] == rec_b["slot"]).all()
    assert len(rest) >= IC.RG_INGEST_BLOCK
    a_first = rng.random(1000) < 0.5
    x, y = rec_a.copy(), rec_b.copy()  # x: the record of a pair that comes first in wire order
    x[~a_first], y[~a_first] = rec_b[~a_first], rec_a[~a_first]
    wave = np.empty(1000, dtype=IC.WIRE_DTYPE)
    wave[0::2], wave[1::2] = x[:500], y[:500]  # records 2 i and 2 i + 1: always the same wave of 64 lanes
    recs = np.concatenate([wave, x[500:], rest, y[500:]])
    if one_call:
        n_groups, drops = eng.ingest_tick(recs)
    else:
        k = split_odd(len(recs))
        drops = eng.ingest(recs[:k]) + eng.ingest(recs[k:])
        n_groups = eng.tick_ingested()
    assert drops == len(pairs), "exactly one record of each pair is dropped"
    got = eng.read_state()
    choice = IC.judge(answers[0], answers[1], got, pairs, P)
    print(f"P={P}: the engine applied A in {int((choice == 0).sum())} and B in {int((choice == 1).sum())} of {len(pairs)} groups")
    # what the engine applied, through the main oracle: everything must agree, the untouched and the `others` included
    applied = copy_state(msgs_a)
    gb, sb = pairs[choice == 1], s[choice == 1]
    applied["m_flags"][gb, sb] = msgs_b["m_flags"][gb, sb]
    for k in ("m_index", "m_commit", "m_hint", "m_rs", "m_logterm"):
        applied[k][sb, gb] = msgs_b[k][sb, gb]
    h.oracle_tick(applied)
    h.check(eng, "the applied records")
    assert h.check_results(eng, "the applied records", applied) == n_groups
    # ... and the run continues
    touched = np.sort(rng.choice(G, size=700, replace=False))
    msgs = h.new_msgs(touched)
    assert eng.ingest_tick(IC.records(msgs, touched, P, rng=rng)) == (int(msgs["m_flags"].any(axis=1).sum()), 0)
    h.oracle_tick()
    h.check(eng, "the window after")
    h.check_results(eng, "the window after")
    h.close()


@pytest.mark.parametrize("order", ["slot_adjacent", "slot_strided"])
def test_all_slots_of_a_group_at_once_claim_and_list_it_once(rg, order):
    """All 8 slots of 2000 groups carry an event and no cell twice. slot_adjacent: the 8 records of a group sit in one wave and
    claim bytes of the same two flag words (the CAS retries). slot_strided: they sit in 8 different workgroups, 2000 records
    apart (the exchange on the group's mark decides who appends it to the list). No drops, every event applied, every group
    listed once."""
    G, P = 4096, 8
    h = Harness(rg, G, P, seed=1320)
    for window in range(2):
        touched = h.rng.permutation(G)[:2000]
        msgs = h.new_msgs(touched)
        IC.fill_cells(msgs, touched, P)
        recs = IC.records(msgs, touched, P, order=order)
        assert len(recs) == 2000 * P
        feed_both(h, recs, 2000, (order, window))
    h.close()


@pytest.mark.parametrize("P", [8, 3])
def test_malformed_records_are_counted_once_and_touch_nothing(rg, P):
    """group == G, group == 2^63, slot == P, slot == 2^31, flags == 0 and flags with only bits above 0xff, scattered through a
    3000-record batch (the first and last record, and both sides of a workgroup boundary among them): each counted once, the
    state is the oracle's with the well-formed records. Then a batch of malformed records ONLY: rg_tick_ingested returns 0,
    nothing changes, and the next window works."""
    G = 4096
    h = Harness(rg, G, P, seed=1330 + P)
    a, b = h.engs
    rng = h.rng

    def malformed(like, kind):
        r = np.zeros(1, dtype=IC.WIRE_DTYPE)  # (everything else a well-formed record of a real cell: one taken for good would show)
        r[0] = like
        if kind == 0:
            r["group"] = G
        elif kind == 1:
            r["group"] = 1 << 63
        elif kind == 2:
            r["slot"] = P
        elif kind == 3:
            r["slot"] = 1 << 31
        elif kind == 4:
            r["flags"] = 0
        else:
            r["flags"] = 0x00010100 | (int(r["flags"][0]) << 16)
        return r[0]

    msgs = h.new_msgs()
    n_bad = 30
    touched = IC.fit_record_count(msgs, rng.permutation(G), 3000 - n_bad, P)
    good = IC.records(msgs, touched, P, rng=rng)
    recs = np.empty(3000, dtype=IC.WIRE_DTYPE)
    at = np.concatenate([[0, 255, 256, 257, 2999], rng.choice(np.arange(300, 2990), size=n_bad - 5, replace=False)])
    is_bad = np.zeros(3000, dtype=bool)
    is_bad[at] = True
    recs[~is_bad] = good
    for i, pos in enumerate(at):
        recs[pos] = malformed(good[i * 7], i % 6)
    feed_both(h, recs, len(touched), "30 malformed among 3000", drops=n_bad)
    # nothing but malformed records
    only_bad = np.empty(600, dtype=IC.WIRE_DTYPE)
    for i in range(600):
        only_bad[i] = malformed(good[i], i % 6)
    before = [e.read_state() for e in (a, b)]
    assert a.ingest_tick(only_bad) == (0, len(only_bad))
    assert b.ingest(only_bad) == len(only_bad) and b.ingested_duplicates() == len(only_bad)
    assert b.tick_ingested() == 0
    for e, st in zip((a, b), before):
        after = e.read_state()
        for k in fuzz.STATE_KEYS:
            assert (after[k] == st[k]).all(), k
        assert not after["out"].any() and len(e.ingested_results()[0]) == 0
        assert e.ingested_duplicates() == 0
    h.gout[:] = 0
    touched = np.sort(rng.choice(G, size=400, replace=False))
    msgs = h.new_msgs(touched)
    feed_both(h, IC.records(msgs, touched, P, rng=rng), int(msgs["m_flags"].any(axis=1).sum()), "the window after")
    h.close()


# ---- 4. density, slot counts, group commit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,gc", [(1, False), (2, False), (5, False), (8, False), (5, True), (8, True)])
def test_touched_fractions_up_to_every_cell(rg, P, gc):
    """1 %, 10 %, 40 % and 100 % of 6000 groups touched, three windows each, both call forms; at 100 % EVERY cell carries a
    record (P = 8: 48 000 records, the three-call road inside rg_ingest_tick). Slots 4..7 live in the second flag word;
    with group commit the list tick runs its group-commit instantiation."""
    G = 6000
    h = Harness(rg, G, P, seed=1400 + P, gc=gc)
    assert bool((h.st["cfg"] & 0x80000).any()) == gc
    for frac in (0.01, 0.10, 0.40, 1.0):
        for window in range(3):
            touched = np.sort(h.rng.choice(G, size=int(G * frac), replace=False))
            msgs = h.new_msgs(touched)
            if frac == 1.0:
                IC.fill_cells(msgs, touched, P)
            recs = IC.records(msgs, touched, P, rng=h.rng)
            if frac == 1.0:
                assert len(recs) == G * P
            feed_both(h, recs, int(msgs["m_flags"].any(axis=1).sum()), (P, gc, frac, window))
    h.close()


# ---- 5. reused cells and what happens between ingest and tick ---------------------------------------------------------------------
def test_a_cell_alternates_between_a_full_reject_and_a_bare_accept(rg):
    """The same cell of the same 800 groups in five consecutive windows: reject + request_snapshot + log_term + hint, then a
    plain accept whose record has those fields zero, and so on. Ingest writes hint / rs / log_term only under their flag
    bits and the tick clears only the flag row: a tick that read a stale one would leave the oracle here. A dense rg_tick
    over OTHER groups sits between windows 2 and 3."""
    G, P = 4096, 5
    st0 = base_state(G, P, seed=1500)
    rng = np.random.default_rng(1501)
    groups, s = probing_cells(st0, rng, 800, P)
    h = Harness(rg, G, P, seed=1500, n_engines=1, st=st0)
    eng = h.engs[0]
    mb = rg.MsgBuffers(G, P, eng.stride)
    for window in range(5):
        msgs = h.new_msgs(groups)
        set_cells(msgs, h.st, groups, s, "reject" if window % 2 == 0 else "accept")
        if window % 2 == 0:  # every reject carries all three here
            msgs["m_flags"][groups, s] = MF_VALID | MF_REJECT | MF_HAS_RS | MF_HAS_LOGTERM
            msgs["m_rs"][s, groups] = 3 + groups % 40
            msgs["m_logterm"][s, groups] = 1 + groups % TERM
        recs = IC.records(msgs, groups, P, rng=rng)
        n_groups = int(msgs["m_flags"].any(axis=1).sum())
        if window in (2, 3):
            k = split_odd(len(recs))
            assert eng.ingest(recs[:k]) + eng.ingest(recs[k:]) == 0 and eng.tick_ingested() == n_groups
        else:
            assert eng.ingest_tick(recs) == (n_groups, 0)
        h.oracle_tick()
        h.check(eng, window)
        h.check_results(eng, window)
        if window == 1:
            other = np.setdiff1d(np.arange(G), groups)
            dense = h.new_msgs(other)
            for k in ("m_index", "m_commit", "m_hint", "m_rs", "m_logterm", "m_flags"):
                getattr(mb, k)[...] = dense[k]
            eng.tick(mb)
            h.oracle_tick()
            h.check(eng, "dense tick between the windows")
    h.close()


def test_records_stay_pending_between_ingest_and_tick(rg):
    """What may run between rg_ingest and rg_tick_ingested, and what the tick then does: the records stay pending and are applied
    to the state as it then is. rg_tick (host columns) would stage its columns over them: refused with RG_ERR_STATE, nothing
    changed. rg_tick_device (the caller's device columns), rg_recompute, and rg_restore of a checkpoint taken before the
    ingest go through; the oracle is driven the same way."""
    import torch
    from raft_rs_amd.engine import ERR
    G, P = 4096, 5
    st0 = base_state(G, P, seed=1510)
    st0["commit"][:] = st0["commit"] // 2  # (room for rg_recompute to commit something)
    st0["pr_commit"][:, :G] = np.minimum(st0["pr_commit"][:, :G], st0["commit"])
    h = Harness(rg, G, P, seed=1510, n_engines=1, st=st0)
    eng, rng = h.engs[0], h.rng
    mb = rg.MsgBuffers(G, P, eng.stride)

    def pending_window():
        touched = np.sort(rng.choice(G, size=900, replace=False))
        msgs = h.new_msgs(touched)
        recs = IC.records(msgs, touched, P, rng=rng)
        k = split_odd(len(recs))
        assert eng.ingest(recs[:k]) + eng.ingest(recs[k:]) == 0
        return touched, int(msgs["m_flags"].any(axis=1).sum())

    def tick_pending(n_groups, what):
        assert eng.tick_ingested() == n_groups, what
        h.oracle_tick()
        h.check(eng, what)
        h.check_results(eng, what)

    # a dense tick in the gap
    touched, n_groups = pending_window()
    other = np.setdiff1d(np.arange(G), touched)
    dense = h.new_msgs(other, msgs=O.alloc_msgs(G, P))
    for k in ("m_index", "m_commit", "m_hint", "m_rs", "m_logterm", "m_flags"):
        getattr(mb, k)[...] = dense[k]
    with pytest.raises(rg.EngineError) as refused:
        eng.tick(mb)
    assert refused.value.code == ERR["STATE"]
    assert not fuzz.diff_states(h.st, eng.read_state(), G, P), "a refused rg_tick changed the state"
    cols = [torch.from_numpy(dense[k].view(np.int64).copy()).cuda() for k in ("m_index", "m_commit", "m_hint", "m_rs")]
    flags = torch.from_numpy(dense["m_flags"].copy()).cuda()
    lt = torch.from_numpy(dense["m_logterm"].view(np.int64).copy()).cuda()
    eng.tick_device(*[c.data_ptr() for c in cols], flags.data_ptr(), lt.data_ptr())
    h.oracle_tick(dense)
    h.check(eng, "rg_tick_device in the gap")
    del cols, flags, lt
    tick_pending(n_groups, "after rg_tick_device in the gap")
    # rg_recompute in the gap
    touched, n_groups = pending_window()
    eng.recompute()
    committed = np.array([1 if h.cl.maybe_commit(g) else 0 for g in range(G)], dtype=np.uint32)
    assert committed.any()
    h.gout[:] = committed
    h.cl.store_soa(h.st)
    h.check(eng, "rg_recompute in the gap")
    tick_pending(n_groups, "after rg_recompute in the gap")
    # checkpoint, a window, an ingest, restore: the pending records meet the checkpoint's state
    eng.checkpoint()
    ckpt = copy_state(h.st)
    touched, n_groups = pending_window()
    tick_pending(n_groups, "the window behind the checkpoint")
    touched, n_groups = pending_window()  # (generated for the state the restore is about to take away)
    eng.restore()
    h.st = ckpt
    h.cl = h.cluster(h.st)
    assert not fuzz.diff_states(h.st, eng.read_state(), G, P), "rg_restore"
    tick_pending(n_groups, "after rg_restore in the gap")
    # and rg_tick is only refused while records are pending
    dense = h.new_msgs(msgs=O.alloc_msgs(G, P))
    for k in ("m_index", "m_commit", "m_hint", "m_rs", "m_logterm", "m_flags"):
        getattr(mb, k)[...] = dense[k]
    eng.tick(mb)
    h.oracle_tick(dense)
    h.check(eng, "rg_tick with nothing pending")
    h.close()


def test_ingested_results_with_short_arrays(rg):
    """rg_ingested_results with cap = 0, 1, n - 1, n, n + 5, from the host copy (after rg_ingest_tick) and from the device
    (after rg_tick_ingested): *n is the true count, exactly min(cap, n) entries are written, the rest of the caller's
    arrays keeps its poison."""
    G, P = 4096, 5
    h = Harness(rg, G, P, seed=1520, n_engines=1)
    eng = h.engs[0]
    for one_call in (True, False):
        touched = np.sort(h.rng.choice(G, size=60, replace=False))
        msgs = h.new_msgs(touched)
        recs = IC.records(msgs, touched, P, rng=h.rng)
        if one_call:
            n = eng.ingest_tick(recs)[0]
        else:
            assert eng.ingest(recs) == 0
            n = eng.tick_ingested()
        h.oracle_tick()
        assert h.check_results(eng, one_call) == n > 10
        full = eng.ingested_results()
        for cap in (0, 1, n - 1, n, n + 5):
            groups, commit, out, count = eng.ingested_results(cap=cap)
            k = min(cap, n)
            assert count == n and len(groups) == len(commit) == len(out) == cap, (one_call, cap)
            for got, want in zip((groups, commit, out), full):
                assert (got[:k] == want[:k]).all(), (one_call, cap)
            assert (groups[k:] == 0xA5A5A5A5A5A5A5A5).all() and (commit[k:] == 0xA5A5A5A5A5A5A5A5).all()
            assert (out[k:] == 0xA5A5A5A5).all(), (one_call, cap)
    h.close()


# ---- 6. the contract of the duplicate counts -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n_host", [20000, 200, 3000, "rg_ingest"])
def test_duplicate_counts_rg_ingest_its_own_call_the_others_the_window(rg, n_host):
    """A window opened by rg_ingest_device with 3 duplicates, closed by a host batch with 2 more (one a copy of a record of
    its own, one a copy of a device-side record): rg_ingest_tick returns 5 on every road -- 20 000 records (three calls),
    200 (one launch), 3000 (round trip) --, rg_ingest returns 2 and rg_ingested_duplicates then 5."""
    G, P = 8192, 5
    h = Harness(rg, G, P, seed=1600, n_engines=1)
    eng, rng = h.engs[0], h.rng
    total = 20000 if n_host == "rg_ingest" else n_host
    assert (total > IC.RG_ROUNDTRIP_MAX) == (total == 20000)
    msgs = h.new_msgs()
    perm = rng.permutation(G)
    host_msgs = copy_state(msgs)
    dev_groups = IC.fit_record_count(msgs, perm[:100], 300, P)
    host_groups = IC.fit_record_count(host_msgs, perm[100:], total - 2, P)
    dev_recs = IC.records(msgs, dev_groups, P, rng=rng)
    host_recs = IC.records(host_msgs, host_groups, P, rng=rng)
    dev_all = np.concatenate([dev_recs, dev_recs[:3]])
    host_all = np.concatenate([host_recs[:total // 2], host_recs[7:8], host_recs[total // 2:], dev_recs[11:12]])
    assert len(host_all) == total and len(dev_all) + 200 <= IC.RG_ZEROCOPY_MAX
    dev = to_device(dev_all)
    eng.ingest_device(dev.data_ptr(), len(dev_all))
    n_groups = len(dev_groups) + len(host_groups)
    if n_host == "rg_ingest":
        assert eng.ingest(host_all) == 2, "rg_ingest reports the drops of its own call"
        assert eng.ingested_duplicates() == 5, "rg_ingested_duplicates reports the window's"
        assert eng.tick_ingested() == n_groups
    else:
        assert eng.ingest_tick(host_all) == (n_groups, 5), "rg_ingest_tick reports the drops of the whole window"
    assert eng.ingested_duplicates() == 0
    del dev
    msgs["m_flags"][host_groups] = host_msgs["m_flags"][host_groups]
    h.oracle_tick()
    h.check(eng, n_host)
    assert h.check_results(eng, n_host) == n_groups
    h.close()
