"""GPU: k_tick_mirror (raft_rs_amd/csrc/rg_mirror.h) at the edges of its word, with ONE escaping lane in a steady wave, at every
slot count and in both cached regimes, and the escape watch on both sides of its bound.

Every case runs a mirror-on engine beside a RG_CFGF_NO_READ_MIRROR twin and the oracle (readmirror.Rig) and asserts its launch
counts: a case that ran build ticks only fails. The first packed tick uses readmirror.deciding_acks, under which the commit index
is the decoded `matched` of a slot that gets no message -- tests/test_mirror_host.py shows on the host twin that a word wrong by
one then changes `commit`."""
import numpy as np
import pytest

import fuzz
import oracle_lib as O
from readmirror import EDGE_COMMITS, KINDS, MSG_KEYS, Rig, absent_garbage, deciding_acks, plant_edges, plant_wave, wave_groups

pytestmark = pytest.mark.gpu
TERM = 5


def edge_state(rng, G, P, base=0):
    """A random shard (absent slots hold garbage within reach of the commit index) with plant_edges on every 4th group."""
    st = O.add_term_table(O.alloc_state(G, P))
    st["cfg"][:] = fuzz.random_cfg(rng, G, P)
    fuzz.random_state(rng, st, base=base)
    absent_garbage(rng, st)
    planted = list(range(3, G, 4))
    plant_edges(rng, st, planted)
    fuzz.random_term_table(rng, st, TERM, max_runs=3)
    return st, planted


def run_edges(rg, G, P, seed, cache_policy, device_msgs, streaming, base=0):
    rng = np.random.default_rng(seed)
    st, planted = edge_state(rng, G, P, base)
    rig = Rig(rg, st, TERM, cache_policy=cache_policy, device_msgs=device_msgs)
    # the oracle sees what the case says it sees: every group of the background, and every planted group whose cells are plain
    # indices; only planted groups at the commits where cells wrap below 0 or sit at 2^63 - 1 are left to the two engines
    plain, wrapping = ((1 << 32) - 1, 1 << 32, 3_000_000), (0, 5, 40_000, 65_535, (1 << 63) - 1)
    assert set(plain) | set(wrapping) == set(EDGE_COMMITS)
    is_planted = np.zeros(G, dtype=bool)
    is_planted[planted] = True
    assert rig.mask[~is_planted].all(), np.nonzero(~rig.mask & ~is_planted)[0][:5]
    for g in planted:
        c = int(st["commit"][g])
        assert c in EDGE_COMMITS and (rig.mask[g] or c in wrapping) and (rig.mask[g] or c not in plain), (g, c)
    assert all(any(int(st["commit"][g]) == c and rig.mask[g] for g in planted) for c in plain)
    assert not any(rig.mask[g] for g in planted if int(st["commit"][g]) == (1 << 63) - 1) and not rig.mask[planted].all()
    msgs = O.alloc_msgs(G, P)
    moved = 0
    for t in range(5):
        cur = rig.oracle_state()
        if t == 0:  # the build tick: the planted groups sit it out, so their planted cells are what is encoded
            fuzz.random_msgs(rng, cur, msgs)
            msgs["m_flags"][planted, :] = 0
        elif t == 1:
            fuzz.random_msgs(rng, cur, msgs)
            decided = [(g, s) for g, s in deciding_acks(cur, msgs, planted) if rig.mask[g]]
            want = {g: int(cur["match"][s, g]) for g, s in decided}
            before = cur["commit"].copy()
        else:  # an election inside a packed tick stores matched = 0: escapes the NEXT packed tick serves from the columns
            fuzz.random_msgs(rng, cur, msgs, elect_p=0.1, elect_term=TERM + t, reject_p=0.25)
            for g in np.nonzero(~rig.mask)[0]:  # (outside the oracle's domain: no election; its term table is not modelled there)
                msgs["m_flags"][g, (int(cur["cfg"][g]) >> 16) & 7] &= ~np.uint8(fuzz.MF_REJECT)
        rig.tick(msgs, streaming=streaming)
        if t == 1:
            after = rig.oracle_state()
            moved = sum(1 for g, v in want.items() if int(after["commit"][g]) == v and v > int(before[g]))
            assert moved == len(want), (moved, len(want))
    if P > 1:  # (one slot: the leader's own cell is the only one, and it never is silent)
        assert moved > 0
        assert rig.rejected > 0
    assert rig.elected > 0, rig.elected
    rig.finish(packed=4)


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 6, 7, 8])
def test_planted_word_edges_at_every_slot_count(rg, P):
    """Cached regime (RG_CACHE_PLAIN), rg_tick from host buffers. The planted groups whose cells wrap around 0 or sit at 2^63 - 1
    are outside the oracle's domain (the reference's arithmetic is not defined there): they are compared between the two
    engines only, cell for cell; every other group also against the oracle."""
    run_edges(rg, 257, P, 0xED6E + P, rg.CACHE.PLAIN, False, 0)


@pytest.mark.parametrize("P", [1, 5, 8])
def test_planted_word_edges_with_streamed_messages(rg, P):
    """RG_CACHE_STREAM_MSGS, rg_tick_device from device buffers: the NTM instantiations of k_tick_mirror (regime 1)."""
    run_edges(rg, 257, P, 0x57E + P, rg.CACHE.STREAM_MSGS, True, 1)


@pytest.mark.parametrize("P", [3, 5, 8])
def test_high_bases(rg, P):
    """The whole shard in the 2^62 region (fuzz.random_state(base=2**62), inside the oracle's domain as
    tests/test_parity_gpu.py::test_tiny_and_ragged_group_counts shows), the planted groups at 2^32 - 1 and 2^32 as well. The
    planted commits at 0 (cells that wrap below it) and at 2^63 - 1 are outside the oracle's domain: engines only."""
    run_edges(rg, 257, P, 0xB16 + P, rg.CACHE.PLAIN, False, 0, base=2 ** 62)


# (G, the planted wave, its lanes): first, middle and tail waves, the tail partial where G says so (a partial wave has no lane
# 63: its last lane stands in), every lane set in every position
LAYOUTS = ((1, 0, (0,)), (63, 0, (0, 62)), (63, 0, (31,)), (65, 1, (0,)), (65, 0, (63,)), (100, 1, (31,)), (100, 1, (0, 35)), (100, 1, (35,)),
           (128, 1, (0, 63)), (128, 1, (63,)), (129, 1, (31,)), (129, 2, (0,)), (257 + 64, 0, (0, 63)), (257 + 64, 0, (31,)),
           (257 + 64, 2, (63,)), (257 + 64, 2, (0, 63)), (257 + 64, 3, (0,)), (257 + 64, 5, (0,)))


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("P", [3, 5, 7])
def test_one_escaping_lane_in_a_steady_wave(rg, P, kind):
    """ONE lane (or two) of a wave holds a field its word cannot represent, the other lanes and every other wave are steady: the
    wave-uniform escape branch of rg_load_group_pk overwrites 63 decoded register sets with their cells, and under deciding_acks
    on the whole planted wave and one steady wave the commit index of each of those groups is one of those registers."""
    for G, wave, lanes in LAYOUTS:
        rng = np.random.default_rng(G * 1000 + wave * 10 + P)
        st = O.add_term_table(O.alloc_state(G, P))
        st["cfg"][:] = fuzz.random_cfg(rng, G, P, transfer_frac=0.0)
        fuzz.random_state(rng, st)
        n_waves = (G + 63) // 64
        for w in range(n_waves):
            plant_wave(st, w, (), kind)
        planted = plant_wave(st, wave, lanes, kind)
        assert len(planted) == len(lanes)
        fuzz.random_term_table(rng, st, TERM, max_runs=3)
        rig = Rig(rg, st, TERM, cache_policy=rg.CACHE.PLAIN)
        assert rig.mask.all()
        msgs = O.alloc_msgs(G, P)
        for t in range(4):
            cur = rig.oracle_state()
            msgs["m_flags"][...] = 0
            if t == 1:
                listed = sorted(set(wave_groups(cur, wave)) | set(wave_groups(cur, (wave + 1) % n_waves)))
                decided = deciding_acks(cur, msgs, listed)
                want = {g: int(cur["match"][s, g]) for g, s in decided}
                assert len(want) >= len(listed) // 4 or G == 1, (G, len(want))
            elif t > 1:
                fuzz.random_msgs(rng, cur, msgs, elect_p=0.05, elect_term=TERM + t, reject_p=0.2)
            rig.tick(msgs, streaming=0)
            if t == 1:
                got = rig.oracle_state()
                assert all(int(got["commit"][g]) == v for g, v in want.items()), (G, wave, lanes)
        rig.finish(packed=3)


# ---- the escape watch on both sides of its bound -------------------------------------------------------------------------------
WATCH_G, WATCH_P, LAG_SLOT = 1024, 5, 4


def watch_state(rg, escaping):
    """Five voters, the leader in slot 0, every wave steady; in the listed (wave, lane) groups the follower of LAG_SLOT has
    matched = commit - 40 000 and never gets a message while the others ack: its word's low field is the escape for good."""
    from raft_rs_amd import engine as E
    G, P = WATCH_G, WATCH_P
    st = O.alloc_state(G, P)
    st["cfg"][:] = E.cfg_make(0b11111, self_slot=0, present=0b11111)
    for w in range(G // 64):
        plant_wave(st, w, (), "mt_lo")
    st["match"][0, :G] = st["term_hi"]  # the leader has persisted its whole log
    st["next"][0, :G] = st["term_hi"] + np.uint64(1)
    lag = [64 * w + lane for w, lane in escaping]
    for g in lag:
        st["match"][LAG_SLOT, g] = st["commit"][g] - np.uint64(40_000)
        st["next"][LAG_SLOT, g] = st["match"][LAG_SLOT, g] + np.uint64(1)
    return st, lag


def watch_msgs(st, lag, t):
    """Tick t: the leader appends two entries and persists them, every follower but the lagging ones acks the last index the
    leader had before (the log is at hi0 + 2 t when the tick starts) and reports the commit index of the tick before."""
    G, P = WATCH_G, WATCH_P
    m = O.alloc_msgs(G, P)
    hi = st["term_hi"] + np.uint64(2 * t)
    m["m_flags"][:, 0] = fuzz.MF_APPEND | fuzz.MF_VALID
    m["m_index"][0, :G] = m["m_commit"][0, :G] = hi + np.uint64(2)
    for p in range(1, P):
        m["m_flags"][:, p] = fuzz.MF_VALID
        m["m_index"][p, :G] = hi
        m["m_commit"][p, :G] = st["commit"] if t == 0 else hi - np.uint64(2)
    m["m_flags"][lag, LAG_SLOT] = 0
    return m


def run_watch(rg, escaping, launches):
    """-> mirror_stats after every launch (read without a synchronisation). Both engines tick from the same device buffers;
    before launches 32, 64, 96 the streams are synchronised (the pinned escape count then is exact at the watch's look, which
    rg_plan_tick takes in front of launches 32, 64, 96: every 32 mirror launches) and every column is compared."""
    import torch
    st, lag = watch_state(rg, escaping)
    on = rg.Engine(WATCH_G, WATCH_P, flags=rg.CFGF.NO_SIZE_CLASSES, cache_policy=rg.CACHE.PLAIN)
    off = rg.Engine(WATCH_G, WATCH_P, flags=rg.CFGF.NO_SIZE_CLASSES | rg.CFGF.NO_READ_MIRROR, cache_policy=rg.CACHE.PLAIN)
    for e in (on, off):
        e.load_state(st)

    def compare(t):
        a, b = on.read_state(), off.read_state()
        diffs = fuzz.diff_states(a, b, WATCH_G, WATCH_P, present_only=False)
        assert not diffs, (t, diffs[:5])
        assert (a["out"] == b["out"]).all(), t
        return a

    dev = []
    for t in range(launches):
        m = watch_msgs(st, lag, t)
        dev.append([torch.from_numpy(np.ascontiguousarray(m[k]).view(np.uint8 if k == "m_flags" else np.int64).copy()).cuda()
                    for k in MSG_KEYS])
    stats = []
    for t in range(launches):
        if t and t % 32 == 0:
            on.sync()
            off.sync()
            compare(t)
        for e in (on, off):
            e.tick_device(*[d.data_ptr() for d in dev[t]])
        stats.append(on.mirror_stats())
    on.sync()
    off.sync()
    a = compare(launches)
    # the stream did what the case needs: every group committed two entries per tick, the lagging cells never moved
    assert (a["commit"] == st["term_hi"] + np.uint64(2 * launches - 2)).all()
    assert (a["match"][LAG_SLOT, lag] == st["match"][LAG_SLOT, lag]).all()
    final = on.mirror_stats()
    assert off.mirror_stats()["build_launches"] == off.mirror_stats()["packed_launches"] == 0
    on.close()
    off.close()
    return stats, final


def test_a_steady_stream_keeps_the_mirror_across_windows(rg):
    """No escape anywhere, 70 launches: two looks of the watch (windows of 32 mirror launches), the mirror stays."""
    stats, s = run_watch(rg, (), 70)
    assert [(x["build_launches"], x["packed_launches"], x["off"]) for x in stats] == [(1, i, 0) for i in range(70)]
    assert (s["build_launches"], s["packed_launches"], s["valid"], s["off"]) == (1, 69, 1, 0), s


def test_one_escaping_wave_in_sixteen_keeps_the_mirror(rg):
    """The keep side of the bound: the watch switches off when (escaping waves seen) * 8 > launches * waves = 32 * 16 = 512 per
    window. One wave of 16 stores an escape per launch: 32 per window, and the pinned word trails the device count by at most
    15, so at most 47 are seen in a window: 376 <= 512. Three looks in 100 launches, the mirror stays."""
    stats, s = run_watch(rg, ((7, 31),), 100)
    assert [(x["build_launches"], x["packed_launches"], x["off"]) for x in stats] == [(1, i, 0) for i in range(100)]
    assert (s["build_launches"], s["packed_launches"], s["valid"], s["off"]) == (1, 99, 1, 0), s


def test_four_escaping_waves_in_sixteen_switch_the_mirror_off(rg):
    """The other side: four waves of 16, 128 per window -- a multiple of 16, so the pinned word is exact after the
    synchronisation -- and 1024 > 512. The word is read without synchronisation by design, so the launch at which the engine
    notices is not asserted beyond: by launch 65 (the second look) at the latest, and no packed launch is counted afterwards."""
    stats, s = run_watch(rg, ((1, 0), (5, 31), (9, 63), (13, 17)), 100)
    assert stats[65]["off"] == 2 and stats[65]["valid"] == 0, stats[65]
    first = next(i for i, x in enumerate(stats) if x["off"] == 2)
    assert first >= 32, first  # (no look before a window is full)
    assert all(x["packed_launches"] == stats[first]["packed_launches"] and x["valid"] == 0 for x in stats[first:])
    assert (s["build_launches"], s["off"], s["valid"]) == (1, 2, 0) and s["packed_launches"] == stats[first]["packed_launches"] >= 31, s
