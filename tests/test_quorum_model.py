"""CPU: tests/quorum_model.py against the reference's golden vote vectors and the oracle, before the model judges a kernel
(tests/test_tick_unit_edges_gpu.py). Every comparison is exact."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import fuzz
import oracle_lib as O
import quorum_model as M
from test_oracle_golden import build_case

HERE = os.path.dirname(os.path.abspath(__file__))
VEC = json.load(open(os.path.join(HERE, "golden", "quorum_vectors.json"), encoding="utf-8"))
NAMES = {"VotePending": 0, "VoteLost": 1, "VoteWon": 2}
G_ORACLE = 2500


def cfg_make(incoming, outgoing=0, self_slot=0, present=None):
    present = (incoming | outgoing) if present is None else present
    return incoming | (outgoing << 8) | (self_slot << 16) | (present << 24)


def test_vote_result_golden_vectors():
    cfg, yes, no, want, names = [], [], [], [], []
    for fname in ("majority_vote.txt", "joint_vote.txt"):
        for case in VEC[fname]:
            ids, idsj, _, look = build_case(case["args"], key="votes")
            slot = {pid: k for k, pid in enumerate(sorted(set(ids) | set(idsj)))}
            m = lambda s: sum(1 << slot[i] for i in s)
            cfg.append(cfg_make(m(ids), m(idsj)))
            yes.append(m([i for i, v in look.items() if v == 2]))
            no.append(m([i for i, v in look.items() if v == 1]))
            want.append(NAMES[case["result"]])
            names.append(f"{fname}:{case['line']}")
    assert len(want) == 61
    cfg, yes, no, want = (np.array(a, dtype=np.uint32) for a in (cfg, yes, no, want))
    got = M.vote_result(cfg, yes, no)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(names[i], int(got[i]), int(want[i])) for i in bad[:5]]
    # joint symmetry (datadriven_test.rs:296-301): the two majorities swapped
    swapped = ((cfg & 0xff) << 8) | ((cfg >> 8) & 0xff) | (cfg & 0xffff0000)
    assert (M.vote_result(swapped, yes, no) == want).all()
    # a slot in both masks is a yes (record_vote keeps the first vote); the tally counts it once
    g, r, res = M.tally_votes(np.array([cfg_make(0b111)]), np.array([0b011]), np.array([0b110]))
    assert (int(g[0]), int(r[0]), int(res[0])) == (2, 1, M.WON)


def random_shard(seed, P, gc=False):
    rng = np.random.default_rng(seed)
    st = O.alloc_state(G_ORACLE, P)
    st["cfg"][:] = fuzz.random_cfg(rng, G_ORACLE, P, joint_frac=0.4, learner_frac=0.4, missing_progress_frac=0.15,
                                   group_commit_frac=0.7 if gc else 0.0)
    fuzz.random_state(rng, st, small_values=True, with_gids=gc)
    st["pflags"][:, :] = rng.integers(0, 256, size=(G_ORACLE, 8), dtype=np.uint8) & 0x2c | (st["pflags"] & 3)
    cl = O.Cluster(G_ORACLE)
    cl.load_soa(st, term=3)
    return rng, st, cl


@pytest.mark.parametrize("P", [3, 8])
def test_tally_votes_matches_oracle(P):
    rng, st, cl = random_shard(100 + P, P)
    G, L = G_ORACLE, O.lib()
    yes = rng.integers(0, 256, size=G, dtype=np.uint8)  # (bits at or above P: no voter there, they count nowhere)
    no = rng.integers(0, 256, size=G, dtype=np.uint8)
    granted, rejected, res = M.tally_votes(st["cfg"], yes, no)
    assert (res == M.vote_result(st["cfg"], yes, no)).all()
    seen = set()
    for g in range(G):
        y, n = int(yes[g]), int(no[g]) & ~int(yes[g])
        ids = [p + 1 for p in range(8) if ((y | n) >> p) & 1]
        votes = [2 if (y >> (i - 1)) & 1 else 1 for i in ids]
        a, b = C.c_size_t(0), C.c_size_t(0)
        want = L.ro_group_tally_votes(cl.h, g, O.u64arr(ids or [0]), (C.c_uint8 * max(1, len(ids)))(*votes), len(ids),
                                      C.byref(a), C.byref(b))
        assert (int(granted[g]), int(rejected[g]), int(res[g])) == (a.value, b.value, want), g
        seen.add(want)
    assert seen == {0, 1, 2}


@pytest.mark.parametrize("P", [3, 8])
def test_quorum_recently_active_matches_oracle(P):
    _, st, cl = random_shard(200 + P, P)
    G, L = G_ORACLE, O.lib()
    self_id = ((st["cfg"] >> 16) & 7).astype(np.int64) + 1
    present = (st["cfg"] >> 24) & 0xff
    pf = st["pflags"].copy()
    for sweep in range(2):  # the second sweep meets the bits the first one left
        got, after = M.quorum_recently_active(st["cfg"], pf)
        want = np.array([L.ro_quorum_recently_active(cl.h, g, int(self_id[g])) for g in range(G)])
        assert (got.astype(bool) == want).all(), (sweep, np.nonzero(got.astype(bool) != want)[0][:5])
        assert 0 < want.sum() < G
        cl.store_soa(st)  # (the oracle writes the Progress fields of present slots only)
        for p in range(8):
            sel = ((present >> p) & 1) == 1
            assert ((after[sel, p] ^ st["pflags"][sel, p]) & M.PF_RECENT_ACTIVE == 0).all(), (sweep, p)
            assert (after[~sel, p] == pf[~sel, p]).all()
        assert ((after ^ pf) & ~np.uint8(M.PF_RECENT_ACTIVE) == 0).all()
        pf = after


@pytest.mark.parametrize("P", [3, 8])
def test_heartbeat_commits_match_oracle(P):
    _, st, cl = random_shard(300 + P, P)
    G, L = G_ORACLE, O.lib()
    hb = M.heartbeat_commits(st["cfg"], st["match"], st["commit"])
    assert hb.shape == (P, G)
    for p in range(P):
        want = np.array([L.ro_heartbeat_commit(cl.h, g, p + 1) for g in range(G)], dtype=np.uint64)
        assert (hb[p] == want).all(), (p, np.nonzero(hb[p] != want)[0][:5])
    assert (hb == st["commit"][None, :]).any() and (hb < st["commit"][None, :]).any()


@pytest.mark.parametrize("gc", [False, True])
@pytest.mark.parametrize("P", [3, 8])
def test_maximal_committed_index_matches_oracle(P, gc):
    _, st, cl = random_shard(400 + P + (50 if gc else 0), P, gc=gc)
    G = G_ORACLE
    mci, used = M.maximal_committed_index(st["cfg"], st["match"], st["gid"])
    want = [cl.mci(g) for g in range(G)]
    wi = np.array([w[0] for w in want], dtype=np.uint64)
    wf = np.array([w[1] for w in want], dtype=bool)
    assert (mci == wi).all(), np.nonzero(mci != wi)[0][:5]
    assert (used == wf).all(), np.nonzero(used != wf)[0][:5]
    if gc:
        assert 0 < wf.sum() < G


def test_census_and_reject_models_on_worked_examples():
    """The functions without an oracle entry point, on cases small enough to check by eye against the header / the reference."""
    cfg = np.array([cfg_make(0b011, self_slot=0, present=0b111), cfg_make(0b110, self_slot=1, present=0b101)], dtype=np.uint32)
    f = np.zeros((2, 8), dtype=np.uint8)
    f[0, 0] = 0x02          # election on the own slot (no VALID needed), not a reject
    f[0, 1] = 0x03          # a reject
    f[0, 2] = 0x02          # REJECT without VALID: neither a message nor a reject
    f[1, 1] = 0x03          # own slot without a Progress: no election, and never a reject
    f[1, 0] = 0x01
    assert M.msg_stats(f, cfg) == [3, 1, 5, 2, 1]
    out = np.array([0x1, 0x3, 0x22, 0x20, 0], dtype=np.uint32)
    assert M.result_counts(out) == (2, 2)
    assert M.host_hints(out, np.array([9, 9, 5, 1, 7], dtype=np.uint8)) == {2: 5, 3: 1}
    # maybe_decr_to (progress.rs:168-206): Probe not stale / Probe stale / Replicate not stale (-> Probe) / Replicate stale /
    # hint + 1 above the rejected index / next would fall to 0
    match = [3, 3, 3, 9, 3, 0]
    nxt = [8, 9, 12, 12, 8, 1]
    psnap = [0, 0, 6, 6, 0, 0]
    pf = [0x04 | 0, 0x04 | 0, 0x44 | 1, 0x44 | 1, 2, 0]
    index = [7, 7, 9, 9, 7, 0]
    hint = [4, 4, 4, 4, 20, 0]
    ok, n2, s2, p2 = M.resolved_reject(match, nxt, psnap, pf, index, hint)
    assert ok.tolist() == [True, False, True, False, True, True]
    assert n2.tolist() == [5, 9, 4, 12, 7, 1]
    assert s2.tolist() == [0, 0, 0, 6, 0, 0]
    assert p2.tolist() == [0, 0x04, 0, 0x45, 2, 0]
