"""CPU: the helpers of the ingest edge tests (tests/ingestcheck.py) -- the road constants mirror the kernels' headers, the
record builders produce the orders they promise, and the judge accepts A, B and per-group mixtures and nothing else."""
import numpy as np
import pytest

import fuzz
import ingestcheck as IC
import oracle_lib as O


def test_road_constants_mirror_the_kernel_headers():
    got = IC.parse_road_constants()
    assert got == {"RG_INGEST_BLOCK": IC.RG_INGEST_BLOCK, "RG_ZEROCOPY_MAX": IC.RG_ZEROCOPY_MAX,
                   "RG_ROUNDTRIP_MAX": IC.RG_ROUNDTRIP_MAX}, \
        "a road threshold moved: move tests/ingestcheck.py (and with it the sizes of test_ingest_edges_gpu.py) along"
    assert IC.RG_INGEST_BLOCK < IC.RG_ZEROCOPY_MAX < IC.RG_ROUNDTRIP_MAX
    counts = IC.edge_counts(8192)
    for edge in (IC.RG_INGEST_BLOCK, 2 * IC.RG_INGEST_BLOCK, IC.RG_ZEROCOPY_MAX, IC.RG_ROUNDTRIP_MAX):
        assert edge in counts and edge + 1 in counts
    assert 1 in counts and IC.RG_INGEST_BLOCK - 1 in counts and max(counts) > IC.RG_ROUNDTRIP_MAX + 1


def test_wire_dtype_is_the_64_byte_record():
    assert IC.WIRE_DTYPE.itemsize == 64
    assert [IC.WIRE_DTYPE.fields[n][1] for n in ("group", "index", "commit", "hint", "rs", "log_term", "slot", "flags", "pad")] \
        == [0, 8, 16, 24, 32, 40, 48, 52, 56]


def _msgs(rng, G, P, fill=0.7):
    m = O.alloc_msgs(G, P)
    m["m_flags"][:, :P] = np.where(rng.random((G, P)) < fill, rng.integers(1, 256, size=(G, P)), 0).astype(np.uint8)
    for k in ("m_index", "m_commit", "m_hint", "m_rs", "m_logterm"):
        m[k][:, :G] = rng.integers(1, 1 << 40, size=(P, G), dtype=np.uint64)
    return m


@pytest.mark.parametrize("order", IC.ORDERS)
def test_records_carry_every_event_once_in_the_promised_order(order):
    rng = np.random.default_rng(3)
    G, P = 700, 8
    m = _msgs(rng, G, P, fill=1.0 if order != "shuffled" else 0.6)
    groups = rng.permutation(G)[:600]
    recs = IC.records(m, groups, P, order=order, rng=rng)
    assert len(recs) == int(np.count_nonzero(m["m_flags"][groups, :P]))
    g, p = recs["group"].astype(np.int64), recs["slot"].astype(np.int64)
    assert len(set(zip(g.tolist(), p.tolist()))) == len(recs)  # one record per cell
    assert set(g.tolist()) == set(groups.tolist())
    assert (recs["flags"] == m["m_flags"][g, p]).all() and (recs["pad"] == 0).all()
    for col, k in (("index", "m_index"), ("commit", "m_commit"), ("hint", "m_hint"), ("rs", "m_rs"), ("log_term", "m_logterm")):
        assert (recs[col] == m[k][p, g]).all(), col
    if order == "slot_adjacent":  # 8 consecutive records per group, aligned: never across a wave of 64 lanes
        assert (g.reshape(-1, P) == g.reshape(-1, P)[:, :1]).all() and (p.reshape(-1, P) == np.arange(P)).all()
    if order == "slot_strided":   # block s = slot s of every group: one group's records are a whole block apart
        assert (p == np.repeat(np.arange(P), len(groups))).all()
        assert (g.reshape(P, -1) == groups).all() and len(groups) >= 2 * IC.RG_INGEST_BLOCK


def test_fit_record_count_trims_and_pads_to_the_exact_count():
    rng = np.random.default_rng(4)
    G, P = 300, 5
    for n in (1, 255, 256, 257, 700, G * P - 1, G * P):
        m = _msgs(rng, G, P)
        before = m["m_flags"].copy()
        order = rng.permutation(G)
        touched = IC.fit_record_count(m, order, n, P)
        f = m["m_flags"]
        assert int(np.count_nonzero(f)) == n and (f[:, P:] == 0).all()
        assert (touched == np.nonzero(f.any(axis=1))[0]).all()
        kept = (f != 0) & (before != 0)
        assert (f[kept] == before[kept]).all()                     # trimming never rewrites an event
        assert set(np.unique(f[(f != 0) & (before == 0)]).tolist()) <= {fuzz.MF_SENT}  # padding uses the pad event only
        assert len(IC.records(m, touched, P, rng=rng)) == n
    m = _msgs(rng, G, P, fill=0.3)
    IC.fill_cells(m, [3, 5], P)
    assert (m["m_flags"][[3, 5], :P] != 0).all() and (m["m_flags"][:, P:] == 0).all()


# ---- the judge ----
def _state(rng, G, P):
    st = O.alloc_state(G, P)
    for k in ("match", "next", "pr_commit", "pend_snap", "pend_rs", "gid"):
        st[k][:, :G] = rng.integers(0, 1000, size=(P, G), dtype=np.uint64)
    st["pflags"][:, :P] = rng.integers(0, 16, size=(G, P), dtype=np.uint8)
    for k in ("commit", "term_lo", "term_hi"):
        st[k][:] = rng.integers(0, 1000, size=G, dtype=np.uint64)
    st["cfg"][:] = np.uint32(((1 << P) - 1) | (((1 << P) - 1) << 24))
    st["out"] = rng.integers(0, 1 << 20, size=G, dtype=np.uint32)
    return st


def _copy(st):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}


def _take(dst, src, g, keys):
    for k in keys:
        if k == "pflags":
            dst[k][g, :] = src[k][g, :]
        elif dst[k].ndim == 2:
            dst[k][:, g] = src[k][:, g]
        else:
            dst[k][g] = src[k][g]


@pytest.fixture(scope="module")
def ab():
    """Two states that differ in the cell (slot 1) of every judged group the way an accept (A: match moves, Replicate) and a
    reject of a probing peer (B: next and pending_request_snapshot move) do, and in the result word."""
    rng = np.random.default_rng(5)
    G, P = 64, 3
    base = _state(rng, G, P)
    groups = np.arange(0, G, 2)
    a, b = _copy(base), _copy(base)
    a["match"][1, groups] += 3
    a["next"][1, groups] = a["match"][1, groups] + 1
    a["pr_commit"][1, groups] += 1
    a["pflags"][groups, 1] = 1 | 8
    a["commit"][groups] += 1
    a["out"][groups] = 1
    b["next"][1, groups] -= 1
    b["pend_rs"][1, groups] = 77
    b["pflags"][groups, 1] = 0 | 8
    b["out"][groups] = 1 << 9
    return G, P, groups, a, b


def test_judge_accepts_all_a_all_b_and_per_group_mixtures(ab):
    G, P, groups, a, b = ab
    IC.assert_distinguishable(a, b, groups, P)
    assert (IC.judge(a, b, _copy(a), groups, P) == 0).all()
    assert (IC.judge(a, b, _copy(b), groups, P) == 1).all()
    mix = _copy(a)
    from_b = groups[::3]
    for g in from_b:
        _take(mix, b, g, IC.JUDGED_KEYS)
    choice = IC.judge(a, b, mix, groups, P)
    assert (choice == np.isin(groups, from_b)).all() and 0 < choice.sum() < len(groups)


def test_judge_rejects_a_mix_inside_one_group(ab):
    G, P, groups, a, b = ab
    g = int(groups[7])
    torn = _copy(a)                      # match of A ...
    _take(torn, b, g, ("pr_commit", "next"))  # ... pr_commit / next of B
    with pytest.raises(AssertionError, match=f"neither A nor B.*group {g}:"):
        IC.judge(a, b, torn, groups, P)
    for key in IC.JUDGED_KEYS:           # and a single foreign column of any kind is enough
        if np.array_equal(a[key], b[key]):
            continue
        torn = _copy(a)
        _take(torn, b, g, (key,))
        with pytest.raises(AssertionError, match="neither A nor B"):
            IC.judge(a, b, torn, groups, P)
    neither = _copy(a)                   # a group in which neither record was applied
    neither["match"][1, g] += 100
    with pytest.raises(AssertionError, match="neither A nor B"):
        IC.judge(a, b, neither, groups, P)


def test_judge_refuses_indistinguishable_inputs(ab):
    G, P, groups, a, b = ab
    same = _copy(b)
    _take(same, a, int(groups[2]), IC.JUDGED_KEYS)
    with pytest.raises(AssertionError, match="could not tell"):
        IC.assert_distinguishable(a, same, groups, P)
    with pytest.raises(AssertionError, match="indistinguishable"):
        IC.judge(a, same, _copy(a), groups, P)
    # columns of slots the cfg word has no Progress for are not compared (as in fuzz.diff_states)
    a2 = _copy(a)
    a2["cfg"][:] = np.uint32(0b011 | (0b011 << 24))
    junk = _copy(a2)
    junk["match"][2, :] += 9
    assert (IC.judge(a2, b, junk, groups, P) == 0).all()
