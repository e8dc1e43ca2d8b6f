"""GPU: the control and reduction kernels of the tick unit (raft_rs_amd/csrc/rg_kernels_quorum.h behind abi_tick.hip) at their edges,
against tests/quorum_model.py (pinned to the reference's golden vectors and the oracle by tests/test_quorum_model.py): votes and
tallies, quorum liveness, heartbeat commits, the two censuses, the host-hint list and its answers, the group-commit flag.
Every comparison is exact."""
import numpy as np
import pytest

import fuzz
import hosthints
import oracle_lib as O
import quorum_model as M
import sendstage

pytestmark = pytest.mark.gpu

HH = hosthints.OUT_HOST_HINT
SENTINEL = 0xA5A5A5A5A5A5A5A5


# ---- shared builders ----------------------------------------------------------------------------------------------------
def cfg_words(incoming, outgoing, self_slot, present, group_commit=False):
    """RG_CFG_MAKE over arrays."""
    a = [np.asarray(x).astype(np.uint32) for x in (incoming, outgoing, self_slot, present)]
    return (a[0] | (a[1] << 8) | (a[2] << 16) | (np.asarray(group_commit).astype(np.uint32) << 19) | (a[3] << 24)).astype(np.uint32)


def random_cfg(rng, G, P, group_commit=False):
    """Every shape rg_load_column accepts over P slots, vectorised: empty and one-sided joint configurations, learners, voters
    without a Progress, a self slot without one."""
    full = (1 << P) - 1
    inc = rng.integers(0, full + 1, size=G)
    out = np.where(rng.random(G) < 0.5, rng.integers(0, full + 1, size=G), 0)
    self_slot = rng.integers(0, P, size=G)
    present = (inc | out | rng.integers(0, full + 1, size=G) | (1 << self_slot)) & ~(rng.integers(0, full + 1, size=G) &
                                                                                    rng.integers(0, full + 1, size=G))
    return cfg_words(inc, out, self_slot, present, group_commit)


def engine_with_cfg(rg, cfg, P, **kw):
    eng = rg.Engine(len(cfg), P, **kw)
    eng.load_column(rg.COL.CFG, cfg)
    return eng


def to_buffers(rg, eng, msgs):
    mb = rg.MsgBuffers(eng.n_groups, eng.n_slots, eng.stride)
    for k in ("m_index", "m_commit", "m_hint", "m_rs", "m_logterm", "m_flags"):
        getattr(mb, k)[...] = msgs[k]
    return mb


def first_bad(got, want):
    bad = np.nonzero(np.asarray(got) != np.asarray(want))
    return [tuple(int(i[k]) for i in bad) for k in range(min(3, len(bad[0])))]


# ---- votes and tally ----------------------------------------------------------------------------------------------------
def check_votes(rg, cfg, P, yes, no):
    eng = engine_with_cfg(rg, cfg, P)
    granted, rejected, res = eng.tally_votes(yes, no)
    res_plain = eng.vote_result(yes, no)
    eng.close()
    w_granted, w_rejected, w_res = M.tally_votes(cfg, yes, no)
    assert (res_plain == w_res).all(), ("rg_vote_result", first_bad(res_plain, w_res))
    assert (res == res_plain).all(), ("rg_tally_votes' result against rg_vote_result's", first_bad(res, res_plain))
    assert (granted == w_granted).all(), ("granted", first_bad(granted, w_granted))
    assert (rejected == w_rejected).all(), ("rejected", first_bad(rejected, w_rejected))
    return w_res


def test_votes_exhaustive_at_four_slots(rg):
    """Every (incoming, outgoing) in 16 x 16, two choices of (present, self) -- one with voters that have no Progress -- and
    every (yes, no) in 16 x 16, one group per case: 131 072 groups in one launch. The masks carry random bits at or above P on
    top; bits of slots that are not voters come with the enumeration."""
    inc, out, choice, yes, no = (a.reshape(-1) for a in np.indices((16, 16, 2, 16, 16)))
    present = np.where(choice == 0, inc | out | 1, 0b0101)  # choice 1: slots 1 and 3 never have a Progress
    self_slot = np.where(choice == 0, 0, 2)
    cfg = cfg_words(inc, out, self_slot, present)
    rng = np.random.default_rng(41)
    hi = rng.integers(0, 16, size=(2, len(cfg))) << 4
    res = check_votes(rg, cfg, 4, (yes | hi[0]).astype(np.uint8), (no | hi[1]).astype(np.uint8))
    assert [int((res == k).sum()) for k in range(3)] == [int((M.vote_result(cfg, yes, no) == k).sum()) for k in range(3)]
    assert all((res == k).sum() > 1000 for k in range(3))


@pytest.mark.parametrize("G,P", [(50000, 1), (50000, 2), (50000, 8), (1, 4), (65, 4)])
def test_votes_random(rg, G, P):
    rng = np.random.default_rng(4100 + 10 * P + G % 7)
    cfg = random_cfg(rng, G, P)
    yes, no = rng.integers(0, 256, size=(2, G), dtype=np.uint8)
    check_votes(rg, cfg, P, yes, no)


# ---- liveness -----------------------------------------------------------------------------------------------------------
def check_liveness(rg, cfg, P, pflags):
    eng = engine_with_cfg(rg, cfg, P)
    eng.load_column(rg.COL.PFLAGS, pflags)
    before = eng.read_column(rg.COL.PFLAGS)  # (the load re-derives the engine-owned RG_PF_PEND_* bits)
    assert ((before ^ pflags) & 0x3f == 0).all()
    for sweep in range(2):  # the second sweep meets the bits the first one left: only the self slot is still active
        got = eng.quorum_recently_active()
        after = eng.read_column(rg.COL.PFLAGS)
        want, want_after = M.quorum_recently_active(cfg, before)
        assert (got == want).all(), (sweep, "result", first_bad(got, want))
        assert (after == want_after).all(), (sweep, "flag rows", first_bad(after, want_after))
        before = after
    eng.close()
    return want


def test_liveness_exhaustive_at_four_slots(rg):
    """Every accepted (incoming, outgoing, present, self) at P = 4 with every recent_active pattern of the four slots: 262 144
    groups. Every other bit of every flag byte is random, the bytes of absent slots and of slots 4 to 7 included; the whole
    8-byte row must come back as the model's."""
    inc, out, present, self_slot, ra = (a.reshape(-1) for a in np.indices((16, 16, 16, 4, 16)))
    cfg = cfg_words(inc, out, self_slot, present)
    rng = np.random.default_rng(42)
    pf = rng.integers(0, 256, size=(len(cfg), 8), dtype=np.uint8)
    pf[:, :4] &= np.uint8(~M.PF_RECENT_ACTIVE & 0xff)
    for s in range(4):
        pf[:, s] |= (((ra >> s) & 1) * M.PF_RECENT_ACTIVE).astype(np.uint8)
    second = check_liveness(rg, cfg, 4, pf)
    assert 0 < second.sum() < len(cfg)


@pytest.mark.parametrize("G,P", [(50000, 8), (63, 3), (64, 3), (65, 3)])
def test_liveness_random(rg, G, P):
    rng = np.random.default_rng(4200 + G % 11)
    check_liveness(rg, random_cfg(rng, G, P), P, rng.integers(0, 256, size=(G, 8), dtype=np.uint8))


# ---- heartbeat commits --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", range(1, 9))
def test_heartbeat_commits_both_destinations(rg, P):
    """min(matched, committed) per slot with indices near 2**62, absent slots inside P, matched below / at / above the commit
    index. The host form and the device form; the device form writes the cells of groups 0 .. G-1 only (raftgroups.h)."""
    import torch
    rng = np.random.default_rng(4300 + P)
    G = 321  # two full blocks of 64 and a partial one
    st = O.alloc_state(G, P)
    st["cfg"][:] = random_cfg(rng, G, P)
    fuzz.random_state(rng, st, base=2 ** 62)
    present = (st["cfg"] >> 24) & 0xff
    has = np.stack([((present >> p) & 1) == 1 for p in range(P)])
    m, c = st["match"][:, :G], st["commit"][None, :]
    assert (has & (m < c)).any() and (has & (m == c)).any() and (has & (m > c)).any() and (P == 1 or (~has).any())
    assert int(st["commit"].min()) >= 2 ** 62 - 16
    want = M.heartbeat_commits(st["cfg"], st["match"], st["commit"])
    eng = rg.Engine(G, P)
    eng.load_state(st)
    assert eng.stride > G
    hb = eng.heartbeat_commits()
    assert (hb[:, :G] == want).all(), ("host form", first_bad(hb[:, :G], want))
    dev = torch.from_numpy(np.full((P, eng.stride), SENTINEL, dtype=np.uint64).view(np.int64)).cuda()
    assert eng.heartbeat_commits(dev_out=dev.data_ptr()) is None
    eng.sync()
    got = dev.cpu().numpy().view(np.uint64)
    assert (got[:, :G] == want).all(), ("device form", first_bad(got[:, :G], want))
    assert (got[:, G:] == SENTINEL).all(), "cells from G up to the stride are not the call's to write"
    eng.close()


# ---- censuses -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 3, 5, 8])
def test_msg_stats_against_the_model(rg, P):
    """rg_msg_stats' five counters on random and on garbage flag rows, G on either side of a wave (= a block) and past the cap
    of 1 024 blocks; self slots without a Progress, elections on own slots, REJECT without VALID. Flag bytes of slots at or
    above P stay zero (raftgroups.h: the census reads all 8 bytes of a group)."""
    import torch
    for G in (1, 63, 64, 65, 257, 65536 + 65):
        rng = np.random.default_rng(4400 + 13 * P + G % 17)
        st = O.alloc_state(G, P)
        st["cfg"][:] = random_cfg(rng, G, P)
        fuzz.random_state(rng, st)
        eng = engine_with_cfg(rg, st["cfg"], P)
        msgs = O.alloc_msgs(G, P)
        for kind in ("random", "garbage"):
            if kind == "random":
                fuzz.random_msgs(rng, st, msgs, reject_p=0.4, elect_p=0.3, elect_term=9)
            else:
                fuzz.garbage_msgs(rng, st, msgs)
            f = msgs["m_flags"]
            assert (f[:, P:] == 0).all()
            dev = torch.from_numpy(f.copy()).cuda()
            got = eng.msg_stats(dev.data_ptr())
            want = M.msg_stats(f, st["cfg"])
            assert [got[k] for k in ("valid", "rejects", "slots", "groups_with_events", "elections")] == want, (G, kind, got, want)
            if G > 65536:
                _, _, self_slot, present = M.cfg_fields(st["cfg"])
                own = f[np.arange(G), self_slot]
                tail = slice(65536, G)  # (only the second pass of the grid-stride loop reaches these)
                assert (f[tail] & 1).any() and want[4] > 0 and ((own & 2) != 0)[((present >> self_slot) & 1) == 0].any()
                if kind == "garbage":
                    assert ((f & 3) == 2).any(), "REJECT without VALID"
        eng.close()


def test_result_counts_past_the_grid_cap(rg):
    """rg_result_counts after a real tick with malformed messages at G = 131 072 + 65 (k_count_out: 2 048 blocks of 64 lanes, then
    the second pass of its grid-stride loop): both counts are the popcounts of RG_COL_OUT, and n_fault is not zero."""
    rng = np.random.default_rng(45)
    G, P = 131072 + 65, 3
    st = O.alloc_state(G, P)
    st["cfg"][:] = random_cfg(rng, G, P)
    fuzz.random_state(rng, st)
    eng = rg.Engine(G, P)
    eng.load_state(st)
    msgs = fuzz.random_msgs(rng, st, O.alloc_msgs(G, P), malformed_p=0.2)
    eng.tick(to_buffers(rg, eng, msgs))
    out = eng.read_column(rg.COL.OUT)
    want = M.result_counts(out)
    assert eng.result_counts() == want
    assert want[0] > 1000 and want[1] > 1000
    assert M.result_counts(out[131072:])[0] > 0 and M.result_counts(out[131072:])[1] > 0, "nothing to count in the second pass"
    eng.close()


# ---- the group-commit flag ----------------------------------------------------------------------------------------------
def flag_cases(group_commit):
    """P = 3: matched in {0..3}^3 x incoming x outgoing x present masks (x gids in {0, 1, 2}^3 with group commit on)."""
    dims = (4, 4, 4, 8, 8, 8) + ((3, 3, 3) if group_commit else ())
    ix = [a.reshape(-1) for a in np.indices(dims)]
    G = len(ix[0])
    stride = (G + 255) // 256 * 256
    match = np.zeros((3, stride), dtype=np.uint64)
    gid = np.zeros((3, stride), dtype=np.uint64)
    for s in range(3):
        match[s, :G] = ix[s]
        if group_commit:
            gid[s, :G] = ix[6 + s]
    cfg = cfg_words(ix[3], ix[4], np.zeros(G, dtype=np.int64), ix[5], group_commit)
    return cfg, match, gid


_flag_reference = {}


def flag_reference(group_commit):
    """The cases, the model's answer for every group and the oracle's for a sample -- computed once, shared, left unchanged."""
    if group_commit not in _flag_reference:
        cfg, match, gid = flag_cases(group_commit)
        G = len(cfg)
        mci, used = M.maximal_committed_index(cfg, match, gid)
        pick = np.arange(G) if G <= 40000 else np.random.default_rng(46).choice(G, size=24000, replace=False)
        pick = np.sort(pick)
        st = O.alloc_state(len(pick), 3)
        st["cfg"][:] = cfg[pick]
        st["match"][:, :len(pick)] = match[:, pick]
        st["gid"][:, :len(pick)] = gid[:, pick]
        st["next"][:, :len(pick)] = match[:, pick] + 1
        st["term_lo"][:] = 1
        st["term_hi"][:] = 3
        cl = O.Cluster(len(pick))
        cl.load_soa(st, term=2)
        want = [cl.mci(k) for k in range(len(pick))]
        assert (mci[pick] == np.array([w[0] for w in want], dtype=np.uint64)).all(), "model against the oracle: mci"
        assert (used[pick] == np.array([w[1] for w in want], dtype=bool)).all(), "model against the oracle: flag"
        _flag_reference[group_commit] = (cfg, match, gid, mci, used)
    return _flag_reference[group_commit]


@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("group_commit,variant", [(False, "DEFAULT"), (False, "LANE"), (False, "COOP"), (True, "DEFAULT"), (True, "LANE")])
def test_group_commit_flag_exhaustive_at_three_slots(rg, group_commit, variant, odd):
    """rg_maximal_committed_index and its used_group_commit flag for every enumerated group, at an even G and (the last group
    dropped) at an odd one, under every variant that can select a recompute kernel of its own. (The two-groups-per-lane kernel
    k_recompute2 is a build-time variant, RG_RECOMPUTE_X2, that the default build leaves out: there DEFAULT runs the kernel LANE
    runs. A build that turns it on meets its odd-G tail here, with and without the flag.)"""
    cfg, match, gid, mci, used = flag_reference(group_commit)
    G = len(cfg) - (1 if odd else 0)
    eng = rg.Engine(G, 3, variant=getattr(rg, "VARIANT_" + variant))
    stride = eng.stride
    eng.load_column(rg.COL.CFG, cfg[:G])
    eng.load_column(rg.COL.MATCH, np.ascontiguousarray(match[:, :stride]))
    eng.load_column(rg.COL.GID, np.ascontiguousarray(gid[:, :stride]))
    got, flag = eng.maximal_committed_index(with_flag=True)
    eng.close()
    assert (got == mci[:G]).all(), ("mci", first_bad(got, mci[:G]))
    assert (flag.astype(bool) == used[:G]).all(), ("used_group_commit", first_bad(flag.astype(bool), used[:G]))
    assert 0 < used[:G].sum() < G


# ---- host hints: a crafted tick whose rejects MUST be left to the host ---------------------------------------------------
# The log: a dummy entry at index 10 (term 1), entries 11..19 whose terms the device does not hold, the first known run from 20
# (term 5), the leader's own entries 30..40 (term 6). Every follower sits in Probe (or Snapshot) at next = 36; a reject of
# index 35 with reject_hint 15 and log_term 3 makes find_conflict_by_term ask for term(15): dummy_term <= 3 < 5, only the host's
# log can answer. In the host's (the oracle's) complete log the gap is 11..13 at term 2 and 14..19 at term 4: the answer is 13.
M_INDEX, M_HINT, M_LOGTERM, NEXT0 = 35, 15, 3, 36
HINT_FLAGS = hosthints.MF_VALID | hosthints.MF_REJECT | hosthints.MF_HAS_LOGTERM
DECOYS = ("log_term_5", "stale_index", "snapshot_request", "no_log_term")  # rejects the tick answers or drops itself


def crafted_tick(G, P, hinted, decoys=(), absent_last=(), paused=(), snapshot=()):
    """hinted: {group: slot mask}; decoys: [(group, slot, kind)]; absent_last: groups whose last slot has no Progress;
    paused / snapshot: (group, slot) cells in Probe + paused / in Snapshot. -> (engine state, the oracle's state, msgs)."""
    st = O.add_term_table(O.alloc_state(G, P))
    full = (1 << P) - 1
    present = np.full(G, full, dtype=np.int64)
    present[list(absent_last)] &= ~(1 << (P - 1))
    st["cfg"][:] = cfg_words(np.full(G, full), np.zeros(G, dtype=np.int64), np.zeros(G, dtype=np.int64), present)
    st["term_lo"][:], st["term_hi"][:], st["commit"][:], st["cur_term"][:] = 30, 40, 25, 6
    st["dummy_index"][:], st["dummy_term"][:] = 10, 1
    st["run_first"][0, :G], st["run_term"][0, :G] = 20, 5
    st["match"][0, :G], st["next"][0, :G], st["pr_commit"][0, :G] = 40, 41, 25
    st["pflags"][:, 0] = O.REPLICATE | M.PF_RECENT_ACTIVE
    st["match"][1:, :G], st["next"][1:, :G], st["pr_commit"][1:, :G] = 12, NEXT0, 12
    st["pflags"][:, 1:P] = O.PROBE
    for g, s in paused:
        st["pflags"][g, s] |= M.PF_PAUSED
    for g, s in snapshot:
        st["pflags"][g, s] = O.SNAPSHOT
        st["pend_snap"][s, g] = 22
    for s in range(P):
        gone = ((present >> s) & 1) == 0
        for k in ("match", "next", "pr_commit", "pend_snap"):
            st[k][s, :G][gone] = 0
        st["pflags"][gone, s] = 0
    host = hosthints._copy(st)
    host["run_first"][:3, :G] = np.array([11, 14, 20], dtype=np.uint64)[:, None]
    host["run_term"][:3, :G] = np.array([2, 4, 5], dtype=np.uint64)[:, None]
    msgs = O.alloc_msgs(G, P)

    def reject(g, s, flags=HINT_FLAGS, index=M_INDEX, log_term=M_LOGTERM, rs=0):
        msgs["m_flags"][g, s] = flags
        msgs["m_index"][s, g], msgs["m_hint"][s, g], msgs["m_logterm"][s, g] = index, M_HINT, log_term
        msgs["m_commit"][s, g], msgs["m_rs"][s, g] = 12, rs

    for g, mask in hinted.items():
        for s in range(1, P):
            if (mask >> s) & 1:
                reject(g, s)
    for g, s, kind in decoys:
        assert g not in hinted
        if kind == "log_term_5":
            reject(g, s, log_term=5)
        elif kind == "stale_index":
            reject(g, s, index=30)
        elif kind == "snapshot_request":
            reject(g, s, flags=HINT_FLAGS | hosthints.MF_HAS_RS, rs=7)
        else:
            reject(g, s, flags=hosthints.MF_VALID | hosthints.MF_REJECT, log_term=0)
    return st, host, msgs


def host_cluster(host, max_inflight=0):
    cl = O.Cluster(host["n_groups"])
    cl.load_soa(host, term=6, max_inflight=max_inflight)
    return cl


def host_answer(cl, g):
    return int(O.lib().ro_log_find_conflict_by_term(cl.h, g, M_HINT, M_LOGTERM))


def all_columns(rg, eng):
    return {name: eng.read_column(col) for col, name in enumerate(rg.COL.NAMES)}


def model_answers(cols, recs, device_inflights=False):
    """rg_resolve_host_hints over numpy copies of the columns (changed in place), one record after the other: a record answers
    bit `slot` of its group's RG_COL_HOST_HINT byte if the group carries RG_OUT_HOST_HINT, the slot has a Progress and the
    bit is still set; the cell takes the reject (quorum_model.resolved_reject), the result word RG_OUT_SEND_APPEND(slot) where
    it applied, and RG_OUT_HOST_HINT falls with the group's last bit. -> ({(group, slot): applied}, groups released)."""
    taken, released = {}, set()
    for g, index, hint, s, _ in recs:
        g, s = int(g), int(s)
        if not (int(cols["cfg"][g]) >> (24 + s)) & 1 or not int(cols["out"][g]) & HH or not (int(cols["host_hint"][g]) >> s) & 1:
            continue
        ok, nxt, psnap, pf = M.resolved_reject([cols["match"][s, g]], [cols["next"][s, g]], [cols["pend_snap"][s, g]],
                                               [cols["pflags"][g, s]], [index], [hint], device_inflights)
        cols["next"][s, g], cols["pend_snap"][s, g], cols["pflags"][g, s] = nxt[0], psnap[0], pf[0]
        cols["host_hint"][g] &= np.uint8(~(1 << s) & 0xff)
        if ok[0]:
            cols["out"][g] |= np.uint32(1 << (8 + s))
        if cols["host_hint"][g] == 0:
            cols["out"][g] &= np.uint32(~HH & 0xffffffff)
            released.add(g)
        taken[(g, s)] = bool(ok[0])
    return taken, released


def assert_columns(rg, eng, want, what, names=None):
    got = all_columns(rg, eng)
    for name in names or rg.COL.NAMES:
        assert (got[name] == want[name]).all(), (what, name, first_bad(got[name], want[name]))


def list_layout(G):
    """Where the list test puts its hints: a whole aligned quadruple (one 32-bit word of RG_COL_HOST_HINT), the first and the
    last lane of a wave, the last group of the shard (in a partial block), and groups that only the second pass of the
    grid-stride loops reaches."""
    hinted = {8: 0b010, 9: 0b100, 10: 0b110, 11: 0b010, 64: 0b110, 127: 0b100, G - 1: 0b110, 131072: 0b010, 131072 + 7: 0b100}
    decoys = [(12 + k, 1 + k % 2, kind) for k, kind in enumerate(DECOYS)] + [(131072 + 20 + k, 1, kind) for k, kind in enumerate(DECOYS)]
    return hinted, decoys


def test_host_hint_list_layouts_and_caps(rg):
    """rg_host_hints at G = 131 072 + 65 (past k_host_hints' 2 048 blocks of 64 lanes), P = 3, on a crafted tick whose hinted
    groups are laid out on purpose; the list against the model and the CPU restatement, *n exact, every `cap`. The engine has
    device Inflights, so the HOST_HINT census of k_count_out gates the next tick: it must still refuse while only groups of the
    second grid-stride pass wait."""
    from raft_rs_amd.engine import ERR
    G, P = 131072 + 65, 3
    hinted, decoys = list_layout(G)
    st, host, msgs = crafted_tick(G, P, hinted, decoys, paused=[(8, 1), (131072, 1)])
    cl = host_cluster(host)
    assert hosthints.expected(cl, st, st, msgs, table_runs=1) == hinted, "the CPU restatement must name exactly the crafted rejects"
    eng = rg.Engine(G, P, max_inflight=2)
    eng.load_state(st)
    mb = to_buffers(rg, eng, msgs)
    eng.tick(mb)
    out, hh = eng.read_column(rg.COL.OUT), eng.read_column(rg.COL.HOST_HINT)
    assert M.host_hints(out, hh) == hinted
    n = len(hinted)
    listed = eng.host_hints()
    assert len(listed) == n and {int(r["group"]): int(r["slot_mask"]) for r in listed} == hinted and (listed["reserved"] == 0).all()
    blank = np.frombuffer(bytes([0xA5]) * 16, dtype=listed.dtype)[0]
    for cap in (0, 1, n - 1, n + 7):
        items, count = eng.host_hints(cap=cap)
        assert count == n, (cap, count)
        k = min(cap, n)
        assert len(items) == cap and (items[k:] == blank).all(), (cap, "the sentinel behind the written entries")
        written = [(int(r["group"]), int(r["slot_mask"])) for r in items[:k]]
        assert len(set(written)) == k and all(hinted.get(g) == m for g, m in written), (cap, written)
    # the groups below the grid cap are answered; those only the second pass counts still hold the next step back
    recs = [(g, M_INDEX, host_answer(cl, g), s, 0) for g, mask in hinted.items() for s in range(P) if (mask >> s) & 1]
    assert eng.resolve_host_hints([r for r in recs if r[0] < 131072]).all()
    with pytest.raises(rg.EngineError) as e:
        eng.tick(mb)
    assert e.value.code == ERR["STATE"] and "3 group(s)" in str(e.value), str(e.value)
    assert {int(r["group"]) for r in eng.host_hints()} == {131072, 131072 + 7, G - 1}
    assert eng.resolve_host_hints([r for r in recs if r[0] >= 131072]).all()
    assert len(eng.host_hints()) == 0 and eng.host_hints(cap=3)[1] == 0
    mb.clear()
    eng.tick(mb)  # nothing waits any more
    eng.close()


def answers_layout(G, P):
    """G = 4 096 + 5, P = 5: every third group is hinted, with one to four slots; some followers paused, some in Snapshot, some
    groups without a Progress in the last slot."""
    masks = (0b00110, 0b11110, 0b01010, 0b10000, 0b11100, 0b00010)
    absent_last = [g for g in range(G) if g % 5 == 1]
    hinted = {}
    for k, g in enumerate(list(range(0, G, 3)) + [G - 1]):
        m = masks[k % len(masks)] & (~(1 << (P - 1)) if g % 5 == 1 else 0xff)
        if m:
            hinted[g] = m
    for g in (8, 9, 10, 11):  # one aligned quadruple: four bytes of one word, several slots each
        hinted[g] = 0b01110
    paused = [(g, 1 + g % (P - 1)) for g in range(0, G, 2)]
    snapshot = [(g, 1 + (g + 1) % (P - 1)) for g in range(0, G, 7)]
    paused = [c for c in paused if c not in set(snapshot)]
    decoys = [(g, 1 + g % 3, DECOYS[g % 4]) for g in range(1, G, 31) if g not in hinted]
    return hinted, decoys, absent_last, paused, snapshot


def answered_engine(rg, max_inflight=0):
    """The crafted tick on the smaller shard -> (engine, host cluster, msgs, buffers, hinted, the records that answer it)."""
    G, P = 4096 + 5, 5
    hinted, decoys, absent_last, paused, snapshot = answers_layout(G, P)
    if max_inflight:
        snapshot = []
    st, host, msgs = crafted_tick(G, P, hinted, decoys, absent_last, paused, snapshot)
    cl = host_cluster(host, max_inflight)
    assert hosthints.expected(cl, st, st, msgs, table_runs=1) == hinted
    eng = rg.Engine(G, P, max_inflight=max_inflight)
    eng.load_state(st)
    mb = to_buffers(rg, eng, msgs)
    eng.tick(mb)
    assert M.host_hints(eng.read_column(rg.COL.OUT), eng.read_column(rg.COL.HOST_HINT)) == hinted
    recs = [(g, M_INDEX, host_answer(cl, g), s, 0) for g, mask in hinted.items() for s in range(P) if (mask >> s) & 1]
    assert len(recs) > 2000 and all(r[2] == 13 for r in recs)
    return eng, cl, msgs, mb, hinted, recs


def resolve_and_compare(rg, eng, cols, recs, what, device_inflights=False, names=None):
    """One rg_resolve_host_hints call against the model; returns (applied u8[n], {(g, s): applied} of the model, released)."""
    taken, released = model_answers(cols, recs, device_inflights)
    applied = eng.resolve_host_hints(recs)
    assert_columns(rg, eng, cols, what, names)
    return applied, taken, released


@pytest.mark.parametrize("scenario", ["one_call", "split", "duplicates", "not_waiting", "stale_index"])
def test_host_hint_answers(rg, scenario):
    """rg_resolve_host_hints (k_resolve_apply, one lane per record) after the crafted tick: RG_COL_NEXT, _PFLAGS, _PEND_SNAP, _OUT and
    _HOST_HINT against the model after every call, every other column unchanged.
    (Not told apart by this or any test: `last` of rg_resolve_hint_at read back from the byte after the clear instead of derived
    from the value the atomic returned. Of the lanes that answer one group at least one then still sees the byte empty, the bit
    falls once or twice to the same value and the host sorts the released groups uniquely: no result of the call differs.)"""
    eng, cl, msgs, mb, hinted, recs = answered_engine(rg)
    rng = np.random.default_rng(47)
    cols = all_columns(rg, eng)
    before = {k: v.copy() for k, v in cols.items()}
    G, P = eng.n_groups, eng.n_slots
    if scenario == "one_call":
        # every record in one call, shuffled: a group's slots land in different workgroups of 256 records; the hints vary so
        # that next becomes hint + 1, the rejected index, and 1
        order = rng.permutation(len(recs))
        recs = [(recs[i][0], M_INDEX, (13, 50, 0)[i % 3], recs[i][3], 0) for i in order]
        slots_at = {}
        for i, r in enumerate(recs):
            slots_at.setdefault(r[0], set()).add(i // 256)
        assert sum(len(v) > 1 for v in slots_at.values()) > 500
        applied, taken, released = resolve_and_compare(rg, eng, cols, recs, scenario)
        assert applied.all() and all(taken.values()) and released == set(hinted)
        assert {int(x) for x in np.unique(cols["next"][1:, list(hinted)])} >= {1, 14, M_INDEX}
        assert not (cols["out"] & HH).any() and len(eng.host_hints()) == 0
    elif scenario == "split":
        first, rest, have = [], [], set()
        for r in recs:
            (rest if r[0] in have else first).append(r)
            have.add(r[0])
        applied, _, released = resolve_and_compare(rg, eng, cols, first, "split: first slots")
        waiting = {r[0] for r in rest}
        assert applied.all() and released == set(hinted) - waiting and len(waiting) > 500
        assert {int(g) for g in np.nonzero(cols["out"] & HH)[0]} == waiting
        assert {int(r["group"]): int(r["slot_mask"]) for r in eng.host_hints()} == M.host_hints(cols["out"], cols["host_hint"])
        middle = [r for r in rest if r[3] != max(s for s in range(P) if (hinted[r[0]] >> s) & 1)]
        mid = set(middle)
        last = [r for r in rest if r not in mid]
        applied, _, released = resolve_and_compare(rg, eng, cols, middle, "split: middle slots")
        assert applied.all() and released == set() and {int(g) for g in np.nonzero(cols["out"] & HH)[0]} == waiting
        applied, _, released = resolve_and_compare(rg, eng, cols, last, "split: last slots")
        assert applied.all() and released == waiting and not (cols["out"] & HH).any()
        assert (cols["host_hint"][list(hinted)] == 0).all()
    elif scenario == "duplicates":
        stale = {(r[0], r[3]) for r in recs[::5]}  # some pairs of copies carry a stale index: neither copy applies
        recs = [(r[0], M_INDEX - 2 if (r[0], r[3]) in stale else M_INDEX, r[2], r[3], 0) for r in recs]
        both = [recs[i] for i in rng.permutation(np.repeat(np.arange(len(recs)), 2))]
        applied, taken, released = resolve_and_compare(rg, eng, cols, both, scenario)
        per_cell = {}
        for r, a in zip(both, applied):
            per_cell.setdefault((r[0], r[3]), []).append(int(a))
        assert all(len(v) == 2 for v in per_cell.values())
        wrong = [(k, v) for k, v in per_cell.items() if sum(v) != (1 if taken[k] else 0)]
        assert not wrong, ("exactly one of two copies applies where the model applies", wrong[:5])
        assert sum(taken.values()) == len(recs) - len(stale) and released == set(hinted)
    elif scenario == "not_waiting":
        absent = [g for g in hinted if not (int(cols["cfg"][g]) >> (24 + P - 1)) & 1]
        noise = [(g, M_INDEX, 13, s, 0) for g, mask in hinted.items() for s in range(P) if not (mask >> s) & 1]  # slots not waiting
        noise += [(g, M_INDEX, 13, P - 1, 0) for g in absent]                                                     # no Progress
        noise += [(g, M_INDEX, 13, 1 + g % (P - 1), 0) for g in range(G) if g not in hinted]                      # groups without the bit
        assert len(absent) > 100 and len(noise) > 5000
        applied, taken, released = resolve_and_compare(rg, eng, cols, [noise[i] for i in rng.permutation(len(noise))], scenario)
        assert not applied.any() and not taken and not released
        assert all((cols[k] == before[k]).all() for k in cols)
        # ... and the waiting slots are still waiting: the real answers apply afterwards, mixed with the noise
        mixed = recs + noise
        applied, taken, released = resolve_and_compare(rg, eng, cols, [mixed[i] for i in rng.permutation(len(mixed))], "noise + answers")
        assert int(applied.sum()) == len(recs) and released == set(hinted)
    else:
        # a stale Message.index: maybe_decr_to returns false and nothing of the Progress moves, but the slot is released
        recs = [(r[0], M_INDEX + (1 if i % 2 else -3), r[2], r[3], 0) for i, r in enumerate(recs)]
        applied, taken, released = resolve_and_compare(rg, eng, cols, [recs[i] for i in rng.permutation(len(recs))], scenario)
        assert not applied.any() and len(taken) == len(recs) and not any(taken.values()) and released == set(hinted)
        for k in ("next", "pflags", "pend_snap"):
            assert (cols[k] == before[k]).all()
        assert not (cols["out"] & HH).any() and ((cols["out"] ^ before["out"]) & ~np.uint32(HH) == 0).all()
    for name in cols:  # whatever the scenario: only these five columns may have moved
        if name not in ("next", "pflags", "pend_snap", "out", "host_hint"):
            assert (cols[name] == before[name]).all(), name
    eng.close()


def test_host_hint_answers_release_the_send_stage(rg):
    """The same tick on an engine with device Inflights (max_inflight = 4): the next tick is refused with RG_ERR_STATE until the
    LAST answer, and the work items of the released groups are the oracle's send stage for the tick."""
    from raft_rs_amd.engine import ERR
    eng, cl, msgs, mb, hinted, recs = answered_engine(rg, max_inflight=4)
    cl.set_own_inflights(True)
    G, P = eng.n_groups, eng.n_slots
    eng.send_appends(0)  # the stage of the tick: it holds the hinted groups' requests back
    gout = np.zeros(G, dtype=np.uint32)
    cl.tick_soa(msgs, gout)
    early = eng.send_items()
    assert len(early) > 0 and not set(hinted) & {int(g) for g in early["group"]}
    cols = all_columns(rg, eng)
    first, rest, have = [], [], set()
    for r in recs:
        (rest if r[0] in have else first).append(r)
        have.add(r[0])
    last_one, rest = rest[-1:], rest[:-1]
    for part, what in ((first, "first slots"), (rest, "all but one"), (last_one, "the last answer")):
        seen = all_columns(rg, eng)
        with pytest.raises(rg.EngineError) as e:
            eng.tick(mb)
        assert e.value.code == ERR["STATE"] and "rg_resolve_host_hints" in str(e.value), what
        assert_columns(rg, eng, seen, "a refused tick changes nothing")
        # (the stage has run: this call also serves the released groups' sends, which move their Progress -- the whole state
        # is compared with the oracle's below, the result words and the hint bytes here)
        applied, _, _ = resolve_and_compare(rg, eng, cols, part, what, device_inflights=True, names=("out", "host_hint"))
        assert applied.all()
    assert (cols["out"] == gout).all(), first_bad(cols["out"], gout)
    got = eng.send_items()
    items = sendstage.compare_items(got, cl.send_stage_soa(gout, 0))
    late = [k for k in items if k[0] in hinted]
    assert len(late) >= len(recs), "every answered reject sends an append (raft.rs:1719)"
    host = hosthints._copy({k: v for k, v in cols.items() if k in fuzz.STATE_KEYS})
    host.update(n_groups=G, n_slots=P, stride=eng.stride)
    cl.store_soa(host)
    diffs = fuzz.diff_states(host, eng.read_state(), G, P)
    assert not diffs, diffs[:5]
    mb.clear()
    eng.tick(mb)  # accepted again
    eng.close()
