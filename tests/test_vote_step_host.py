"""CPU only: the dense vote step. (1) tests/vote_step_model.py restates Raft::step for the two vote kinds with its lines named and
composes the other stages' models; its Leader carries a real election_elapsed, and the lease formula evaluated on it equals
check_quorum for every value a leader can hold -- the observation the kernel relies on; (2) the arithmetic of csrc/rg_vote.h -- what
the kernels run -- is compiled for the HOST with g++ (tests/host_check/vote_twin.cpp, a stand-alone program) and diffed against the
model over the header's case table and over seeded random cases, then once more under AddressSanitizer + UBSan, run directly;
(3) what the seed covers is asserted from the model alone; (4) the Leader row the golden data lists as skipped is replayed;
(5) every new name is declared, exported and bound, the three older headers are what they were, the refusals are host checks;
(6) the kernels carry no scratch and no LDS (tools/kernel_resources.py).

Citations: pingcap/raft-rs v0.6.0."""
import copy
import ctypes
import json
import os
import random
import re
import shutil
import subprocess
import sys

import pytest

import follower_model as F
import gate_model as G
import handoff_model as H
import lead_clock_model as L
import vote_step_model as V

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_NAMES = ("rgv_vote_version", "rgv_follow_vote_device", "rgv_follow_vote", "rgv_follow_vote_counts")
SEED, CASES = 41, 20000
M64 = (1 << 64) - 1
EMPTY = {"committed": 0, "last_index": 0, "dummy_index": 0, "dummy_term": 0, "runs": []}


def build_twin(tmp_path, name, extra):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build the host twin")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, os.path.join(HERE, "host_check", "vote_twin.cpp"), "-o", exe])
    return exe


def state_words(c):
    runs = c["runs"]
    assert len(runs) <= H.FOLLOW_RUNS
    pad = [0] * (H.FOLLOW_RUNS - len(runs))
    return [c["committed"], c["last_index"], c["dummy_index"], c["dummy_term"], len(runs)] + [r[0] for r in runs] + pad + [r[1] for r in runs] + pad


def clock_word(node):
    return node.elapsed | int(node.promotable) << 15 | node.timeout << 16


def case_line(cfg, node, lead, clock, m, has_lead):
    d = lead if lead is not None else H.fresh_lead(3, 0)
    words = [int(has_lead), int(clock is not None), m.kind, m.term, m.frm, m.index, m.log_term, m.commit, m.commit_term, m.priority & M64, int(m.force),
             cfg.flags, cfg.election_tick, cfg.min_timeout, cfg.max_timeout, cfg.seed, node.group,
             node.term, node.lead, node.vote, node.priority & M64, node.role, clock_word(node), getattr(node, "self_id", 0),
             L.cell_word(clock) if clock is not None else 0, clock["tag"] if clock is not None else 0, d.get("cfg", 0),
             d["commit"], d["term_lo"], d["term_hi"], d["cur_term"], d["dummy_index"], d["dummy_term"], d["run_count"]] + list(d["run_first"]) + list(d["run_term"])
    return "V " + " ".join("%d" % w for w in words + state_words(node.log.canonical()))


def expected(cfg, node, lead, clock, m, has_lead):
    """The model's step on copies -> (the twin's output words, answer, deposed)"""
    n, d, k = copy.deepcopy(node), (H.copy_lead(lead) if lead is not None else None), (L.copy_group(clock) if clock is not None else None)
    a, deposed = V.step(cfg, cfg.election_tick, n, d if has_lead else None, k, None, m)
    words = list(a) + [int(deposed), n.term, n.lead, n.vote, n.role, clock_word(n), L.cell_word(k) if k is not None else 0, k["tag"] if k is not None else 0,
                       (d or {}).get("cfg", 0)] + state_words(n.log.canonical())
    if not deposed and has_lead and V.win_state(node):  # nothing of a led group changes unless it is deposed
        assert (n.soft(), d, k) == (node.soft(), lead, clock)
    return words, a, deposed


def run_twin(exe, cases):
    lines = [case_line(*c) for c in cases]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    got = out.stdout.split("\n")[:-1]
    assert len(got) == len(cases)
    for line, c in zip(got, cases):
        want = expected(*c)[0]
        w = line.split()
        assert w[0] == "V" and [int(x) for x in w[1:]] == want, (line, want, case_line(*c))


def random_cases(seed, n):
    rng = random.Random(seed)
    out = []
    for k in range(n):
        cfg = G.Config(5, flags=rng.choice((0, G.CHECK_QUORUM, G.PRE_VOTE, G.CHECK_QUORUM | G.PRE_VOTE)), seed=9)
        led, node, lead, clock, m = V.random_case(rng, cfg, k % 600)
        if lead is not None:
            lead["cfg"] = lead.get("cfg", 0)
        has_lead = led or rng.random() < 0.1
        if has_lead and lead is None:  # a dev_lead cell that names a group the arena does not hold the win state for
            lead = H.fresh_lead(3, 0)
        out.append((cfg, node, lead, clock, m, has_lead))
    return out


def table():
    return [(cfg, node, lead, clock, m, True) for cfg, node, lead, clock, m in V.table_cases()]


def test_model_cites_the_reference_lines_and_composes_the_other_models():
    src = open(os.path.join(HERE, "vote_step_model.py")).read()
    for cite in ("raft.rs:1282-1411", ":1285-1317", ":1289-1291", ":1319-1330", ":1346", ":1349-1410", "raft.rs:1418-1461", ":1420-1426", "raft.rs:2126-2164", ":2131",
                 "raft.rs:1051-1079", "raft.rs:942-971"):
        assert cite in src, cite
    for mod in ("gate_model", "handoff_model", "lead_clock_model", "term_gate_model", "readonly_model", "follower_model"):
        assert "import %s" % mod in src
    for theirs in ("def demote", "def become_follower", "def reset", "def abort_leader_transfer", "def draw", "def lead_stop", "def _maybe_commit_by_vote", "rg_vote_"):
        assert theirs not in src, theirs


def test_a_leaders_lease_is_check_quorum_alone():
    """The observation: for every election_elapsed a leader can hold, [0, election_tick), and both CHECK_QUORUM settings the lease
    formula of raft.rs:1289-1291, evaluated as written on the model's Leader, equals check_quorum -- and lead_clock_model's tick never
    leaves a led group at or beyond election_tick. The request of a higher term is IGNORED exactly under CHECK_QUORUM without FORCE."""
    for c in L.SWEEP_CONFIGS:
        g = L.new_group(3, L.cfg_word((0, 1, 2), self_slot=0), pflags=L.flags_of((0, 1, 2)))
        for _ in range(min(3 * c.election_tick, 200)):
            L.tick(c, g)
            assert not g["led"] or g["el"] < c.election_tick
    for flags in (0, G.CHECK_QUORUM):
        cfg = G.Config(7, flags=flags, seed=3)
        for el in range(cfg.election_tick):
            assert V.in_lease(cfg.check_quorum, 3, el, cfg.election_tick) == cfg.check_quorum
            for force in (False, True):
                for kind in (G.VOTE, G.PREVOTE):
                    _, node, lead, clock, _ = V.table_cases((flags,))[0]
                    clock["el"] = el
                    a, deposed = V.step_leader(cfg, cfg.election_tick, node, lead, clock, None, G.Msg(kind, 9, 12, index=7, log_term=6, force=force))
                    assert (a[1] == G.G_IGNORED) == (cfg.check_quorum and not force), (flags, el, force, kind, a)
                    assert deposed == (a[1] != G.G_IGNORED and kind == G.VOTE)


def test_the_table_rows_are_what_the_header_says():
    """Every row of the header's case table on the model: who is IGNORED, who is answered, who is deposed, and that nothing changes
    unless the group is deposed (asserted in expected())."""
    seen = set()
    for cfg, node, lead, clock, m, _ in table():
        words, a, deposed = expected(cfg, node, lead, clock, m, True)
        rel = "<" if m.term < 6 else "=" if m.term == 6 else ">"
        seen.add((rel, m.kind, a[1], deposed))
        assert a[0] == F.NONE and a[2] & V.EV_LED
        if rel == "<":
            assert a[1] == (G.G_PREVOTE_LOW if m.kind == G.PREVOTE else G.G_IGNORED) and a[3] == 6 and not deposed
        elif rel == "=":
            assert (a[1], a[3], a[4], a[5], deposed) == (G.G_VOTE_REJECT, 6, 5, 6, False)  # commit_info() of the leader's log: (5, term 6)
        elif cfg.check_quorum and not m.force:
            assert a[1] == G.G_IGNORED and not deposed
        elif m.kind == G.PREVOTE:
            grant = m.index >= 7 and (m.index > 7 or 1 <= m.priority)
            assert (a[1], a[3], deposed) == ((G.G_VOTE_GRANT, m.term, False) if grant else (G.G_VOTE_REJECT, 6, False))
        else:
            grant = m.index >= 7 and (m.index > 7 or 1 <= m.priority)
            assert deposed and a[1] == (G.G_VOTE_GRANT if grant else G.G_VOTE_REJECT) and a[3] == m.term
            assert a[2] & (G.EV_HARD_STATE | G.EV_LEADER_CHANGED | V.EV_DEPOSED) == G.EV_HARD_STATE | G.EV_LEADER_CHANGED | V.EV_DEPOSED
            assert bool(a[2] & V.EV_TRANSFER_ABORTED) == bool(lead["cfg"] >> 20 & 0xF)
            # the soft cells: term = m.term, vote = from where granted, leader_id 0, election_elapsed 0; the clock cell stopped
            assert words[8:12] == [m.term, 0, m.frm if grant else 0, G.FOLLOWER] and words[12] & 0x7FFF == 0 and words[13] >> 31 == 1
            assert words[16] == (6 if not grant else 5)  # a reject ran maybe_commit_by_vote(6, 6); a grant left the commit alone
    assert len(seen) >= 10, seen


def test_the_seed_covers_every_outcome_from_the_model_alone():
    cov = {}
    for cfg, node, lead, clock, m, has_lead in random_cases(SEED, CASES):
        led = has_lead and V.win_state(node)
        _, a, deposed = expected(cfg, node, lead, clock, m, has_lead)
        for key in ((led, "gate", a[1]), (led, "status", a[0]), ("deposed", deposed), ("status", a[0])):
            cov[key] = cov.get(key, 0) + 1
    for led in (True, False):
        for gate in (G.G_IGNORED, G.G_PREVOTE_LOW, G.G_VOTE_GRANT, G.G_VOTE_REJECT):
            assert cov.get((led, "gate", gate), 0) >= 200, (led, gate, cov)
    assert cov.get(("deposed", True), 0) >= 200 and cov.get(("status", F.HOST), 0) >= 20, cov
    assert cov.get((True, "status", F.HOST), 0) >= 5 and cov.get((True, "status", F.FAULT), 0) >= 200, cov  # ... the led class has both too


def test_host_twin_matches_the_model(tmp_path):
    exe = build_twin(tmp_path, "vote_twin", [])
    run_twin(exe, table())
    run_twin(exe, random_cases(SEED, CASES))


def test_host_twin_is_clean_under_asan_and_ubsan(tmp_path):
    """The same program, -fsanitize=address,undefined -fno-sanitize-recover=all, run directly (a stand-alone executable)."""
    exe = build_twin(tmp_path, "vote_twin_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    run_twin(exe, table())
    run_twin(exe, random_cases(SEED + 1, 4000))


def golden_leader(t, state, vote_for, log_term):
    """The Leader row of test_recv_msg_request_vote_for_type as the engine holds it: the log [(2, 1), (2, 2)] is one older run below an
    EMPTY current range, at term = max(last_term, log_term)."""
    term = max(t["log"][-1][0], log_term)
    lead = H.fresh_lead(3, L.cfg_word((0, 1, 2), self_slot=0))
    lead.update(commit=0, term_lo=len(t["log"]) + 1, term_hi=len(t["log"]), cur_term=term, dummy_index=0, dummy_term=0, run_count=1,
                run_first=[1] + [0] * (H.TERM_RUNS - 1), run_term=[t["log"][0][0]] + [0] * (H.TERM_RUNS - 1))
    cfg = G.Config(t["constants"]["election_tick"])
    node = G.Node(cfg, 0)
    node.load(term, vote_for, vote_for, 0, G.FOLLOWER, 0, 0, True)
    node.self_id = vote_for
    return cfg, node, lead, L.new_group(3, lead["cfg"], cur_term=term), term


def test_golden_leader_row_is_a_reject(tmp_path):
    """tests/golden/vote_gate.json, RECV_MSG_REQUEST_VOTE: the rows listed under skipped_leader_rows (row 18, the Leader), for
    MsgRequestVote and MsgRequestPreVote: reject, at the leader's term, nothing changes."""
    t = json.load(open(os.path.join(HERE, "golden", "vote_gate.json")))["RECV_MSG_REQUEST_VOTE"]
    assert t["skipped_leader_rows"] == [18]
    cases = []
    for k in t["skipped_leader_rows"]:
        state, index, log_term, vote_for, w_reject = t["rows"][k]
        assert state == 3 and w_reject
        for kind in (G.VOTE, G.PREVOTE):
            cfg, node, lead, clock, term = golden_leader(t, state, vote_for, log_term)
            m = G.Msg(kind, term, t["constants"]["from"], index=index, log_term=log_term)
            _, a, deposed = expected(cfg, node, lead, clock, m, True)
            assert (a[0], a[1], a[3], deposed) == (F.NONE, G.G_VOTE_REJECT, term, False), (kind, a)
            cases.append((cfg, node, lead, clock, m, True))
    run_twin(build_twin(tmp_path, "vote_twin_gold", []), cases)


def test_kernels_carry_no_scratch_and_no_lds():
    """tools/kernel_resources.py over ext_vote.hip: exactly k_vote_dense and k_vote_list, both index widths."""
    from raft_rs_amd import build as engine_build
    engine_build.hipcc()  # (raises where there is no hipcc: the engine is built with it)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--src=raft_rs_amd/csrc/ext_vote.hip"], cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines()[1:]:
        m = re.match(r"(\S.*?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)$", line)
        if m:
            rows[m.group(1)] = (int(m.group(5)), int(m.group(6)))
    want = sorted(name + "<unsigned %s>" % w for name in ("k_vote_dense", "k_vote_list") for w in ("int", "long"))
    assert sorted(rows) == want, (sorted(rows), out.stderr[-1000:])  # ... and the unit instantiates none of the term gate's kernels
    for k, (scratch, lds) in rows.items():
        print(k, scratch, lds)
        assert scratch == 0 and lds == 0, (k, scratch, lds)


def test_every_new_name_is_declared_exported_and_bound(rg):
    """include/raftgroups_vote.h: every function it declares is exported (as rgv_*, nothing else with that prefix) and bound, in
    Python and in the generated bindings/raftgroups_vote.rs with the header's arity; the three older headers, their versions and
    their export sets are what they were."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_bindings
    from raft_rs_amd import engine as E
    hdr = open(os.path.join(ROOT, "include", "raftgroups_vote.h"), encoding="utf-8").read()
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(rgv_\w+)\s*\([^()]*\)\s*;", plain))
    assert declared == set(NEW_NAMES)
    assert not re.findall(r"\b(rg[xt]?_\w+)\s*\([^()]*\)\s*;", plain)  # ... and it declares no rg_* / rgx_* / rgt_* function
    assert '#include "raftgroups_term.h"' in hdr and "SUPERSEDES" in hdr
    older = {k: open(os.path.join(ROOT, "include", k), encoding="utf-8").read() for k in ("raftgroups.h", "raftgroups_lead.h", "raftgroups_term.h")}
    assert all("rgv_" not in v and "RGV_" not in v for v in older.values())
    assert "#define RG_ABI_VERSION 12u" in older["raftgroups.h"] and "#define RGX_LEAD_VERSION 1u" in older["raftgroups_lead.h"]
    assert "#define RGT_TERM_VERSION 1u" in older["raftgroups_term.h"]
    counts = {"rg_": 129, "rgx_": 8, "rgt_": 6}
    for name, prefix in (("raftgroups.h", "rg_"), ("raftgroups_lead.h", "rgx_"), ("raftgroups_term.h", "rgt_")):
        assert len(set(re.findall(r"\b(" + prefix + r"\w+)\s*\([^()]*\)\s*;", re.sub(r"/\*.*?\*/", "", older[name], flags=re.S)))) == counts[prefix], name
    nm = subprocess.run(["nm", "-D", "--defined-only", rg.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split() and " T " in l}
    assert {s for s in exported if s.startswith("rgv_")} == declared
    for prefix in ("rg_", "rgx_", "rgt_"):  # nothing new under the older prefixes
        assert len({s for s in exported if s.startswith(prefix)}) == counts[prefix], prefix
    lib = ctypes.CDLL(rg.LIB_PATH)
    for name in NEW_NAMES:
        assert hasattr(lib, name) and name in E.SYMBOLS, name
    rs = open(os.path.join(ROOT, "bindings", "raftgroups_vote.rs")).read()
    assert rs == gen_rust_bindings.generate_vote()
    assert open(os.path.join(ROOT, "bindings", "raftgroups_term.rs")).read() == gen_rust_bindings.generate_term()
    rust = {m.group(1): m.group(2) for m in re.finditer(r"pub fn (rgv_\w+)\((.*?)\)(?: -> [^;]+)?;", rs)}
    assert set(rust) == declared
    for name in declared:
        c_args = [x for x in re.search(r"\b" + name + r"\s*\(([^()]*)\)\s*;", plain, flags=re.S).group(1).split(",") if x.strip() and x.strip() != "void"]
        assert len(c_args) == len([x for x in rust[name].split(",") if x.strip()]) == len(E.SYMBOLS[name][1]), name
    for needle in ("pub struct RgvVoteOut", "pub struct RgvVoteRec", "pub struct RgvVoteResp", "pub const RGV_VOTE_VERSION: u32 = 1;", "pub const RGV_VOTE_EV_DEPOSED: u32 = 0x80;",
                   "dev_msgs: *const RgFollowMsgs", "dev_priority: *const i64", "use super::raftgroups_term::*;"):
        assert needle in rs, needle
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_bindings.py"), "--check"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lib.rgv_vote_version.restype = ctypes.c_uint32
    assert lib.rgv_vote_version() == int(re.search(r"#define RGV_VOTE_VERSION (\d+)u", hdr).group(1)) == E.VOTE_VERSION
    for k, v in (("LED", E.VOTE_EV_LED), ("TRANSFER_ABORTED", E.VOTE_EV_TRANSFER_ABORTED), ("DEPOSED", E.VOTE_EV_DEPOSED)):
        assert int(re.search(r"#define RGV_VOTE_EV_%s (0x[0-9a-f]+)u" % k, hdr).group(1), 16) == v == getattr(V, "EV_" + k), k
    assert (ctypes.sizeof(E.VoteOut), E.VOTE_REC_DTYPE.itemsize, E.VOTE_RESP_DTYPE.itemsize) == (64, 80, 48)
    assert [f for f, _ in E.VoteOut._fields_] == list(E.VOTE_OUT_FIELDS)
    assert E.VOTE_REC_DTYPE.names == ("follow_group", "lead_group", "term", "from", "index", "log_term", "commit", "commit_term", "priority", "kind", "flags")
    assert E.VOTE_RESP_DTYPE.names == ("term", "commit", "log_term", "last_index", "gate", "events", "status", "reserved")
    for method in ("follow_vote_device", "follow_vote", "follow_vote_counts"):
        assert callable(getattr(E.Engine, method)), method
    assert (E.ABI_VERSION, E.LEAD_VERSION, E.TERM_VERSION) == (12, 1, 1)
    lib.rgv_follow_vote_counts.restype = ctypes.c_void_p
    lib.rgv_follow_vote_counts.argtypes = [ctypes.c_void_p]
    assert lib.rgv_follow_vote_counts(None) is None


def test_api_refusals_are_host_checks():
    """What the calls refuse is decided on the host, before anything is staged or launched; the unit is not an abi_* unit and adds no
    kernel to ext_term.hip; every int entry point of it is a function-try-block that ends in RG_ABI_GUARD; the HIP-free header
    includes rg_term.h and the extension's public header only; the count words are free words of the d_counts scratch."""
    csrc = os.path.join(ROOT, "raft_rs_amd", "csrc")
    src = open(os.path.join(csrc, "ext_vote.hip")).read()
    for fn, needles in (("rgv_follow_vote_device", ("rg_vote_state", "dev_lead && h->host_mirror", "!dev_out->status", "!dev_out->log_term", "dev_out->answered_cap && !dev_out->answered",
                                                    "!dev_msgs->ent_term", "!dev_term")),
                        # (the record walk with its bounds and duplicate rules: rg_handoff_host.h, which tests/test_handoff_host.py reads)
                        ("rgv_follow_vote", ("rg_vote_state", "!rg_vote_is_request(q.kind)", "q.term == 0", "q.from == 0", "q.flags & ~RG_GATE_FORCE",
                                             'rg_walk_pairs(h, "rgv_follow_vote", host_recs, n, RG_WALK_NO_LEAD_OK | RG_WALK_SIDE_IN_WHO, rule)'))):
        body = src[src.index('extern "C" int %s(' % fn):]
        body = body[:body.index("} RG_ABI_GUARD")]
        enter = body.index("RG_ENTER(h)")
        for needle in needles:
            assert 0 <= body.find(needle) < enter, (fn, needle)
    sparse = src[src.index('extern "C" int rgv_follow_vote('):]
    assert 0 <= sparse.find("if (h->host_mirror) h->host_cfg_valid = false;") < sparse.index("rg_list_round_trip(")  # the mirror re-reads its cfg copy
    state = src[src.index("static int rg_vote_state("):src.index('extern "C" int rgv_follow_vote_device(')]
    assert "rg_elect_enabled" in state and "RG_GATE_CHECK_QUORUM" in state and state.count("RG_ERR_STATE") == 1  # (the other: rg_elect_enabled's)
    shared = open(os.path.join(csrc, "rg_handoff_host.h")).read()
    walk = shared[shared.index("static inline int rg_walk_pairs"):shared.index("// The round trip of a sparse call")]
    assert "no_lead_ok && q.lead_group == RG_HANDOFF_NO_LEAD" in walk and "q.lead_group >= h->G && !no_lead" in walk and "if (!no_lead)" in walk
    hdr = open(os.path.join(csrc, "rg_vote.h")).read()
    assert re.findall(r"#include\s+(\S+)", hdr) == ['"rg_term.h"', '"../../include/raftgroups_vote.h"']
    heads = [l for l in src.split("\n") if l.startswith('extern "C" int ')]
    assert len(heads) == 2 and src.count("\n} RG_ABI_GUARD") == 2
    for h in heads:  # (a prototype runs over several lines: the function-try-block opens where it ends)
        tail = src[src.index(h):]
        assert tail[:tail.index("{")].rstrip().endswith("try"), h
    assert "__global__" not in src and "k_vote_" not in open(os.path.join(csrc, "ext_term.hip")).read()
    # the count words: six of the 32 that the RG_COUNTS_* enum of rg_engine.h lays out (a static_assert there keeps its users apart);
    # the reductions use the first five, the term gate three behind them
    engine_h = open(os.path.join(csrc, "rg_engine.h")).read()
    at, term_at, hint_at = (int(re.search(r"\bRG_COUNTS_%s = (\d+)," % k, engine_h).group(1)) for k in ("VOTE", "TERM", "HINT"))
    assert at >= term_at + 3 and at + 6 <= 256 // 8 and not hint_at <= at < hint_at + 1 and "RG_COUNTS_WORDS = 32" in engine_h
    assert "h->d_counts + RG_COUNTS_VOTE)" in src and "h->d_counts + RG_COUNTS_TERM)" in open(os.path.join(csrc, "ext_term.hip")).read()
    assert "_COUNTS_AT" not in src + engine_h
    others = "".join(open(os.path.join(csrc, f)).read() for f in os.listdir(csrc) if f.endswith((".hip", ".h")) and f not in ("ext_vote.hip", "ext_term.hip"))
    # every other user starts at word 0 or at a word the enum names
    assert not re.search(r"d_counts\s*\+(?!\s*RG_COUNTS_)", others) and not re.search(r"d_counts\[", others)
    for m in re.finditer(r"hipMemsetAsync\(h->d_counts, 0, (\d+)", others):
        assert int(m.group(1)) <= 8 * term_at
    build = open(os.path.join(ROOT, "raft_rs_amd", "build.py")).read()
    assert '"ext_vote.hip"' in build and '"rg_vote.h"' in build and '"rg_kernels_vote.h"' in build and "raftgroups_vote.h" in build
    assert not os.path.exists(os.path.join(csrc, "abi_vote.hip"))
