"""CPU only: the leader's term gate and the deposition. (1) tests/term_gate_model.py restates the reference's term gate with its
lines named and composes the other stages' models; (2) three of the reference's scenarios run on it; (3) the arithmetic of
csrc/rg_term.h -- what the kernels run -- is compiled for the HOST with g++ (tests/host_check/term_gate_twin.cpp, a stand-alone
program) and diffed against the model over seeded rows, then once more under AddressSanitizer + UBSan, run directly; (4) what the
rows contain is asserted from the model alone; (5) every new name is declared, exported and bound, the two older headers are what
they were, and the refusals are host checks; (6) the kernels carry no scratch and no LDS (tools/kernel_resources.py).

Citations: pingcap/raft-rs v0.6.0."""
import ctypes
import os
import random
import re
import shutil
import subprocess
import sys

import pytest

import gate_model as G
import handoff_model as H
import lead_clock_model as L
import readonly_model as RO
import term_gate_model as T
from test_lead_clock_host import GATE, step_down_cases

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_NAMES = ("rgt_term_version", "rgt_lead_gate_device", "rgt_lead_gate_counts", "rgt_follow_depose", "rgt_follow_depose_device", "rgt_follow_depose_scan_device")
ROWS = 8000


def build_twin(tmp_path, name, extra):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build the host twin")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, os.path.join(HERE, "host_check", "term_gate_twin.cpp"), "-o", exe])
    return exe


def row_of(flags):
    return sum(b << (8 * s) for s, b in enumerate(flags))


def leader_of(term, last_index, self_id=1, read_depth=None):
    """A Raft that has just become leader at `term` with `last_index` entries of that term, as the three stages hold it: the lead
    group's log columns, its clock dict (led), the followed group in the state its win left."""
    cfg = L.cfg_word((0, 1, 2), self_slot=0)
    lead = H.fresh_lead(3, cfg)
    lead.update(commit=0, term_lo=1, term_hi=last_index, cur_term=term, dummy_index=0, dummy_term=0)
    node = G.Node(GATE, 7)
    node.load(term, self_id, self_id, 0, G.FOLLOWER, 0, 0, True)
    node.self_id = self_id
    clock = L.new_group(3, cfg, cur_term=term)
    ro = RO.Group(cfg, commit=0, term_lo=0, term=term, depth=read_depth) if read_depth else None
    return T.Leader(node, lead, clock, ro)


def test_model_cites_the_reference_lines():
    src = open(os.path.join(HERE, "term_gate_model.py")).read()
    for cite in ("raft.rs:1282-1411", ":1282-1283", ":1284-1348", ":1319-1330", ":1346", ":1349-1410", ":1399-1409", "raft.rs:942-971", ":952", ":957",
                 "raft.rs:1082-1087"):
        assert cite in src, cite
    # it composes the four models and defines nothing they define
    for mod in ("gate_model", "handoff_model", "lead_clock_model"):
        assert "import %s" % mod in src
    for theirs in ("def demote", "def become_follower", "def reset", "def abort_leader_transfer", "def quorum_recently_active", "def draw"):
        assert theirs not in src, theirs


def test_all_server_stepdown_leader_row():
    """harness/tests/integration_cases/test_raft.rs:1721-1781, the Leader row: become_candidate + become_leader at term 1 (one
    entry), then MsgRequestVote and MsgAppend of term 3 from peer 2. After each: Follower, term 3, last_index 1, one entry;
    leader_id 0 after the vote request and 2 after the append."""
    ld = leader_of(1, 1)
    assert ld.state == "Leader"
    assert ld.step_higher(3, G.INVALID_ID) == "deposed"  # MsgRequestVote: no check_quorum, so no lease (raft.rs:1288-1292)
    n = ld.node
    assert (ld.state, n.role, n.term, n.lead, n.vote) == ("Follower", G.FOLLOWER, 3, 0, 0)
    c = n.log.canonical()
    assert c["last_index"] == 1 and c["runs"] == [(1, 1)]
    assert ld.lead["cur_term"] == 1  # RG_COL_CUR_TERM is left alone, as a demotion leaves it
    # the MsgAppend of the same term now finds a follower: the equal-term arm, step_follower sets leader_id = m.from
    m = G.Msg(G.APPEND, 3, 2, index=0, log_term=3)
    n.step(m)
    assert (n.role, n.term, n.lead) == (G.FOLLOWER, 3, 2) and n.log.canonical()["last_index"] == 1


def test_disruptive_follower_last_step():
    """test_raft.rs:2154-2170: the leader n1 at term 2 gets the candidate's MsgAppendResponse of term 3 and becomes a Follower at
    term 3 that knows no leader; its pending reads are gone (Raft::reset, raft.rs:957)."""
    ld = leader_of(2, 2, read_depth=4)
    ld.read_only.term_lo = 0
    assert ld.read_only.request(11)[0] == RO.QUEUED
    assert ld.step_response("MsgAppendResponse", 3) == "deposed"
    n = ld.node
    assert (ld.state, n.role, n.term, n.lead, n.vote, n.elapsed) == ("Follower", G.FOLLOWER, 3, 0, 0, 0)
    assert ld.read_only.queue() == [] and ld.read_only.ack(1, 11) == []
    assert GATE.min_timeout <= n.timeout < GATE.max_timeout
    # a response that arrives afterwards finds no leader
    assert ld.step_response("MsgHeartbeatResponse", 3) == "ignored"


def test_a_stale_response_is_ignored():
    """raft.rs:1349-1410: a response of a lower term changes nothing and nothing is sent; equal and local terms are stepped."""
    ld = leader_of(3, 4, read_depth=4)
    assert ld.read_only.request(5)[0] == RO.QUEUED
    before = (ld.node.soft(), H.copy_lead(ld.lead), L.copy_group(ld.clock), ld.read_only.queue())
    for kind in T.MSG_KINDS:
        assert ld.step_response(kind, 2) == "ignored"
        assert ld.step_response(kind, 3) == "stepped" and ld.step_response(kind, 0) == "stepped"
    assert (ld.node.soft(), ld.lead, ld.clock, ld.read_only.queue()) == before and ld.state == "Leader"
    # ... and the row form: the stale slot keeps SENT | INS_FULL, its neighbours pass untouched
    flags = [T.MF_VALID | T.MF_SENT | T.MF_INS_FULL | T.MF_REJECT | T.MF_HAS_LOGTERM, T.MF_HEARTBEAT, T.MF_VALID | T.MF_APPEND, 0, 0, 0, 0, 0]
    row, ev, new_term, stale, not_led = T.gate(ld.clock, flags, [2, 3, 0, 9, 9, 9, 9, 9], 3)
    assert (row, ev, new_term, stale, not_led) == ([T.MF_SENT | T.MF_INS_FULL, T.MF_HEARTBEAT, T.MF_VALID | T.MF_APPEND, 0, 0, 0, 0, 0], T.EV_STALE, None, 1, 0)


def gate_cases(seed, n):
    """(P, clock dict, flags, terms): every flag bit x {t = 0, < cur, == cur, > cur} x {led, stopped, tag != cur}."""
    rng = random.Random(seed)
    out = []
    for k in range(n):
        P = rng.choice((1, 3, 5, 8))
        cur = rng.choice((1, 2, 5, 9, 1 << 40))
        cfg = L.cfg_word(range(min(P, 3)), self_slot=0, transferee=(rng.randrange(P) if rng.random() < 0.4 else None))
        g = T.random_clock(rng, cfg, cur)
        flags, terms = T.random_row(rng, P, cur, calm=0.6)
        out.append((P, g, flags, terms))
    # the exhaustive grid on one slot: every flag bit alone x the four term classes x the three clock states
    for bit in T.FLAG_BITS:
        for t in (0, 4, 5, 6):
            for state in ("led", "stopped", "tag"):
                g = L.new_group(3, L.cfg_word((0, 1, 2), self_slot=0, transferee=1), cur_term=5)
                g["el"], g["hb"] = 3, 1
                if state == "stopped":
                    g["led"] = False
                elif state == "tag":
                    g["tag"], g["led"] = 4, False
                out.append((3, g, [0, bit | (T.MF_SENT if bit != T.MF_SENT else 0), 0, 0, 0, 0, 0, 0], [0, t, 0, 0, 0, 0, 0, 0]))
    return out


def run_gates(exe, cases):
    lines = ["G %d %d %d %d %d %d %s" % (P, L.cell_word(g), g["tag"], g["cur_term"], g["cfg"], row_of(flags), " ".join("%d" % t for t in terms))
             for P, g, flags, terms in cases]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    got = out.stdout.split("\n")[:-1]
    assert len(got) == len(cases)
    seen = set()
    for line, (P, g, flags, terms) in zip(got, cases):
        m = L.copy_group(g)
        row, ev, new_term, stale, not_led = T.gate(m, flags, terms, P)
        want = [ev, row_of(row), new_term or 0, stale, not_led, L.cell_word(m), m["tag"], m["cfg"]]
        w = line.split()
        assert w[0] == "G" and [int(x) for x in w[1:]] == want, (line, want, P, g, flags, terms)
        if not ev & T.EV_DEPOSED:
            assert m == g  # nothing of an undeposed group's state changes
        seen.add(ev)
    return seen


def depose_cases(seed, n):
    rng = random.Random(seed)
    out = []
    for node, lead in step_down_cases(seed, n):
        new_term = max(0, lead["cur_term"] + rng.choice((-1, 0, 1, 1, 1, 7)))
        out.append((node, lead, new_term, rng.random() < 0.7))
    return out


def run_deposes(exe, cases):
    lines, want = [], []
    for node, lead, new_term, soft in cases:
        clock = node.elapsed | int(node.promotable) << 15 | node.timeout << 16
        lines.append("D %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %s %s" % (
            soft, new_term, node.role, node.lead, node.self_id, node.term, clock, GATE.seed, GATE.min_timeout, GATE.max_timeout, node.group, lead["commit"],
            lead["term_lo"], lead["term_hi"], lead["cur_term"], lead["dummy_index"], lead["dummy_term"], lead["run_count"],
            " ".join("%d" % x for x in lead["run_first"]), " ".join("%d" % x for x in lead["run_term"])))
        lead["cfg"] = lead.get("cfg", 0)
        before_lead, before_soft = H.copy_lead(lead), node.soft()
        a, c = T.depose(node, lead, new_term, soft=soft)
        if a[0] != H.DONE:
            assert node.soft() == before_soft and lead == before_lead
            want.append([a[0]])
        elif soft:
            assert (node.term, node.vote, node.role, node.lead, node.elapsed) == (new_term, 0, G.FOLLOWER, 0, 0) and new_term > before_soft[0]
            new_clock = int(node.promotable) << 15 | node.timeout << 16
            want.append([a[0], new_term, a[2], a[3], 0, new_term, new_clock, 1 | 2 | 8 | (4 if new_clock != clock else 0)])
        else:
            assert node.soft() == before_soft
            want.append([a[0], new_term, a[2], a[3], node.lead, node.term, clock, 0])
    out = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    got = out.stdout.split("\n")[:-1]
    assert len(got) == len(cases)
    for line, w in zip(got, want):
        assert line.split()[0] == "D" and [int(x) for x in line.split()[1:]] == w, (line, w)
    return {(w[0], c[3]) for w, c in zip(want, cases)}


def run_scans(exe, seed, n):
    rng = random.Random(seed)
    lines, want = [], []
    for node, lead in step_down_cases(seed, n):
        kind = rng.choice((0, G.APPEND, G.HEARTBEAT, G.TOUCH, G.VOTE, G.PREVOTE, G.APPEND | G.HEARTBEAT))
        m_term = max(0, node.term + rng.choice((-1, 0, 1, 2)))
        lines.append("N %d %d %d %d %d %d %d" % (kind, node.role, node.lead, node.self_id, node.term, lead["cur_term"], m_term))
        want.append(int(T.scan_selects(node, lead, kind, m_term)))
    got = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")[:-1]
    assert [l.split() for l in got] == [["N", str(w)] for w in want]
    return set(want)


def test_rows_cover_the_issue_list_from_the_model_alone():
    """Every flag bit x every term class x every clock state occurs; every event byte the gate can give occurs; a deposition and a
    stale report never come together; bytes at or beyond P survive unless the row is zeroed."""
    combos, events = set(), set()
    for P, g, flags, terms in gate_cases(31, ROWS):
        state = "tag" if g["tag"] != g["cur_term"] else "led" if g["led"] else "stopped"
        for s in range(P):
            if T.is_record(flags[s]) or flags[s]:
                cls = T.term_branch(g["cur_term"], terms[s])
                for bit in T.FLAG_BITS:
                    if flags[s] & bit:
                        combos.add((bit, cls, state))
        m = L.copy_group(g)
        row, ev, new_term, stale, not_led = T.gate(m, flags, terms, P)
        events.add(ev)
        assert not (ev & T.EV_DEPOSED and ev & (T.EV_STALE | T.EV_NOT_LED)) and bool(ev & T.EV_DEPOSED) == (new_term is not None)
        if ev & (T.EV_DEPOSED | T.EV_NOT_LED):
            assert row == [0] * 8
        else:
            assert row[P:] == flags[P:] and all((row[s] ^ flags[s]) & ~T.RESPONSE_BITS & 0xFF == 0 for s in range(8))
        if ev & T.EV_DEPOSED:
            assert not m["led"] and m["tag"] == m["cur_term"] and m["cfg"] >> 20 & 0xF == 0 and new_term > g["cur_term"]
    assert combos >= {(bit, cls, state) for bit in T.FLAG_BITS for cls in (T.LOCAL, T.EQUAL, T.LOWER, T.HIGHER) for state in ("led", "stopped", "tag")}
    assert events == {0, T.EV_STALE, T.EV_NOT_LED, T.EV_DEPOSED, T.EV_DEPOSED | T.EV_TRANSFER_ABORTED}
    kinds = set()
    for node, lead, new_term, soft in depose_cases(33, 3000):
        kinds.add((T.depose(node, lead, new_term, soft=soft)[0][0], soft))
    assert kinds == {(s, soft) for s in (H.DONE, H.NOT_WON, H.FAULT) for soft in (True, False)}


def test_host_twin_matches_the_model(tmp_path):
    exe = build_twin(tmp_path, "term_gate_twin", [])
    for seed in (31, 32):
        seen = run_gates(exe, gate_cases(seed, ROWS))
        assert seen == {0, T.EV_STALE, T.EV_NOT_LED, T.EV_DEPOSED, T.EV_DEPOSED | T.EV_TRANSFER_ABORTED}
    assert run_deposes(exe, depose_cases(33, 3000)) == {(s, soft) for s in (H.DONE, H.NOT_WON, H.FAULT) for soft in (True, False)}
    assert run_scans(exe, 34, 2000) == {0, 1}


def test_host_twin_is_clean_under_asan_and_ubsan(tmp_path):
    """The same program, -fsanitize=address,undefined -fno-sanitize-recover=all, run directly (a stand-alone executable)."""
    exe = build_twin(tmp_path, "term_gate_twin_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    run_gates(exe, gate_cases(35, 2000))
    run_deposes(exe, depose_cases(36, 600))
    run_scans(exe, 37, 400)


def test_kernels_carry_no_scratch_and_no_lds():
    """tools/kernel_resources.py over ext_term.hip: the gate and the three deposition kernels, both index widths."""
    from raft_rs_amd import build as engine_build
    engine_build.hipcc()  # (raises where there is no hipcc: the engine is built with it)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--src=raft_rs_amd/csrc/ext_term.hip"], cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines()[1:]:
        m = re.match(r"(\S.*?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)$", line)
        if m:
            rows[m.group(1)] = (int(m.group(5)), int(m.group(6)))
    want = sorted(name + "<unsigned %s>" % w for name in ("k_term_gate", "k_term_depose_list", "k_term_depose_dense", "k_term_depose_scan") for w in ("int", "long"))
    assert sorted(rows) == want, (sorted(rows), out.stderr[-1000:])  # ... and the unit instantiates none of the clock's kernels
    for k, (scratch, lds) in rows.items():
        print(k, scratch, lds)
        assert scratch == 0 and lds == 0, (k, scratch, lds)


def test_every_new_name_is_declared_exported_and_bound(rg):
    """include/raftgroups_term.h: every function it declares is exported (as rgt_*, nothing else with that prefix) and bound, in
    Python and in the generated bindings/raftgroups_term.rs with the header's arity; raftgroups.h and raftgroups_lead.h, their
    versions and their counts are what they were."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_bindings
    from raft_rs_amd import engine as E
    hdr = open(os.path.join(ROOT, "include", "raftgroups_term.h"), encoding="utf-8").read()
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(rgt_\w+)\s*\([^()]*\)\s*;", plain))
    assert declared == set(NEW_NAMES)
    assert not re.findall(r"\b(rgx?_\w+)\s*\([^()]*\)\s*;", plain)  # ... and it declares no rg_* / rgx_* function
    core = open(os.path.join(ROOT, "include", "raftgroups.h"), encoding="utf-8").read()
    lead = open(os.path.join(ROOT, "include", "raftgroups_lead.h"), encoding="utf-8").read()
    assert "rgt_" not in core and "rgt_" not in lead and "#define RG_ABI_VERSION 12u" in core and "#define RGX_LEAD_VERSION 1u" in lead
    assert len({name for name, _, _ in gen_rust_bindings.parse(core)[3]}) == 129
    assert len(set(re.findall(r"\b(rgx_\w+)\s*\([^()]*\)\s*;", re.sub(r"/\*.*?\*/", "", lead, flags=re.S)))) == 8
    nm = subprocess.run(["nm", "-D", "--defined-only", rg.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert {l.split()[-1] for l in nm.splitlines() if l.split() and l.split()[-1].startswith("rgt_")} == declared
    lib = ctypes.CDLL(rg.LIB_PATH)
    for name in NEW_NAMES:
        assert hasattr(lib, name) and name in E.SYMBOLS, name
    rs = open(os.path.join(ROOT, "bindings", "raftgroups_term.rs")).read()
    assert rs == gen_rust_bindings.generate_term()
    assert open(os.path.join(ROOT, "bindings", "raftgroups_lead.rs")).read() == gen_rust_bindings.generate_lead()
    rust = {m.group(1): m.group(2) for m in re.finditer(r"pub fn (rgt_\w+)\((.*?)\)(?: -> [^;]+)?;", rs)}
    assert set(rust) == declared
    for name in declared:
        c_args = [x for x in re.search(r"\b" + name + r"\s*\(([^()]*)\)\s*;", plain, flags=re.S).group(1).split(",") if x.strip() and x.strip() != "void"]
        assert len(c_args) == len([x for x in rust[name].split(",") if x.strip()]), name
    for needle in ("pub struct RgtLeadGateOut", "pub struct RgtDeposeRec", "pub const RGT_TERM_VERSION: u32 = 1;", "pub const RGT_GATE_EV_DEPOSED: u32 = 0x80;",
                   "dev_out: *const RgHandoffOut", "dev_msgs: *const RgMsgs"):
        assert needle in rs, needle
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_bindings.py"), "--check"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lib.rgt_term_version.restype = ctypes.c_uint32
    assert lib.rgt_term_version() == int(re.search(r"#define RGT_TERM_VERSION (\d+)u", hdr).group(1)) == E.TERM_VERSION
    for k, v in (("TRANSFER_ABORTED", E.TERM_GATE_EV_TRANSFER_ABORTED), ("STALE", E.TERM_GATE_EV_STALE), ("NOT_LED", E.TERM_GATE_EV_NOT_LED),
                 ("DEPOSED", E.TERM_GATE_EV_DEPOSED)):
        assert int(re.search(r"#define RGT_GATE_EV_%s (0x[0-9a-f]+)u" % k, hdr).group(1), 16) == v == getattr(T, "EV_" + k), k
    assert E.TERM_GATE_EV_TRANSFER_ABORTED == E.LEAD_EV_TRANSFER_ABORTED
    assert (ctypes.sizeof(E.TermGateOut), E.DEPOSE_REC_DTYPE.itemsize) == (40, 32)
    assert [f for f, _ in E.TermGateOut._fields_] == list(E.TERM_GATE_OUT_FIELDS) and E.DEPOSE_REC_DTYPE.names == ("follow_group", "lead_group", "term", "reserved")
    for method in ("lead_gate_device", "lead_gate_counts", "follow_depose", "follow_depose_device", "follow_depose_scan_device"):
        assert callable(getattr(E.Engine, method)), method
    assert E.ABI_VERSION == 12 and E.LEAD_VERSION == 1
    lib.rgt_lead_gate_counts.restype = ctypes.c_void_p
    lib.rgt_lead_gate_counts.argtypes = [ctypes.c_void_p]
    assert lib.rgt_lead_gate_counts(None) is None


def test_api_refusals_are_host_checks():
    """What the calls refuse is decided on the host, before anything is staged or launched; the unit is not an abi_* unit, every
    int entry point of it ends in RG_ABI_GUARD; the HIP-free header includes rg_lead.h and the extension's public header."""
    src = open(os.path.join(ROOT, "raft_rs_amd", "csrc", "ext_term.hip")).read()
    for fn, needles in (("rgt_lead_gate_device", ("!h->ld", "h->host_mirror", "!dev_out->events", "!dev_out->new_term", "dev_out->down_cap && !dev_out->down")),
                        # (the election layer, and the record walk with its bounds and duplicate rules: rg_handoff_host.h, which
                        # tests/test_handoff_host.py reads)
                        ("rgt_follow_depose", ("rg_elect_enabled", "q.reserved", "rg_walk_pairs")),
                        ("rgt_follow_depose_device", ("rg_elect_enabled", "h->host_mirror", "rg_handoff_out_complete")),
                        ("rgt_follow_depose_scan_device", ("rg_elect_enabled", "h->host_mirror", "rg_handoff_out_complete"))):
        body = src[src.index('extern "C" int %s(' % fn):]
        body = body[:body.index("} RG_ABI_GUARD")]
        enter = body.index("RG_ENTER(h)")
        for needle in needles:
            assert 0 <= body.find(needle) < enter, (fn, needle)
    hdr = open(os.path.join(ROOT, "raft_rs_amd", "csrc", "rg_term.h")).read()
    assert re.findall(r"#include\s+(\S+)", hdr) == ['"rg_lead.h"', '"../../include/raftgroups_term.h"']
    heads = [l for l in src.split("\n") if l.startswith('extern "C" int ')]
    assert len(heads) == 4 and src.count("\n} RG_ABI_GUARD") == 4
    for h in heads:  # (a prototype may run over two lines: the function-try-block opens where it ends)
        tail = src[src.index(h):]
        assert tail[:tail.index("{")].rstrip().endswith("try"), h
    build = open(os.path.join(ROOT, "raft_rs_amd", "build.py")).read()
    assert '"ext_term.hip"' in build and '"rg_term.h"' in build and '"rg_kernels_term.h"' in build and "raftgroups_term.h" in build
    assert not os.path.exists(os.path.join(ROOT, "raft_rs_amd", "csrc", "abi_term.hip"))
