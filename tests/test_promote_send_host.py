"""CPU only: the promotion into an engine with device Inflights (include/raftgroups_handoff.h). (1) tests/promote_send_model.py --
handoff_model.promote, then the window resets and the reference's own send loop, line by line -- against the reference's route
through the oracle (handoff_rig.route_state, the RG_MF_BECOME_LEADER tick, Cluster.send_stage_soa with the oracle's own Inflights):
every leader column, every window, the item set, exactly; (2) the closed form of csrc/rg_promote.h -- what the kernels run -- compiled
for the HOST with g++ (tests/host_check/promote_send_twin.cpp, a stand-alone program) against the model over seeded cases, and once
more under AddressSanitizer + UBSan, run directly; (3) the same closed form against rg_group_send itself, the send stage's own code
on the host (tests/host_check/host_tick.hip); (4) the size of the empty entry against the exported rg_entry_size at the varint
boundaries; (5) every rgh_* name is declared, exported and bound, the older export sets are what they were, the refusals are host
checks; (6) no kernel instantiation carries scratch (tools/kernel_resources.py: resource metadata only).

Citations: pingcap/raft-rs v0.6.0."""
import ctypes
import os
import random
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import handoff_model as H
import handoff_rig as R
import promote_send_model as M
import sendstage
from test_handoff_host import promote_line
from test_host_check import host_send  # noqa: F401  (the fixture: rg_group_send on the host)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_NAMES = ("rgh_handoff_version", "rgh_follow_promote", "rgh_follow_promote_device")
SWEEP = 4000
U64_MAX = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------------------------------
# 1. the model against the reference's route through the oracle
# ---------------------------------------------------------------------------------------------------------------------
def model_and_route(P, cap, cases, **limits):
    st = R.state_with(M.N_LEAD, P, 256, cases)
    meta, ring, shapes = M.window_arrays(M.N_LEAD, P, 256, cap, [c.L for c in cases])
    want, want_meta, answers, items = M.promote_state(st, meta, ring, cases, cap, **limits)
    after, gout, sent, cl = M.oracle_route(st, cases, cap, **limits)
    diffs = R.diff(want, after)
    assert not diffs, (P, cap, diffs)
    sendstage.compare_items(M.items_array(items), sent)
    done = [c for c in cases if c.expect == H.DONE]
    routed = want_meta.copy()
    for c in cases:  # (the oracle's windows were empty at the load: those of a refused group are not its to compare)
        if c.expect != H.DONE:
            assert (want_meta[:, c.L] == meta[:, c.L]).all(), c.name
            routed[:, c.L] = 0
    sendstage.compare_rings(cl, routed, ring, after, cap)
    for c, a in zip(cases, answers):
        assert int(gout[c.L]) == a[4] == (0x18 if c.expect == H.DONE else 0), c.name
    return st, meta, shapes, want, want_meta, items, done


@pytest.mark.parametrize("cap", [1, 4, 8])
@pytest.mark.parametrize("P", [1, 3, 5, 8])
def test_model_equals_the_route_through_the_oracle(oracle, P, cap):
    """Slot counts 1, 3, 5 and 8, windows in all five starting shapes: every column, every window and the item set of the oracle's
    tick + send stage; the peers end up Probe and paused with one item each, learners included, the own and the absent slots none."""
    cases = M.edge_cases(P)
    st, meta, shapes, want, want_meta, items, done = model_and_route(P, cap, cases)
    assert set(shapes.values()) == set(M.WINDOW_SHAPES) and {a for a in (c.expect for c in cases)} == {H.DONE, H.FAULT}
    for c in done:
        incoming, outgoing, self_slot, _, present = H.cfg_fields(c.lead["cfg"])
        hi = c.f.canonical()["last_index"] + 1
        for s in range(P):
            if not present >> s & 1:
                assert (c.L, s) not in items and want_meta[s, c.L] == meta[s, c.L] and int(want["pflags"][c.L, s]) == c.lead["pflags"][s]
            elif s == self_slot:
                assert (c.L, s) not in items and want_meta[s, c.L] == 0 and int(want["pflags"][c.L, s]) & 0x1F == H.REPLICATE
            else:
                assert items[(c.L, s)] == (M.SEND_APPEND, hi - 1, hi, 1) and want_meta[s, c.L] == 0 and int(want["pflags"][c.L, s]) == H.PROBE | M.PF_PAUSED
    if P in (5, 8):
        assert any(not (H.cfg_fields(c.lead["cfg"])[0] | H.cfg_fields(c.lead["cfg"])[1]) >> s & 1 for c in done for (L, s) in items if L == c.L), "a learner gets an item"
    if P == 1:
        assert not items


@pytest.mark.parametrize("limits", [{"max_entries": 1}, {"max_bytes": 0}, {"max_bytes": 1}, {"max_bytes": U64_MAX}])
def test_no_limit_splits_the_one_entry(oracle, limits):
    """max_entries_per_msg 1 and Config::max_size_per_msg of 0, 1 and NO_LIMIT bytes: the reference's stage sends the same single
    entry to every peer (util::limit_size keeps the first entry whatever its size)."""
    a = model_and_route(5, 8, M.edge_cases(5), **limits)
    b = model_and_route(5, 8, M.edge_cases(5))
    assert a[5] == b[5] and not R.diff(a[3], b[3])


def test_handoff_model_cases_too(oracle):
    """handoff_model.gpu_cases (the cases the older promotion is tested on), on their own shapes"""
    for P in (3, 8):
        cases = H.gpu_cases(P)
        st = R.state_with(H.SHAPES[P], P, 512, cases)
        meta, ring, _ = M.window_arrays(H.SHAPES[P], P, 512, 4, [c.L for c in cases])
        want, want_meta, answers, items = M.promote_state(st, meta, ring, cases, 4)
        after, gout, sent, cl = M.oracle_route(st, cases, 4)
        assert not R.diff(want, after)
        sendstage.compare_items(M.items_array(items), sent)


def test_model_cites_the_reference():
    src = open(os.path.join(HERE, "promote_send_model.py")).read()
    for needle in ("raft.rs:773-819", "raft.rs:857-864", "progress.rs:210-216", "progress.rs:231-243", "progress.rs:82-92", "inflights.rs:121-124", "util.rs:52-76",
                   "raft.rs:959-966", ":2190-2191", "H.promote("):
        assert needle in src, needle


# ---------------------------------------------------------------------------------------------------------------------
# 2. the stand-alone twin of csrc/rg_promote.h
# ---------------------------------------------------------------------------------------------------------------------
def build_twin(tmp_path, name, extra):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build the host twin")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, os.path.join(HERE, "host_check", "promote_send_twin.cpp"), "-o", exe])
    return exe


def sweep_cases(seed, n):
    """(Follower, lead, P, persisted, cap, window metas, esz_w, esz row): handoff_model.random_case with random windows and size rows"""
    rng = random.Random(seed)
    out = []
    for k in range(n):
        P = rng.choice((1, 3, 3, 5, 7, 8))
        f, lead, persisted = H.random_case(rng, P)
        for s in range(P):  # the engine keeps the PEND bits exact and the cells of a clean Progress zero
            lead["pend_rs"][s] = 23 if lead["pflags"][s] & H.PF_PEND_RS else 0
        cap = rng.choice((1, 4, 8, 256))
        metas = []
        for s in range(P):
            start, entries = M.window_of(rng.choice(M.WINDOW_SHAPES), cap)
            metas.append(start | len(entries) << 16)
        esz_w = rng.choice((0, 8, 8, 64))
        esz = [rng.randrange(1 << 32) for _ in range(esz_w)]
        out.append((f, lead, P, persisted, cap, metas, esz_w, esz))
    return out


def run_twin(exe, cases):
    lines = []
    for f, lead, P, persisted, cap, metas, esz_w, esz in cases:
        lines.append("S" + promote_line(f, lead, P, persisted)[1:] + " %d" % esz_w + "".join(" %d" % v for v in esz) + "".join(" %d" % v for v in metas))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    got = out.stdout.split("\n")[:-1]
    assert len(got) == len(cases)
    statuses = []
    for k, (line, (f, lead, P, persisted, cap, metas, esz_w, esz)) in enumerate(zip(got, cases)):
        w = line.split()
        m = H.copy_lead(lead)
        present = H.cfg_fields(lead["cfg"])[4]
        win = [[1] * (metas[s] >> 16) if present >> s & 1 else None for s in range(P)]
        row = list(esz) if esz_w else None
        a, items = M.promote_send(f, m, win, P, cap, persisted, esz=row, esz_w=esz_w)
        assert w[0] == "S" and tuple(int(x) for x in w[1:6]) == a, (k, line, a)
        statuses.append(a[0])
        if a[0] != H.DONE:
            assert len(w) == 6 and m == lead, (k, line)
            continue
        assert w[6] == "F" and w[11] == "E" and w[12 + esz_w] == "M" and w[13 + esz_w + P] == "I", (k, line)
        pf, windows, peers, n_items = (int(x) for x in w[7:11])
        assert [pf >> (8 * s) & 0xFF for s in range(P)] == m["pflags"], (k, line, m["pflags"])
        assert pf >> (8 * P) == sum(b << (8 * s) for s, b in enumerate(lead["pflags"])) >> (8 * P)
        assert windows == present & ((1 << P) - 1) and peers == windows & ~(1 << H.cfg_fields(lead["cfg"])[2]) and n_items == len(items)
        assert [int(x) for x in w[12:12 + esz_w]] == (row or []), (k, line, row)
        assert [int(x) for x in w[13 + esz_w:13 + esz_w + P]] == [0 if win[s] is not None else metas[s] for s in range(P)], (k, line)
        assert all(v == [] for v in win if v is not None)
        flat = [int(x) for x in w[14 + esz_w + P:]]
        assert [tuple(flat[i:i + 5]) for i in range(0, len(flat), 5)] == [(s, prev, last, n, kind) for s, kind, prev, last, n in items], (k, line, items)
    return statuses


def test_host_twin_matches_the_model(tmp_path):
    """Seeded cases: every answer field, the flag row, the window cells, the size row and the items the kernels would store."""
    exe = build_twin(tmp_path, "promote_send_twin", [])
    for seed in (21, 22):
        st = run_twin(exe, sweep_cases(seed, SWEEP))
        assert set(st) == {H.DONE, H.NOT_WON, H.CONF, H.NOT_PERSISTED, H.FAULT}


def test_host_twin_is_clean_under_asan_and_ubsan(tmp_path):
    """The same program, -fsanitize=address,undefined -fno-sanitize-recover=all, run directly (a stand-alone executable)."""
    exe = build_twin(tmp_path, "promote_send_twin_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert len(run_twin(exe, sweep_cases(23, 1500))) == 1500
    out = subprocess.run([exe], input="Z 0 0\nZ 18446744073709551615 18446744073709551615\n", stdout=subprocess.PIPE, text=True, check=True).stdout
    assert out == "Z 0\nZ 22\n"


# ---------------------------------------------------------------------------------------------------------------------
# 3. the closed form against the send stage's own code
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,cap,max_entries,flags", [(3, 4, 0, 0), (5, 8, 1, 0), (5, 8, 0, 1), (8, 1, 0, 0), (1, 4, 0, 0), (5, 8, 0, 2), (5, 8, U64_MAX, 2)])
def test_closed_form_is_what_rg_group_send_does(host_send, P, cap, max_entries, flags):  # noqa: F811
    """rg_group_send (csrc/rg_send.h, compiled for the host) over the cells handoff_model.promote leaves, with the result word
    RG_OUT_BECAME_LEADER | RG_OUT_APPENDED and the windows in their starting shapes: the state, the windows and the items are the
    model's -- and so the twin's, which is the closed form the kernels run. flags 1 = RG_SEND_SKIP_BCAST_COMMIT, 2 = RG_SEND_BYTES."""
    cases = M.edge_cases(P)
    st = R.state_with(M.N_LEAD, P, 256, cases)
    meta, ring, _ = M.window_arrays(M.N_LEAD, P, 256, cap, [c.L for c in cases])
    want, want_meta, answers, items = M.promote_state(st, meta, ring, cases, cap)
    promoted, _ = R.model_state(st, cases)  # the promotion alone
    out = np.zeros(M.N_LEAD, dtype=np.uint32)
    head, tail = np.zeros((P, 256), dtype=np.uint64), np.zeros((P, 256), dtype=np.uint64)
    for c in cases:
        if c.expect == H.DONE:
            out[c.L] = 0x18
        for s in range(P):  # the engine-internal columns of a ring window: its oldest and its newest entry
            start, count = int(meta[s, c.L]) & 0xFFFF, int(meta[s, c.L]) >> 16
            if count:
                head[s, c.L], tail[s, c.L] = ring[c.L, s, start], ring[c.L, s, (start + count - 1) % cap]
    esz = np.full((M.N_LEAD, 8), 5, dtype=np.uint32) if flags & 2 else None
    got_meta = meta.copy()
    got = host_send(promoted, out, got_meta, (head, tail), ring.copy(), cap, max_entries, flags, esz=esz)
    diffs = R.diff(want, promoted)
    assert not diffs, diffs
    assert sendstage.items_dict(got) == items
    for c in cases:
        self_slot, present = H.cfg_fields(c.lead["cfg"])[2], H.cfg_fields(c.lead["cfg"])[4]
        for s in range(P):  # (the stage never looks at the own slot: the call empties that window itself)
            if c.expect != H.DONE or s != self_slot or not present >> s & 1:
                assert got_meta[s, c.L] >> 16 == want_meta[s, c.L] >> 16, (c.name, s)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the size of the empty entry
# ---------------------------------------------------------------------------------------------------------------------
def test_empty_entry_size_is_rg_entry_size(rg, tmp_path):
    """T and hi at the varint boundaries -- 0, 1, 127/128, 2^14 - 1/2^14, 2^35, 2^63 - 1 -- against the exported rg_entry_size, in
    the model and in the twin"""
    from raft_rs_amd import engine as E
    edges = [0, 1, 127, 128, (1 << 14) - 1, 1 << 14, 1 << 35, (1 << 63) - 1]
    exe = build_twin(tmp_path, "promote_send_twin", [])
    pairs = [(t, i) for t in edges for i in edges]
    out = subprocess.run([exe], input="".join("Z %d %d\n" % p for p in pairs), stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")[:-1]
    lib = rg.load_library()
    for (t, i), line in zip(pairs, out):
        e = E.EntryC(0, 0, t, i, None, 0, None, 0)
        want = int(lib.rg_entry_size(ctypes.byref(e)))
        assert M.empty_entry_size(t, i) == want == int(line.split()[1]), (t, i, want, line)
    assert M.empty_entry_size(127, 128) == 2 + 3 and M.empty_entry_size(1 << 35, (1 << 63) - 1) == 7 + 10


# ---------------------------------------------------------------------------------------------------------------------
# 5. declared, exported, bound; refusals are host checks
# ---------------------------------------------------------------------------------------------------------------------
def test_every_new_name_is_declared_exported_and_bound(rg):
    """include/raftgroups_handoff.h: every function it declares is exported (as rgh_*, nothing else with that prefix) and bound, in
    Python and in the generated bindings/raftgroups_handoff.rs with the header's arity; the four older headers, their versions,
    their export sets and their generated bindings are what they were."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_bindings
    from raft_rs_amd import engine as E
    hdr = open(os.path.join(ROOT, "include", "raftgroups_handoff.h"), encoding="utf-8").read()
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(rgh_\w+)\s*\([^()]*\)\s*;", plain))
    assert declared == set(NEW_NAMES)
    assert not re.findall(r"\b(rg[xtv]?_\w+)\s*\([^()]*\)\s*;", plain)  # ... and it declares no function of an older prefix
    assert '#include "raftgroups.h"' in hdr and "SUPERSEDES" in hdr and "stay the host's duty" in hdr
    older = {k: open(os.path.join(ROOT, "include", k), encoding="utf-8").read() for k in ("raftgroups.h", "raftgroups_lead.h", "raftgroups_term.h", "raftgroups_vote.h")}
    assert all("rgh_" not in v and "RGH_" not in v for v in older.values())
    for name, needle in (("raftgroups.h", "#define RG_ABI_VERSION 12u"), ("raftgroups_lead.h", "#define RGX_LEAD_VERSION 1u"), ("raftgroups_term.h", "#define RGT_TERM_VERSION 1u"),
                         ("raftgroups_vote.h", "#define RGV_VOTE_VERSION 1u")):
        assert needle in older[name], name
    counts = {"rg_": 129, "rgx_": 8, "rgt_": 6, "rgv_": 4}
    for name, prefix in (("raftgroups.h", "rg_"), ("raftgroups_lead.h", "rgx_"), ("raftgroups_term.h", "rgt_"), ("raftgroups_vote.h", "rgv_")):
        assert len(set(re.findall(r"\b(" + prefix + r"\w+)\s*\([^()]*\)\s*;", re.sub(r"/\*.*?\*/", "", older[name], flags=re.S)))) == counts[prefix], name
    nm = subprocess.run(["nm", "-D", "--defined-only", rg.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split() and " T " in l}
    assert {s for s in exported if s.startswith("rgh_")} == declared
    for prefix, n in counts.items():  # nothing new under the older prefixes
        assert len({s for s in exported if s.startswith(prefix)}) == n, prefix
    lib = ctypes.CDLL(rg.LIB_PATH)
    for name in NEW_NAMES:
        assert hasattr(lib, name) and name in E.SYMBOLS, name
    rs = open(os.path.join(ROOT, "bindings", "raftgroups_handoff.rs")).read()
    assert rs == gen_rust_bindings.generate_handoff()
    for path, gen in (("raftgroups.rs", gen_rust_bindings.generate), ("raftgroups_lead.rs", gen_rust_bindings.generate_lead), ("raftgroups_term.rs", gen_rust_bindings.generate_term),
                      ("raftgroups_vote.rs", gen_rust_bindings.generate_vote)):
        assert open(os.path.join(ROOT, "bindings", path)).read() == gen(), path
    rust = {m.group(1): m.group(2) for m in re.finditer(r"pub fn (rgh_\w+)\((.*?)\)(?: -> [^;]+)?;", rs)}
    assert set(rust) == declared
    for name in declared:
        c_args = [x for x in re.search(r"\b" + name + r"\s*\(([^()]*)\)\s*;", plain, flags=re.S).group(1).split(",") if x.strip() and x.strip() != "void"]
        assert len(c_args) == len([x for x in rust[name].split(",") if x.strip()]) == len(E.SYMBOLS[name][1]), name
    for needle in ("pub struct RghPromoteOut", "pub out: RgHandoffOut", "pub items: *mut RgSendItem", "pub count: *mut u32", "pub const RGH_HANDOFF_VERSION: u32 = 1;",
                   "host_items: *mut RgSendItem", "dev_out: *const RghPromoteOut", "use super::raftgroups::*;"):
        assert needle in rs, needle
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_bindings.py"), "--check"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lib.rgh_handoff_version.restype = ctypes.c_uint32
    assert lib.rgh_handoff_version() == int(re.search(r"#define RGH_HANDOFF_VERSION (\d+)u", hdr).group(1)) == E.HANDOFF_EXT_VERSION
    assert [f for f, _ in E.PromoteOut._fields_] == list(E.PROMOTE_OUT_FIELDS) and ctypes.sizeof(E.PromoteOut) == 48
    for method in ("follow_promote_send", "follow_promote_send_device"):
        assert callable(getattr(E.Engine, method)), method
    assert (E.ABI_VERSION, E.LEAD_VERSION, E.TERM_VERSION, E.VOTE_VERSION) == (12, 1, 1, 1)


def test_api_refusals_are_host_checks():
    """What the two calls refuse is decided on the host, before anything is staged or launched: the state checks stand in front of
    RG_ENTER_STEP (which refuses unresolved host hints where every next step does), the record walk and the mirror's rule in front
    of the staging; every int entry point is a function-try-block that ends in RG_ABI_GUARD; rg_follow_promote* still refuses engines
    with device Inflights; the new arithmetic's header needs no HIP; the kernels call rg_handoff_promote_one and copy none of it."""
    csrc = os.path.join(ROOT, "raft_rs_amd", "csrc")
    src = open(os.path.join(csrc, "ext_handoff.hip")).read()
    for fn, needles in (("rgh_follow_promote", ("rgh_promote_state", "rg_walk_pairs", "RG_ERR_SLOT_BUSY", "rg_handoff_first_queued", "!n_items", "item_cap && !host_items")),
                        ("rgh_follow_promote_device", ("rgh_promote_state", "h->host_mirror", "rg_handoff_out_complete", "!dev_out->count", "dev_out->item_cap && !dev_out->items"))):
        body = src[src.index('extern "C" int %s(' % fn):]
        body = body[:body.index("} RG_ABI_GUARD")]
        assert ") try {" in body[:700], fn
        enter = body.index("RG_ENTER_STEP(h")
        assert "RG_ENTER(h)" not in body
        for needle in needles:
            assert 0 <= body.find(needle) < enter, (fn, needle)
        for later in ("rg_stage_reserve", "hipMemsetAsync", "RGH_LAUNCH", "rg_follow_round_trip", "rg_handoff_promoted"):
            assert body.find(later) == -1 or body.find(later) > enter, (fn, later)
        assert "rg_handoff_promoted(h)" in body
    state = src[src.index("static int rgh_promote_state"):src.index("// One launch of kernel<P, IX>")]
    for needle in ("!h->ins_arena", "rg_follow_promote", "rg_elect_enabled", "rg_send_check", "h->send_ready", "RG_ERR_STATE"):
        assert needle in state, needle
    assert state.index("!h->ins_arena") < state.index("rg_elect_enabled") < state.index("rg_send_check") < state.index("h->send_ready")
    step = open(os.path.join(csrc, "rg_engine.h")).read()
    step = step[step.index("#define RG_ENTER_STEP"):step.index("// The one switch on the slot count")]
    assert "rg_require_hints_resolved" in step
    check = open(os.path.join(csrc, "abi_tick.hip")).read()
    check = check[check.index("int rg_send_check("):check.index("// The pre-pass of a tick whose messages")]
    assert "RG_SEND_BYTES" in check and "!h->esz" in check and "unknown flags" in check
    older = open(os.path.join(csrc, "abi_handoff.hip")).read()
    assert "h->ins_arena" in older[older.index("static int rg_handoff_promote_state"):older.index("// ... and what a promotion leaves behind")]
    for unit in ("send_items", "send_cols", "send_last_dense", "stage_max_entries", "stage_flags", "send_counter", "rg_list_stage_ran", "send_bound"):
        assert unit not in src, unit  # the engine's send-stage bookkeeping is not this unit's
    assert "h->send_ready = " not in src
    kernels = open(os.path.join(csrc, "rg_kernels_promote.h")).read()
    code = re.sub(r"//.*", "", kernels)
    assert "rg_handoff_promote_one<IX>(" in code and "__restrict__" not in code and code.count("atomicAdd(") == 1 and "__syncthreads_or(" in code
    assert "rg_handoff_promote_check" not in code and "rg_handoff_import" not in code and "rg_handoff_become_leader" not in code
    header = open(os.path.join(csrc, "rg_promote.h")).read()
    assert '#include "rg_handoff.h"' in header and "hip" not in re.sub(r"//.*", "", header).lower()
    build = open(os.path.join(ROOT, "raft_rs_amd", "build.py")).read()
    assert '"ext_handoff.hip"' in build and '"rg_promote.h"' in build and '"rg_kernels_promote.h"' in build and "raftgroups_handoff.h" in build


# ---------------------------------------------------------------------------------------------------------------------
# 6. kernel resources
# ---------------------------------------------------------------------------------------------------------------------
def test_no_instantiation_carries_scratch():
    """tools/kernel_resources.py over ext_handoff.hip: exactly k_promote_send_list and k_promote_send_dense, every slot count x
    both index widths, no scratch (the resource metadata of the code objects; the instruction text is not searched)."""
    if not os.path.exists(shutil.which("hipcc") or "/opt/rocm/bin/hipcc"):
        pytest.fail("hipcc is needed (the engine is built with it)")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--src=raft_rs_amd/csrc/ext_handoff.hip"], cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines()[1:]:
        m = re.match(r"(\S.*?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)$", line)
        if m:
            rows[m.group(1)] = (int(m.group(2)), int(m.group(5)), int(m.group(6)))
    want = sorted("%s<%d, %s>" % (k, p, ix) for k in ("k_promote_send_list", "k_promote_send_dense") for p in range(1, 9) for ix in ("unsigned int", "unsigned long"))
    assert sorted(rows) == want, (sorted(rows), out.stderr[-1000:])
    for k, (vgpr, scratch, lds) in rows.items():
        print(k, vgpr, scratch, lds)
        assert scratch == 0 and lds <= 512 and vgpr <= 128, (k, vgpr, scratch, lds)
