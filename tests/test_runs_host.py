"""CPU only: csrc/rg_runs.h, the run cutter and the staging layout of the follower side's sparse calls, compiled for the HOST
with g++ (tests/host_check/runs_check.cpp, a stand-alone program). The cutter: n = 1, one group, sorted, reversed, interleaved
(stable within a run), group ids around 2^32 and 2^64 in one batch, and a seeded sweep against a plain reference, each with
run_start[0] == 0, run_start[runs] == n, strictly ascending starts, one group per run, groups ascending across runs and orig a
permutation. The layout: offsets on 256 bytes, empty regions, the unpadded total, and the offsets of the three call shapes equal
to the hand-chained expressions they replaced. Once plainly, once under AddressSanitizer (with LeakSanitizer) + UBSan."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def build_and_run(tmp_path, name, extra):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build the run cutter check")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "raft_rs_amd", "csrc"),
                           os.path.join(HERE, "host_check", "runs_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.returncode, r.stdout, r.stderr[-2000:])


def test_run_cutter_and_layout_contract(tmp_path):
    build_and_run(tmp_path, "runs_check", [])


def test_run_cutter_and_layout_are_clean_under_asan_and_ubsan(tmp_path):
    """The same program, -fsanitize=address,undefined -fno-sanitize-recover=all, run directly (a stand-alone executable)."""
    build_and_run(tmp_path, "runs_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
