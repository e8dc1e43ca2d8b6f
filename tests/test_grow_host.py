"""CPU only: csrc/rg_grow.h, the one grower of the engine's staging buffers (d_records, pin_records, the packed pair, d_cells),
compiled for the HOST with g++ over malloc / free (tests/host_check/grow_check.cpp, a stand-alone program): capacities at
need = first - 1, first, first + 1 and 4 * first + 1, no reallocation when the need fits, the padding bytes, and the contract
on a failed allocation -- (nullptr, 0), the old buffer freed, the next call recovers; for the pair, a failed second allocation
frees the first. Once plainly, once under AddressSanitizer (with LeakSanitizer) + UBSan."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def build_and_run(tmp_path, name, extra):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build the grower check")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "raft_rs_amd", "csrc"),
                           os.path.join(HERE, "host_check", "grow_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.returncode, r.stdout, r.stderr[-2000:])


def test_grower_contract(tmp_path):
    build_and_run(tmp_path, "grow_check", [])


def test_grower_is_clean_under_asan_and_ubsan(tmp_path):
    """The same program, -fsanitize=address,undefined -fno-sanitize-recover=all, run directly (a stand-alone executable)."""
    build_and_run(tmp_path, "grow_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
