"""Host build of r48::reset_lines and of k_step_n's auto-reset from the line-form table (CPU).

Compiles tests/native/reset_lines_test.cpp with g++ (the same r48_board.h the gfx950 kernels
include, with v_perm_b32 emulated) and runs: all 128 (action, cell, tile) table entries against the
transpose + select route and back to rows; the orientation-tracked random-policy loop with the
read-ahead selector and the table reset (4096 near-full boards x 300 steps) and the given-action
loop with bad bytes, both against step_board + reset_board on rows at every step. The same program
runs once more as a stand-alone ASan + UBSan binary.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "reset_lines_test.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_reset_lines_table_and_loop(tmp_path, flags):
    exe = tmp_path / "reset_lines_test"
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-o", str(exe), SRC])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK (0 failures)" in r.stdout
