"""Host build of the n-tuple network's header (r48_ntuple.h: nt_expand, nt_pack, nt_index, nt_entry,
nt_value) vs a naive restatement (CPU).

Compiles tests/native/ntuple_logic_test.cpp with g++ (the same header the gfx950 kernels include)
and runs it: for five layouts (both named ones, a 3 x 3-tuple one, the smallest and the largest the
contract allows) the 8 entry indices of every tuple equal those of eight explicit board transforms
indexed cell by cell, and the value sum over integer tables equals the naive sum, on 100k random
boards with exponents 0..18, the empty board, a fully symmetric board (all 8 hits equal) and the
clamp at 16, 17 and 18; plus the layouts nt_expand must refuse.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ntuple_logic_matches_the_naive_restatement(tmp_path):
    exe = tmp_path / "ntuple_logic_test"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "ntuple_logic_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK (0 failures)" in r.stdout
