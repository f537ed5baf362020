"""Host build of the n-tuple network's per-board search at depth 3 (r48_ntuple.h: nt_search_board
over nt_best / nt_q_level, the recursion k_nt_search3 shares its arithmetic with) vs a naive float64
restatement (CPU).

Compiles tests/native/ntuple_search3_test.cpp with g++ (the same header the gfx950 kernels include)
and runs it: layouts 3x3 and lines-squares, float and integer tables, 40 random boards each
(exponents up to 17) and nine crafted ones (no move, one tile with its 120 children, boards one and
two spawns away from game over, a fully symmetric one). The restatement uses explicit 4x4 arrays,
its own line-by-line move, plain recursion and float64, and carries the rounding bound up the tree
(derived at the top of the program). Legal sets are exact, q is within the bound, the action is a
maximiser of the float64 Q within it, and depths 1 and 2 keep the bits of the code they had.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ntuple_search3_matches_the_naive_restatement(tmp_path):
    exe = tmp_path / "ntuple_search3_test"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "ntuple_search3_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK (0 failures)" in r.stdout
