"""Host build of the n-tuple network's per-board search (r48_ntuple.h: nt_search_board, built from
the pieces k_nt_search runs per lane -- nt_leaf, nt_cell_term, nt_q2, nt_argmax4 -- and the cell sum
in the butterfly's order) vs a naive restatement (CPU).

Compiles tests/native/ntuple_search_test.cpp with g++ (the same header the gfx950 kernels include)
and runs it: layouts 3x3 and lines-squares, integer tables of spread 8 and 1, depth 1 and 2, on 300
random boards each (exponents up to 17) and eight crafted ones (no move, one tile, a board one spawn
away from game over, a fully symmetric one). The restatement uses explicit 4x4 arrays, its own
line-by-line move and float64. Actions and legal sets are exact; q is within 2 * 2^-23 * (|r_a| +
|S_a| / (10 |E|)), the division's and the last add's roundings -- everything before them is integer
arithmetic below 2^24, which the program checks per board.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ntuple_search_matches_the_naive_restatement(tmp_path):
    exe = tmp_path / "ntuple_search_test"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "ntuple_search_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK (0 failures)" in r.stdout
