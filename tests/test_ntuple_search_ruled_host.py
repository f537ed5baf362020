"""Host build of the n-tuple network's per-board search at depth 4 and of the ruled wrapper
(r48_ntuple.h: nt_search_board over nt_best / nt_q_level, nt_rule_depth, nt_search_board_ruled, the
contract k_nt_search_ruled shares its arithmetic with) vs a naive float64 restatement (CPU).

Compiles tests/native/ntuple_search4_test.cpp with g++ (the same header the gfx950 kernels include)
and runs it: layouts 3x3 and lines-squares, float and integer tables, 20 random boards of at most 3
blanks each (exponents up to 17) and six crafted crowded ones (no move, boards one and two spawns
away from game over, a full board with two moves, a fully symmetric one, a 2^18 reward). The
restatement uses explicit 4x4 arrays, its own line-by-line move, plain recursion and float64, and carries the 3-ply test's rounding bound one level further (derived at the top of the
program). Legal sets are exact, q is within the bound, the action is a maximiser of the float64 Q
within it; depths 1 to 3 keep their bits (each depth is recomposed from calls one depth down); the
ruled wrapper equals nt_search_board at rule[blanks] per board under three rules.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ntuple_search4_and_the_ruled_wrapper_match_the_naive_restatement(tmp_path):
    exe = tmp_path / "ntuple_search4_test"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "ntuple_search4_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK (0 failures)" in r.stdout
