"""Host build of the legal-move board logic (r48_board.h: legal_mask, move_rows<A>, move_rows4) vs
the C oracle (CPU).

Compiles tests/native/moves_logic_test.cpp with g++ (the same source the gfx950 kernels include)
and runs: legal_mask against "the oracle's move changed the board" exhaustively over all 18^4
lines in every row and column of an otherwise empty board, then on 400k random boards (exponents
0..17, nearly empty to full) legal_mask, the templated move helper with its merge reward, the
four-moves-at-once helper, and legal == 0 against the oracle's game over; the empty board.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_moves_logic_matches_oracle(tmp_path):
    orc = tmp_path / "orc.o"
    exe = tmp_path / "moves_logic_test"
    subprocess.check_call(["gcc", "-O2", "-std=c11", "-c", "-o", str(orc), os.path.join(ROOT, "oracle", "r48_oracle.c")])
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "moves_logic_test.cpp"), str(orc)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK (0 failures)" in r.stdout
