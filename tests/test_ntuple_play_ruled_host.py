"""Host build of the n-tuple network's ruled play contract (r48_ntuple.h: nt_play_board_ruled, the
written definition of what r48_ntuple_play_ruled computes) vs an explicit loop over nt_search_board
at rule[the board's zero bytes], step_draw and step_board (CPU).

Compiles tests/native/ntuple_play_ruled_test.cpp with g++ (the same header the gfx950 kernels include)
and runs it: layouts 3x3 and lines-squares, float and integer tables; the rules all-1 and all-2 (which
must also equal nt_play_board at depths 1 and 2), all-3 and a mixed rule that uses all four depths,
depth 4 at no more than one blank; an even board id at step counter 0 and an odd one at 0xFFFFFFF0 (the
uint32 add wraps), n_steps 0, 1 and 24, bit for bit in the board, length, gain and done; chunked calls
add up; a board without a move comes back unchanged with length and gain untouched and done 1.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ntuple_play_board_ruled_equals_the_explicit_loop(tmp_path):
    exe = tmp_path / "ntuple_play_ruled_test"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "ntuple_play_ruled_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK (0 failures)" in r.stdout
