"""Host build of the n-tuple network's play contract (r48_ntuple.h: nt_play_board, the written
definition of what r48_ntuple_play computes) vs an explicit loop over nt_search_board, step_draw and
step_board (CPU).

Compiles tests/native/ntuple_play_test.cpp with g++ (the same header the gfx950 kernels include) and
runs it: layouts 3x3 and lines-squares, float and integer tables, depths 1 and 2, an even and an odd
board id, step counters 0 and 0xFFFFFFF0 (the uint32 add wraps), n_steps 0, 1 and 300, bit for bit in
the board, length, gain and done. A board without a move comes back unchanged with length and gain
untouched and done 1; a game played to its end in chunks has counted its changing steps and summed
its StepOut rewards.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ntuple_play_board_equals_the_explicit_loop(tmp_path):
    exe = tmp_path / "ntuple_play_test"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "ntuple_play_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK (0 failures)" in r.stdout
