"""Host build of the temporal-coherence learning-rate rule (r48_ntuple.h: nt_mean, nt_tc_rate,
nt_tc_update, nt_tc_rate_mean) vs a naive double-precision restatement (CPU).

Compiles tests/native/ntuple_tc_test.cpp with g++ (the same header the gfx950 kernels include) and
runs it: A == 0 gives rate 1 and the table increment of plain apply bit for bit; a run of same-sign
means keeps |E| == A bit for bit and the rate exactly 1; alternating signs drive the rate down
monotonically; mean == 0 leaves the table, E and A unchanged; the clamp holds with |E| set above A
by hand; the mean rate over a board's hits equals the naive mean.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tc_rule_matches_the_naive_restatement(tmp_path):
    exe = tmp_path / "ntuple_tc_test"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "ntuple_tc_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK (0 failures)" in r.stdout
