"""Host build of the TD step's arithmetic (r48_ntuple.h: nt_td_delta, nt_fixed_delta) vs a naive
double-precision restatement (CPU).

Compiles tests/native/ntuple_td_test.cpp with g++ (the same header the gfx950 kernels include) and
runs it: a prev_done row has target 0; zero rewards and negative values; reward + value rounds to
fp32 before prev_value is subtracted; the fixed-point word at and beyond +-2^20 and at the ties of
d * 65536, which go to the even neighbour; random cases of both bit for bit.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_td_delta_and_fixed_point_match_the_naive_restatement(tmp_path):
    exe = tmp_path / "ntuple_td_test"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "ntuple_td_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK (0 failures)" in r.stdout
