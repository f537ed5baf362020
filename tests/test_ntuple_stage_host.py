"""Host build of the multi-stage n-tuple contract (r48_ntuple.h: nt_stage, the staged nt_value and
nt_search_board, nt_staged_update_pull) vs the naive restatement in tests/native (CPU).

Compiles tests/native/ntuple_stage_test.cpp with g++ (the same header the gfx950 kernels include) and
runs it: nt_stage on boards whose largest tile is at each cut - 1, cut, cut + 1, at 15 and at 16..18
(the clamp) for cuts (15), (1) and (1, 2, 3); the staged value reads the board's stage block and the
search the afterstate's stage; the update's pull form (the header) and push form (what the kernels
run, restated naively) agree bitwise on every resolved entry over a few hundred random update calls
(L = 2 and 3, m = 1 and 2, S = 2 and 4, with and without TC) and the invariant holds after every call;
a first hit of (1, e) beside a hit of (0, e) starts from the pre-call tables[0][e]; a three-stage
chain with (1, e) owned and (2, e) not. The program is built and run once more under
-fsanitize=address,undefined.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "ntuple_stage_test.cpp")


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")],
                         ids=["plain", "sanitized"])
def test_stage_contract_matches_the_naive_restatement(tmp_path, flags):
    exe = tmp_path / "ntuple_stage_test"
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-o", str(exe), SRC])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK (0 failures)" in r.stdout
