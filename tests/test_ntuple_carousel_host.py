"""Host build of the carousel-shaping contract (r48_ntuple.h: nt_carousel_host over nt_stage,
nt_carousel_turn and nt_carousel_donor) vs a naive restatement in tests/native (CPU).

Compiles tests/native/ntuple_carousel_test.cpp with g++ (the same header the gfx950 kernels include)
and runs it: the header's loop against the restatement (the stage cell by cell, Philox4x32-10 from the
paper, every board decided from a copy of the state before the call) over 1,080 random calls in
chains of 40 -- S = 2, 3, 4, n = 1, 2, 65, gid0 small and 2^32 + 5, ctr up to its wrap, boards with
their largest tile around the cuts, at 15..18 and empty, any non-zero done byte -- and the named cases:
the board's own slot as donor; a donor slot that records in the same call (the old content is read,
and an empty slot filled in the same call is still empty to the restart); the fallback to stage 0 and
the next restart trying stage 1 again; turn wrapping from S - 1 to 0; a board that crosses a cut
records and one already at seen does not; a done board never records; tiles of 15..18 against cut 15
and cuts (3, 4, 6); the draw for (seed, gid, ctr) against a pinned Philox4x32-10 word and the donors it
gives for n = 1, 65, 257 and 2^31 - 1. The program is built and run once more under
-fsanitize=address,undefined.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "ntuple_carousel_test.cpp")


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")],
                         ids=["plain", "sanitized"])
def test_carousel_contract_matches_the_naive_restatement(tmp_path, flags):
    exe = tmp_path / "ntuple_carousel_test"
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-o", str(exe), SRC])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK (0 failures)" in r.stdout
