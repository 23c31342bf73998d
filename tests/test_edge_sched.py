"""edge_sums_range_sched equals edge_sums bit for bit (no GPU).

tests/native/edge_sched.cpp compiles gqmap_math.h as the CPU model does and
runs the hand-scheduled pair loop of the trimmed dataflow item -- a pair's
table rows read a pair ahead, its two roots side by side; each part alone and
both -- against edge_sums on the same operands: the whole range from zero with
the centre point (edge_sums itself) and without it (edge_sums_range), and the
halo chain's four slices carried from slice to slice through memory, for four
equal slices and for the kernel's cut (GQ_FLOW_HALO_EPI = 0 and 8).  K = 2..16,
double and float, 400 operand sets each: random ones, half of them with the
correlation at or next to its clamps, and an eighth that make d exactly 0.
K = 2 gives empty slices, K = 3 one-pair slices; the table ends at row K^2 - 1
with a row of NaNs behind it, so a use of a row past the table shows in the
sums.  The six sums must be identical bits.
"""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
SRC = os.path.join(NATIVE, "edge_sched.cpp")
HDR = os.path.join(os.path.dirname(HERE), "gqmap-opticalflow_amd", "csrc", "gqmap_math.h")
KS = tuple(range(2, 17))
LINE = re.compile(r"^(double|float) K=(\d+) pairs=(\d+) centre=(\d) empty_slices=(\d) empty_kernel=(\d) one_pair_kernel=(\d) "
                  r"sets=(\d+) zero_d=(\d+) mismatches=(\d+)$")


@pytest.fixture(scope="module")
def cases():
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    out = os.path.join(NATIVE, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "edge_sched")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        # the flags of the CPU model (tests/native/Makefile, oracle/Makefile): explicit fma only
        subprocess.run([cxx, "-O1", "-std=c++17", "-mfma", "-ffp-contract=off", "-Wall", "-o", exe, SRC],
                       check=True, capture_output=True, text=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    rows = [LINE.match(l) for l in r.stdout.splitlines()]
    assert rows and all(rows), r.stdout + r.stderr
    return r.returncode, [m.groups() for m in rows]


def test_every_case_ran(cases):
    _, rows = cases
    assert {(t, int(K)) for t, K, *_ in rows} == {(t, K) for t in ("double", "float") for K in KS}
    for _, K, pairs, centre, empty, empty_k, one_k, sets, zero_d, _ in rows:
        K = int(K)
        np_ = K * K // 2
        assert int(pairs) == np_ and int(centre) == K % 2
        assert int(empty) == (2 if K == 2 else 0)
        cut = [min(np_, (np_ + 8) * w // 4) for w in range(5)]  # chain_cut at GQ_FLOW_HALO_EPI = 8
        assert int(empty_k) == sum(a == b for a, b in zip(cut, cut[1:]))
        assert int(one_k) == sum(b - a == 1 for a, b in zip(cut, cut[1:]))
        if K == 2:
            assert int(empty_k) == 3
        if K == 3:
            assert int(one_k) >= 1
        assert int(sets) >= 300 and int(zero_d) >= int(sets) // 8


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("typ", ["double", "float"])
def test_sched_matches_edge_sums_bit_for_bit(cases, typ, K):
    _, rows = cases
    mine = [r for r in rows if r[0] == typ and int(r[1]) == K]
    assert len(mine) == 1
    assert int(mine[0][9]) == 0, mine


def test_program_reports_success(cases):
    _, _ = cases
    assert cases[0] == 0
