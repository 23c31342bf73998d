"""edge_sums_range carried over the halo chain's four slices equals edge_sums (no GPU).

tests/native/halo_chain.cpp compiles gqmap_math.h as the CPU model does and
runs an edge's pair range cut as the dataflow item cuts it -- four consecutive
slices, each continuing the six sums the one before left in memory, the centre
point with the last -- against edge_sums in one piece, for two cuts: four
equal slices [np w / 4, np (w + 1) / 4) and the kernel's own (chain_cut with
its shorter last slice).  K = 2 (two pairs, no centre; two empty slices of the
equal cut, three of the kernel's), 3, 4, 9, 11 and 16, double and float, 400
random operand sets each, half of them with the correlation at or next to its
clamps.  The six sums must be identical bits.
"""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
SRC = os.path.join(NATIVE, "halo_chain.cpp")
HDR = os.path.join(os.path.dirname(HERE), "gqmap-opticalflow_amd", "csrc", "gqmap_math.h")
KS = (2, 3, 4, 9, 11, 16)
LINE = re.compile(r"^(double|float) K=(\d+) pairs=(\d+) centre=(\d) empty_slices=(\d) empty_kernel=(\d) sets=(\d+) near_corr=(\d+) "
                  r"mismatches=(\d+)$")


@pytest.fixture(scope="module")
def cases():
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    out = os.path.join(NATIVE, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "halo_chain")
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
    for _, K, pairs, centre, empty, empty_k, sets, near, _ in rows:
        K = int(K)
        assert int(pairs) == K * K // 2 and int(centre) == K % 2
        assert int(empty) == (2 if K == 2 else 0)
        cut = [min(K * K // 2, (K * K // 2 + 8) * w // 4) for w in range(5)]  # chain_cut at GQ_FLOW_HALO_EPI = 8
        assert int(empty_k) == sum(a == b for a, b in zip(cut, cut[1:])) == {2: 3, 3: 2, 4: 2}.get(K, 0)
        assert int(sets) >= 300 and int(near) >= int(sets) // 4


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("typ", ["double", "float"])
def test_chain_matches_edge_sums_bit_for_bit(cases, typ, K):
    _, rows = cases
    mine = [r for r in rows if r[0] == typ and int(r[1]) == K]
    assert len(mine) == 1
    assert int(mine[0][8]) == 0, mine


def test_program_reports_success(cases):
    assert cases[0] == 0
