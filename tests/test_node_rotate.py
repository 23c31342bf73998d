"""node_sums' loop forms agree bit for bit on the host (no GPU).

tests/native/node_rotate.cpp compiles gqmap_math.h as the CPU model does and
runs node_sums<0, true, false> (the straight loop) against the pipelined loop
(plain and with four trips per pass) and its rotated forms (the rotation, the
root in stages between the tap rows, that with two trips per pass) on a 24x24 integer frame padded as the engine pads it, with means and sigmas
that put samples on both sides of the clamps; K = 2, 3, 9; (k0, dk) = (0, 1),
(1, 2), (3, 4), a lane with exactly one sample and a lane with none; double
and float.  The six sums must be identical bits in every case.
"""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
SRC = os.path.join(NATIVE, "node_rotate.cpp")
HDR = os.path.join(os.path.dirname(HERE), "gqmap-opticalflow_amd", "csrc", "gqmap_math.h")
FORMS = ("pf", "pf4", "rot", "staged", "staged2")
LINE = re.compile(r"^(double|float) K=(\d+) k0=(\d+) dk=(\d+) samples=(\d+) form=(\S+) nodes=(\d+) clamped=(\d+) "
                  r"mismatches=(\d+)$")


@pytest.fixture(scope="module")
def cases():
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    out = os.path.join(NATIVE, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "node_rotate")
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
    seen = {(t, int(K), int(k0), int(dk), form) for t, K, k0, dk, _, form, *_ in rows}
    want = set()
    for t in ("double", "float"):
        for K in (2, 3, 9):
            for k0, dk in ((0, 1), (1, 2), (3, 4), (K * K - 1, 16), (K * K, 16)):
                want |= {(t, K, k0, dk, f) for f in FORMS}
    assert seen == want
    for t, K, k0, dk, samples, form, nodes, clamped, _ in rows:
        K2, k0, dk = int(K) ** 2, int(k0), int(dk)
        assert int(samples) == len(range(k0, K2, dk))
        # samples on both sides of the clamps: some nodes clamped, some not
        assert 0 < int(clamped) < int(nodes)
    assert {int(r[4]) for r in rows} >= {0, 1, 2, 4, 9, 81}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("typ", ["double", "float"])
def test_sums_match_the_straight_loop_bit_for_bit(cases, typ, form):
    _, rows = cases
    mine = [r for r in rows if r[0] == typ and r[5] == form]
    assert len(mine) == 15
    bad = [r for r in mine if int(r[8]) != 0]
    assert not bad, bad


def test_program_reports_success(cases):
    assert cases[0] == 0
