"""The offset store's arithmetic on the host (no GPU): taps by table against
taps by conversion.

tests/native/tap_lut.cpp compiles gqmap_math.h as the CPU model does and runs

  * node_sums on the offset store (vvo2_t through a TapViewLut: node_sums_lut,
    its trips written out 1 and 4 per pass) against node_sums' pipelined loop
    on a float store of the same integer frame -- 240 nodes per K on six
    random frames with values over the whole table range [-510, 765], sigma
    up to the cap (thousands of clamped samples per K) and a quarter of the
    nodes clamp-free, where both loops also run without the clamps -- for
    K = 2..16: the six sums must be identical bits;
  * every integer of [-510, 765] through taplut_offset and taplut_entry
    against the pair store's conversion chain (binary16 -> float -> double, the
    binary16 step in software), for three table origins each, and the form of
    the offsets (multiples of 8 below 8 TAPLUT_N).
"""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
SRC = os.path.join(NATIVE, "tap_lut.cpp")
HDR = os.path.join(os.path.dirname(HERE), "gqmap-opticalflow_amd", "csrc", "gqmap_math.h")
KS = tuple(range(2, 17))
NODE = re.compile(r"^node K=(\d+) sets=(\d+) clamped_samples=(\d+) free_sets=(\d+) mismatches=(\d+)$")
TABLE = re.compile(r"^table values=(\d+) mismatches=(\d+)$")


@pytest.fixture(scope="module")
def cases():
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    out = os.path.join(NATIVE, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "tap_lut")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        # the flags of the CPU model (tests/native/Makefile, oracle/Makefile): explicit fma only
        subprocess.run([cxx, "-O1", "-std=c++17", "-mfma", "-ffp-contract=off", "-Wall", "-o", exe, SRC],
                       check=True, capture_output=True, text=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    lines = r.stdout.splitlines()
    node = [NODE.match(l) for l in lines if l.startswith("node")]
    table = [TABLE.match(l) for l in lines if l.startswith("table")]
    assert node and all(node) and len(table) == 1 and table[0] and len(node) + 1 == len(lines), r.stdout + r.stderr
    return r.returncode, [tuple(map(int, m.groups())) for m in node], tuple(map(int, table[0].groups()))


def test_every_case_ran(cases):
    _, node, table = cases
    assert [K for K, *_ in node] == list(KS)
    for K, sets, clamped, free, _ in node:
        assert sets >= 200 and clamped >= 100 * K and free >= sets // 5
    assert table[0] == 1276  # [-510, 765]


@pytest.mark.parametrize("K", KS)
def test_node_loop_on_the_offset_store_bit_for_bit(cases, K):
    _, node, _ = cases
    mine = [r for r in node if r[0] == K]
    assert len(mine) == 1 and mine[0][4] == 0, mine


def test_table_equals_the_conversion_chain(cases):
    assert cases[2][1] == 0, cases[2]


def test_program_reports_success(cases):
    assert cases[0] == 0


def test_offset_store_kernel_keeps_two_waves_without_scratch(tmp_path):
    """The item with the table (tests/test_occupancy.py's guard for the new
    kernel): at most 256 VGPRs, no AGPRs, no scratch in the built library."""
    from tests import test_occupancy as occ
    if not os.path.exists(occ.LIB) or not shutil.which(f"{occ.LLVM}/llvm-readelf"):
        pytest.skip("library or ROCm LLVM tools absent")
    regs = occ._kernel_registers(str(tmp_path))
    name = "_ZN2gq11k_iter_flowIdNS_6vvo2_tELi0ELi1ELb0ELi0EEEvNS_10IterParamsIT_T0_EEiPjiPKNS_3CtlE"
    assert name in regs, name
    v, a, scratch = regs[name]
    assert v <= 256 and a == 0 and scratch == 0, regs[name]
