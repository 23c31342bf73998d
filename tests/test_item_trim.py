"""The trimmed dataflow item's address forms on the host (no GPU).

The fp64 mixture item on the offset store (k_iter_flow<double, vvo2_t, 0, 1>)
reads its taps through biased bases (gqmap_math.h TapViewLutBiased: a cell is
iy + M2 ix, the second column pair on a base of its own) and loads its edge
operands at 32-bit element offsets where edge_addr32_ok holds.  Neither
changes an operand.  tests/native/item_trim.cpp compiles gqmap_math.h as the
CPU model does (the harness of tests/test_tap_lut.py) and runs

  * every cell (iy, ix) of [1, Mo] x [1, No] at 40 x 56 and 388 x 584: the
    biased index on the biased bases addresses cell_elem's elements and those
    2 M2 further, inside the buffer -- cell (1, 1) at its first element, cell
    (Mo, No) reaching the zero column -- and returns load_taps16's taps;
  * the 32-bit element offset against the 64-bit index for planes 0..8 at
    every node of C2's grid and of the largest grid the host gives the 32-bit
    form (M N = 2^24 - 1), and with L = 3; the sizes just above take the
    64-bit form;
  * node_sums_lut through the biased view against the present view, clamped
    and clamp-free, 1 and 4 trips per pass, K = 2, 9, 16: the six sums bit for
    bit.

The exact partial sums (fix128, integers modulo 2^128) reduced over a wave in
the DPP order of wave_sum_fix3_dpp (gqmap_engine.hip, GQ_FIXSUM_DPP) against
the xor butterfly of wave_sum_fix, both modelled here on 32-bit limbs with
their carries: random values, and values whose sums carry across each of the
three limb boundaries and through all of them.
"""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
SRC = os.path.join(NATIVE, "item_trim.cpp")
HDR = os.path.join(os.path.dirname(HERE), "gqmap-opticalflow_amd", "csrc", "gqmap_math.h")
KS = (2, 9, 16)
BIAS = re.compile(r"^bias Mo=(\d+) No=(\d+) cells=(\d+) last_byte_slack=(\d+) mismatches=(\d+)$")
ADDR = re.compile(r"^addr M=(\d+) N=(\d+) L=(\d+) checks=(\d+) mismatches=(\d+)$")
OK = re.compile(r"^ok M=(\d+) N=(\d+) L=(\d+) bytes=(\d+) ok=([01])$")
NODE = re.compile(r"^node K=(\d+) sets=(\d+) clamped_samples=(\d+) free_sets=(\d+) mismatches=(\d+)$")


@pytest.fixture(scope="module")
def cases():
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    out = os.path.join(NATIVE, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "item_trim")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        # the flags of the CPU model (tests/native/Makefile, oracle/Makefile): explicit fma only
        subprocess.run([cxx, "-O1", "-std=c++17", "-mfma", "-ffp-contract=off", "-Wall", "-o", exe, SRC],
                       check=True, capture_output=True, text=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    got = {}
    for key, rx in (("bias", BIAS), ("addr", ADDR), ("ok", OK), ("node", NODE)):
        ms = [rx.match(l) for l in r.stdout.splitlines() if l.startswith(key + " ")]
        assert ms and all(ms), r.stdout + r.stderr
        got[key] = [tuple(map(int, m.groups())) for m in ms]
    assert sum(map(len, got.values())) == len(r.stdout.splitlines()), r.stdout
    return r.returncode, got


def test_program_reports_success(cases):
    assert cases[0] == 0


@pytest.mark.parametrize("Mo,No", [(40, 56), (388, 584)])
def test_biased_bases_address_the_cells_elements(cases, Mo, No):
    mine = [r for r in cases[1]["bias"] if r[:2] == (Mo, No)]
    assert len(mine) == 1
    _, _, cells, slack, bad = mine[0]
    assert cells == Mo * No and bad == 0, mine
    # the tail past cell (Mo, No)'s last element: a column less one element, and VV_TAIL
    assert slack == 4 * ((Mo + 2) + 8 - 1)


@pytest.mark.parametrize("M,N,L,every", [(388, 584, 1, True), (4095, 4097, 1, True), (1023, 1025, 3, False)])
def test_32_bit_element_offsets_equal_the_64_bit_index(cases, M, N, L, every):
    mine = [r for r in cases[1]["addr"] if r[:3] == (M, N, L)]
    assert len(mine) == 1
    checks, bad = mine[0][3:]
    assert bad == 0, mine
    assert checks == 9 * M * N * L if every else checks >= 9 * 25 * L


def test_host_bound_of_the_32_bit_form(cases):
    ok = {r[:4]: r[4] for r in cases[1]["ok"]}
    assert ok[(388, 584, 1, 8)] == 1
    # the largest: M N L = 2^24 - 1 (a buffer of 9 planes is then 1.2 GB, below 4 GiB)
    assert 4095 * 4097 == 2 ** 24 - 1 and ok[(4095, 4097, 1, 8)] == 1
    assert ok[(4096, 4096, 1, 8)] == 0 and ok[(4095, 4098, 1, 8)] == 0
    assert ok[(1023, 1025, 4, 8)] == 1 and ok[(1024, 1024, 4, 8)] == 0
    assert ok[(16777215, 1, 1, 8)] == 1 and ok[(16777216, 1, 1, 8)] == 0


def test_every_node_case_ran(cases):
    node = cases[1]["node"]
    assert [K for K, *_ in node] == list(KS)
    for K, sets, clamped, free, _ in node:
        assert sets >= 200 and clamped >= 100 * K and free >= sets // 5


@pytest.mark.parametrize("K", KS)
def test_node_loop_through_the_biased_view_bit_for_bit(cases, K):
    mine = [r for r in cases[1]["node"] if r[0] == K]
    assert len(mine) == 1 and mine[0][4] == 0, mine


# --- the wave reductions of a fix128 on four 32-bit limbs ---
M32, M128 = (1 << 32) - 1, (1 << 128) - 1


def _limbs(v):
    return [(v >> (32 * k)) & M32 for k in range(4)]


def _add128(src, own):
    """v_add_co_u32 then three v_addc_co_u32 on the limbs of src + own."""
    out, carry = [], 0
    for a, b in zip(src, own):
        s = a + b + carry
        out.append(s & M32)
        carry = s >> 32
    return out


def _butterfly(vals):
    """wave_sum_fix: v += shfl_xor(v, o), o = 32 .. 1; every lane ends with the total."""
    x = [_limbs(v) for v in vals]
    for o in (32, 16, 8, 4, 2, 1):
        x = [_add128(x[i ^ o], x[i]) for i in range(64)]
    return x


def _dpp(vals):
    """wave_sum_fix3_dpp: row_shr 1, 2, 4, 8 (no source lane: 0), row_bcast:15 into
    rows 1 and 3, row_bcast:31 into rows 2 and 3; lane 63 ends with the total."""
    x = [_limbs(v) for v in vals]
    zero = [0, 0, 0, 0]
    for n in (1, 2, 4, 8):
        x = [_add128(x[i - n] if i % 16 >= n else zero, x[i]) for i in range(64)]
    x = [_add128(x[16 * (i // 16) - 1], x[i]) if (i // 16) in (1, 3) else x[i] for i in range(64)]
    x = [_add128(x[31], x[i]) if (i // 16) in (2, 3) else x[i] for i in range(64)]
    return x


def _fix128_cases():
    import random
    rng = random.Random(20240)
    cases = [[rng.getrandbits(128) for _ in range(64)] for _ in range(20)]
    cases += [[(-rng.getrandbits(90)) & M128 if rng.random() < 0.5 else rng.getrandbits(90) for _ in range(64)]
              for _ in range(20)]  # signed sums of the engine's size: both signs, the total of either sign
    for k in (1, 2, 3):  # a carry across limb boundary k alone: all ones below it, plus one
        cases.append([(1 << (32 * k)) - 1] + [1] + [0] * 62)
        cases.append([0] * 62 + [1] + [(1 << (32 * k)) - 1])
        cases.append([((1 << (32 * k)) - 1) // 64 + 1] * 64)
    cases.append([M128 >> 1] + [1] * 63)  # through all three boundaries
    cases.append([M32, M32 << 32, M32 << 64, 1] * 16)
    cases.append([M128] * 64)  # 64 x (-1)
    return cases


@pytest.mark.parametrize("case", range(len(_fix128_cases())))
def test_dpp_reduction_order_equals_the_butterfly(case):
    vals = _fix128_cases()[case]
    want = _limbs(sum(vals) & M128)
    b, d = _butterfly(vals), _dpp(vals)
    assert all(lane == want for lane in b)
    assert d[63] == want
    # rows' totals on the way: lane 15 row 0, lane 31 rows 0-1
    assert d[15] == _limbs(sum(vals[:16]) & M128) and d[31] == _limbs(sum(vals[:32]) & M128)
