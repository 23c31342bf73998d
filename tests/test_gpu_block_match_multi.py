"""gqmap_block_match_multi (HIP kernel) against gqmap_block_match_multi_host:
one header (csrc/gqmap_blockmatch.h) behind both, so flow and cost agree BIT
FOR BIT, ties and the NaN pattern of missing ranks included; the host model
itself is checked against numpy in tests/test_block_match_multi.py.  Then
gqmap_init_state_flows (one flow per mixture component) against its host
formula, and one short solve seeded from all three ranks."""
import ctypes as C

import numpy as np
import pytest

from tests import _blockmatch_gpu as BG
from tests import _blockmatch_np as R
from tests._blockmatch_gpu import KEYS, as_fp32, assert_bit_equal, assert_state_equal, flows, force_cols, problem

pytestmark = pytest.mark.gpu


def both(A, B, params, H, sep):
    return BG.both(A, B, params, hypotheses=H, sep=sep)


@pytest.mark.parametrize("params", R.PARAMS, ids=str)
@pytest.mark.parametrize("crop", R.CROPS, ids=str)
def test_kernel_equals_host_model(crop, params):
    assert_bit_equal(*both(*R.crop_pair(crop), params, 3, 2))


@pytest.mark.parametrize("crop,params,H,sep", [(R.CROPS[0], (7, 7, 3, 1.7), 4, 1), (R.CROPS[3], (7, 7, 3, 1.7), 2, 3),
                                               (R.CROPS[4], (1, 1, 1, 0.8), 4, 2),  # 3 x 3 window: ranks run out, pixel by pixel
                                               (R.CROPS[0], (32, 32, 4, 2.0), 3, 2)],  # the largest LDS window
                         ids=str)
def test_other_hypothesis_counts_and_the_largest_window(crop, params, H, sep):
    assert_bit_equal(*both(*R.crop_pair(crop), params, H, sep))


@pytest.mark.parametrize("cols", [0, 8, 16, 32])
def test_several_tiles_with_partial_tiles_at_every_tile_width(cols):
    """97 x 130 (tests/test_gpu_block_match.py): four tile rows, the last tile
    of each row and column partial; 8, 16, 32 force each instantiation of the
    new kernel.  Rank 0 is the single-hypothesis kernel's result, bit for bit."""
    from gqmap_opticalflow_amd import block_match
    I1, I2, _ = R.rubberwhale()
    A, B = (np.asfortranarray(a[60:157, 210:340]) for a in (I1, I2))
    try:
        force_cols(cols)
        dev, host = both(A, B, (7, 7, 3, 1.7), 3, 2)
        assert_bit_equal(dev, host)
        assert_bit_equal((dev[0][..., 0], dev[1][..., 0]), block_match(A, B, 7, 7, 3, 1.7))
    finally:
        force_cols(0)


@pytest.mark.parametrize("shape", [(1, 1), (64, 1), (1, 64)], ids=str)
def test_degenerate_images(shape):
    I1, I2, _ = R.rubberwhale()
    M, N = shape
    A, B = (np.asfortranarray(a[120:120 + M, 250:250 + N]) for a in (I1, I2))
    assert_bit_equal(*both(A, B, (7, 7, 3, 1.7), 3, 2))


def test_missing_ranks_and_elapsed_ms():
    from gqmap_opticalflow_amd import block_match
    z = np.zeros((16, 16))
    flow, cost, ms = block_match(z, z, 1, 1, 1, 1.0, hypotheses=3, sep=3, timed=True)
    assert np.isfinite(ms) and ms > 0
    assert np.all(flow[:, :, :, 0] == 1) and np.all(cost[:, :, 0] == 0)
    assert np.all(flow[:, :, :, 1:].view(np.uint64) == 0x7FF8000000000000) and np.all(np.isposinf(cost[:, :, 1:]))


# ---- gqmap_init_state_flows ---------------------------------------------------

@pytest.mark.parametrize("engine,precision,H", [("mixture", "fp64", 3), ("mixture", "fp64", 2), ("mixture", "fp32", 3),
                                                ("super", "fp64", 3)])
def test_device_state_equals_host_formula(engine, precision, H):
    """Components l < H are the clamped slices (through float32 in fp32), NaN
    and unknown entries and every other plane are init_state's; the host
    formula (initial_state) says the same and tests/test_block_match_multi.py
    checks it entry by entry."""
    from gqmap_opticalflow_amd import Engine, initial_state
    I1, I2, o, (M, N) = problem(engine)
    f = flows(M, N, H, seed=11)
    with Engine(o, I1, I2, engine, precision) as e:
        assert (e.M, e.N, e.L) == (M, N, 3)
        e.init_state_from_flow(f, seed=7)
        got = e.get_state()
        e.init_state(7)  # the plain init keeps its bits
        plain = e.get_state()
    want, base = initial_state(o, M, N, seed=7, flow=f), initial_state(o, M, N, seed=7)
    if precision == "fp32":
        want, base = as_fp32(want), as_fp32(base)
    assert_state_equal(got, want, "flows init")
    assert_state_equal(plain, base, "plain init")
    for l in range(3):
        same = np.array_equal(got.muu[:, :, l], plain.muu[:, :, l])
        assert same == (l >= H), f"component {l}"
    # directly, without the host formula: slice 1 clamped, NaN keeps the draw
    x = np.clip(f[:, :, 0, 1], o["minu"], o["maxu"])
    x = x.astype(np.float32).astype(np.float64) if precision == "fp32" else x
    known = ~(np.isnan(f[:, :, 0, 1]) | (np.abs(f[:, :, 0, 1]) > 1e9))
    assert np.array_equal(got.muu[:, :, 1][known], x[known])
    assert np.array_equal(got.muu[:, :, 1][~known], plain.muu[:, :, 1][~known]) and not known[5, 4]


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_one_hypothesis_is_the_three_dimensional_call(precision):
    from gqmap_opticalflow_amd import Engine
    I1, I2, o, (M, N) = problem("mixture")
    f = flows(M, N, 1, seed=3)
    with Engine(o, I1, I2, "mixture", precision) as e:
        e.init_state_from_flow(f, seed=5)
        a = e.get_state()
        e.init_state_from_flow(np.asfortranarray(f[:, :, :, 0]), seed=5)
        b = e.get_state()
    assert_state_equal(a, b, "H = 1")


def test_two_tiles_take_their_columns_of_the_full_flows():
    from gqmap_opticalflow_amd import Engine, initial_state
    I1, I2, o, (M, N) = problem("mixture")
    f = flows(M, N, 3, seed=9)
    want = initial_state(o, M, N, seed=4, flow=f)
    tiles = [Engine(o, I1, I2, n_tiles=2, tile=t) for t in range(2)]
    try:
        cols = 0
        for t in tiles:
            t.init_state_from_flow(f, seed=4)
            got = t.get_state()
            for k in KEYS[:6]:
                np.testing.assert_array_equal(getattr(got, k)[:, t.col0:t.col1], getattr(want, k)[:, t.col0:t.col1],
                                              err_msg=f"tile {t.tile} {k}")
            cols += t.col1 - t.col0
        assert cols == N
    finally:
        for t in tiles:
            t.close()


def test_more_flows_than_components_is_an_argument_error():
    from gqmap_opticalflow_amd import Engine
    I1, I2, o, (M, N) = problem("mixture")
    with Engine(o, I1, I2) as e:
        e.init_state(2)
        before = e.get_state()
        f = np.zeros((M, N, 2, 4), order="F")  # H = L + 1
        assert e.lib.gqmap_init_state_flows(e.ctx, f.ctypes.data_as(C.POINTER(C.c_double)), 4, C.c_uint64(2)) == 1
        assert b"gqmap_init_state_flows" in e.lib.gqmap_last_error()
        assert e.lib.gqmap_init_state_flows(e.ctx, f.ctypes.data_as(C.POINTER(C.c_double)), 0, C.c_uint64(2)) == 1
        assert_state_equal(e.get_state(), before, "nothing written")


def test_short_solve_seeded_from_three_hypotheses():
    """40 x 48, L = 3, 60 iterations from block_match_init(hypotheses=3): runs
    to the end with finite Energy, and the plain-init solve keeps its trace bit
    for bit before and after it in the same process."""
    from gqmap_opticalflow_amd import block_match_init, gqmap_gpu_mixture
    I1, I2 = R.crop_pair(R.CROPS[0])
    flow, ranges = block_match_init(I1, I2, hypotheses=3)
    assert flow.shape == (40, 48, 2, 3)
    hflow, _ = block_match_init(I1, I2, host=True, hypotheses=3)
    assert np.array_equal(flow.view(np.uint64), hflow.view(np.uint64))
    c2 = dict(K=9, temperature=0.0, drate=0.5, epsn=1e-6, lambdas=5.0, lambdad=1.0)  # optical_flow.m
    o = {**c2, **ranges, "L": 3, "its": 60}
    before = gqmap_gpu_mixture(o, I1, I2, seed=1)
    mu, sigma, alpha, _, energy, _ = gqmap_gpu_mixture(o, I1, I2, seed=1, init_flow=flow)
    after = gqmap_gpu_mixture(o, I1, I2, seed=1)
    assert mu.shape == (40, 48, 3, 2) and energy.shape == (60,)
    assert np.all(np.isfinite(energy)) and np.all(np.isfinite(mu)) and np.all(np.isfinite(sigma))
    assert not np.array_equal(energy, before[4])
    for a, b, what in zip(before, after, ("mu", "sigma", "alpha", "AEPE", "Energy", "logP")):
        np.testing.assert_array_equal(a, b, err_msg=what)
