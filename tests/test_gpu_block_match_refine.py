"""gqmap_block_match_refine (HIP kernel) against gqmap_block_match_refine_host:
one header (csrc/gqmap_blockmatch.h) behind both, so flow, cost and curvature
agree BIT FOR BIT, NaN patterns included; the host model itself is checked
against numpy in tests/test_block_match_refine.py.  Then gqmap_init_state_seeded
(a flow and a width per mixture component) against its host formula, and one
short solve seeded with both through the public solver."""
import ctypes as C

import numpy as np
import pytest

from tests import _blockmatch_gpu as BG
from tests import _blockmatch_np as R
from tests._blockmatch_gpu import (KEYS, NAN_BITS, as_fp32, assert_bit_equal, assert_state_equal, bits, flows, force_cols,
                                   problem)

pytestmark = pytest.mark.gpu


def both(A, B, params, H, sep):
    dev, host = BG.both(A, B, params, hypotheses=H, sep=sep, subpixel=True)
    assert len(dev) == len(host) == 3
    return dev, host


@pytest.mark.parametrize("params", R.PARAMS, ids=str)
@pytest.mark.parametrize("crop", R.CROPS, ids=str)
def test_kernel_equals_host_model(crop, params):
    assert_bit_equal(*both(*R.crop_pair(crop), params, 3, 2))


@pytest.mark.parametrize("crop,params,H,sep", [(R.CROPS[0], (7, 7, 3, 1.7), 4, 1), (R.CROPS[3], (7, 7, 3, 1.7), 2, 3),
                                               (R.CROPS[4], (1, 1, 1, 0.8), 4, 2),  # 3 x 3 window: ranks run out, pixel by pixel
                                               (R.CROPS[0], (32, 32, 4, 2.0), 3, 2),  # the largest LDS window
                                               (R.CROPS[0], (7, 7, 3, 1.7), 1, 2)],  # H = 1: two scans
                         ids=str)
def test_other_hypothesis_counts_and_the_largest_window(crop, params, H, sep):
    assert_bit_equal(*both(*R.crop_pair(crop), params, H, sep))


@pytest.mark.parametrize("cols", [0, 8, 16, 32])
def test_several_tiles_with_partial_tiles_at_every_tile_width(cols):
    """97 x 130: four tile rows, the last tile of each row and column partial;
    8, 16, 32 force each instantiation of the new kernel.  A wrong T-buffer
    parity at a scan boundary or a neighbour capture that crosses tiles shows
    here.  cost is gqmap_block_match_multi's on the device, bit for bit."""
    from gqmap_opticalflow_amd import block_match
    I1, I2, _ = R.rubberwhale()
    A, B = (np.asfortranarray(a[60:157, 210:340]) for a in (I1, I2))
    try:
        force_cols(cols)
        dev, host = both(A, B, (7, 7, 3, 1.7), 3, 2)
        assert_bit_equal(dev, host)
        mflow, mcost = block_match(A, B, 7, 7, 3, 1.7, hypotheses=3, sep=2)
        assert np.array_equal(bits(dev[1]), bits(mcost))
        assert np.abs(dev[0] - mflow).max() <= 0.5 and np.any(dev[2] > 0)
    finally:
        force_cols(0)


@pytest.mark.parametrize("shape", [(1, 1), (64, 1), (1, 64)], ids=str)
def test_degenerate_images(shape):
    I1, I2, _ = R.rubberwhale()
    M, N = shape
    A, B = (np.asfortranarray(a[120:120 + M, 250:250 + N]) for a in (I1, I2))
    assert_bit_equal(*both(A, B, (7, 7, 3, 1.7), 3, 2))


def test_a_window_of_one_displacement():
    dev, host = both(*R.crop_pair(R.CROPS[3]), (0, 0, 3, 1.7), 2, 2)
    assert_bit_equal(dev, host)
    assert np.all(dev[0][:, :, :, 0] == 0) and np.all(dev[2] == 0)
    assert np.all(bits(dev[0][:, :, :, 1]) == NAN_BITS) and np.all(np.isposinf(dev[1][:, :, 1]))


def test_missing_ranks_and_elapsed_ms():
    from gqmap_opticalflow_amd import block_match
    z = np.zeros((16, 16))
    flow, cost, curv, ms = block_match(z, z, 1, 1, 1, 1.0, hypotheses=3, sep=3, subpixel=True, timed=True)
    assert np.isfinite(ms) and ms > 0
    assert np.all(flow[:, :, :, 0] == 1) and np.all(cost[:, :, 0] == 0) and np.all(curv == 0)
    assert np.all(bits(flow[:, :, :, 1:]) == NAN_BITS) and np.all(np.isposinf(cost[:, :, 1:]))
    assert_bit_equal((flow, cost, curv), block_match(z, z, 1, 1, 1, 1.0, host=True, hypotheses=3, sep=3, subpixel=True))


def test_cost_and_curv_may_be_null():
    from gqmap_opticalflow_amd import _lib
    lib = _lib.load()
    A, B = R.crop_pair(R.CROPS[4])
    flow = np.zeros((5, 7, 2, 2), order="F")
    assert lib.gqmap_block_match_refine(_lib.dptr(A), _lib.dptr(B), 5, 7, 3, 3, 2, 1.0, 2, 2, _lib.dptr(flow), None, None,
                                        None, 0) == 0
    from gqmap_opticalflow_amd import block_match
    assert np.array_equal(bits(flow), bits(block_match(A, B, 3, 3, 2, 1.0, host=True, hypotheses=2, subpixel=True)[0]))


# ---- gqmap_init_state_seeded ----------------------------------------------------

def widths(M, N, H, seed, o):
    """Widths of every kind: inside the bounds, below sig_lo, above sig_hi, and
    NaN, 0, negative and infinite entries, which keep the draw."""
    lo, hi = o.get("sig_lo", 0.01), o.get("sig_hi", 23.0)
    rng = np.random.default_rng(seed)
    s = np.asfortranarray(rng.uniform(0.2, 3.0, (M, N, 2, H)))
    s[0, 1, 0, 0], s[1, 0, 1, 0], s[2, 2, 0, 0], s[3, 1, 1, 0] = np.nan, 0.0, -1.5, np.inf
    s[4, 0, 0, 0], s[0, 4, 1, 0] = lo / 4, hi * 3
    s[:, N - 1, :, H - 1] = hi * 2  # the last column: the border ring is reached
    s[M - 1, :, :, 0] = lo / 2
    return s


@pytest.mark.parametrize("engine,precision,H", [("mixture", "fp64", 3), ("mixture", "fp64", 1), ("mixture", "fp32", 3),
                                                ("mixture", "fp32", 1), ("super", "fp64", 3), ("super", "fp64", 1),
                                                ("super", "fp32", 3), ("super", "fp32", 1)])
def test_device_state_equals_host_formula(engine, precision, H):
    from gqmap_opticalflow_amd import Engine, initial_state
    I1, I2, o, (M, N) = problem(engine)
    f, s = flows(M, N, H, seed=11), widths(M, N, H, 13, o)
    with Engine(o, I1, I2, engine, precision) as e:
        assert (e.M, e.N, e.L) == (M, N, 3)
        e.init_state_from_flow(f, seed=7, sigma=s)
        got = e.get_state()
        e.init_state_from_flow(f, seed=7)  # the flows init keeps its bits
        plain = e.get_state()
        # sigmas = NULL is gqmap_init_state_flows
        assert e.lib.gqmap_init_state_seeded(e.ctx, f.ctypes.data_as(C.POINTER(C.c_double)), None, H, C.c_uint64(7)) == 0
        null = e.get_state()
    want, base = initial_state(o, M, N, seed=7, engine=engine, flow=f, sigma=s), \
        initial_state(o, M, N, seed=7, engine=engine, flow=f)
    if precision == "fp32":
        want, base = as_fp32(want), as_fp32(base)
    assert_state_equal(got, want, "seeded init")
    assert_state_equal(plain, base, "flows init")
    assert_state_equal(null, base, "sigmas = NULL")
    for l in range(3):
        same = np.array_equal(got.sigu[:, :, l], plain.sigu[:, :, l])
        assert same == (l >= H), f"component {l}"
    # directly, without the host formula
    lo, hi = e.opts.sig_lo, e.opts.sig_hi
    x = s[:, :, 0, 0]
    with np.errstate(invalid="ignore"):
        given = np.isfinite(x) & (x > 0)
    c = np.clip(x, lo, hi)
    c = c.astype(np.float32).astype(np.float64) if precision == "fp32" else c
    assert np.array_equal(got.sigu[:, :, 0][given], c[given])
    assert np.array_equal(got.sigu[:, :, 0][~given], plain.sigu[:, :, 0][~given])
    assert not given[0, 1] and not given[2, 2] and given[4, 0]
    assert got.sigv[:, :, 0][1, 0] == plain.sigv[:, :, 0][1, 0] and got.sigv[:, :, 0][3, 1] == plain.sigv[:, :, 0][3, 1]


def test_three_iterations_equal_the_set_state_path():
    """Both state buffers and the border ring take the widths: the iteration reads them."""
    from gqmap_opticalflow_amd import Engine, initial_state
    I1, I2, o, (M, N) = problem("mixture")
    f, s = flows(M, N, 3, seed=5), widths(M, N, 3, 6, o)
    with Engine(o, I1, I2) as e:
        e.init_state_from_flow(f, seed=2, sigma=s)
        d1, t1 = e.run(3)
        s1 = e.get_state()
    with Engine(o, I1, I2) as e:
        e.set_state(initial_state(o, M, N, seed=2, flow=f, sigma=s))
        d2, t2 = e.run(3)
        s2 = e.get_state()
    assert d1 == d2 == 3
    np.testing.assert_array_equal(t1, t2)
    assert_state_equal(s1, s2, "after 3 iterations")


def test_two_tiles_take_their_columns_of_the_full_widths():
    from gqmap_opticalflow_amd import Engine, initial_state, tile_group_run
    I1, I2, o, (M, N) = problem("mixture")
    f, s = flows(M, N, 3, seed=9), widths(M, N, 3, 10, o)
    want = initial_state(o, M, N, seed=4, flow=f, sigma=s)
    tiles = [Engine(o, I1, I2, n_tiles=2, tile=t) for t in range(2)]
    try:
        cols = 0
        for t in tiles:
            t.init_state_from_flow(f, seed=4, sigma=s)
            got = t.get_state()
            for k in KEYS[:6]:
                np.testing.assert_array_equal(getattr(got, k)[:, t.col0:t.col1], getattr(want, k)[:, t.col0:t.col1],
                                              err_msg=f"tile {t.tile} {k}")
            cols += t.col1 - t.col0
        assert cols == N
        # the ghost columns take the widths too: three lockstep iterations equal the whole grid's
        with Engine(o, I1, I2) as e:
            e.init_state_from_flow(f, seed=4, sigma=s)
            _, tr = e.run(3)
            ref = e.get_state()
        done, ttr = tile_group_run(tiles, 3)
        assert done == 3
        np.testing.assert_array_equal(ttr, tr)
        for t in tiles:
            got = t.get_state()
            for k in KEYS[:6]:
                np.testing.assert_array_equal(getattr(got, k)[:, t.col0:t.col1], getattr(ref, k)[:, t.col0:t.col1],
                                              err_msg=f"tile {t.tile} {k} after 3 iterations")
    finally:
        for t in tiles:
            t.close()


def test_more_flows_than_components_is_an_argument_error():
    from gqmap_opticalflow_amd import Engine
    I1, I2, o, (M, N) = problem("mixture")
    D = C.POINTER(C.c_double)
    with Engine(o, I1, I2) as e:
        e.init_state(2)
        before = e.get_state()
        f = np.zeros((M, N, 2, 4), order="F")  # H = L + 1
        s = np.ones((M, N, 2, 4), order="F")
        assert e.lib.gqmap_init_state_seeded(e.ctx, f.ctypes.data_as(D), s.ctypes.data_as(D), 4, C.c_uint64(2)) == 1
        assert b"gqmap_init_state_seeded" in e.lib.gqmap_last_error()
        assert e.lib.gqmap_init_state_seeded(e.ctx, f.ctypes.data_as(D), s.ctypes.data_as(D), 0, C.c_uint64(2)) == 1
        assert e.lib.gqmap_init_state_seeded(e.ctx, None, s.ctypes.data_as(D), 1, C.c_uint64(2)) == 1
        assert_state_equal(e.get_state(), before, "nothing written")


def test_short_solve_seeded_with_flows_and_widths():
    """24 x 20, L = 3, 20 iterations through the public solver from
    block_match_init(hypotheses=3, subpixel=True, sigma_from_cost=True): bit for
    bit the solve started from set_state(initial_state(flow=, sigma=))."""
    from gqmap_opticalflow_amd import block_match_init, gqmap_gpu_mixture, initial_state
    I1, I2, o, (M, N) = problem("mixture")
    flow, ranges, sig = block_match_init(I1, I2, hypotheses=3, subpixel=True, sigma_from_cost=True)
    assert flow.shape == sig.shape == (M, N, 2, 3)
    hflow, _, hsig = block_match_init(I1, I2, host=True, hypotheses=3, subpixel=True, sigma_from_cost=True)
    assert np.array_equal(bits(flow), bits(hflow)) and np.array_equal(bits(sig), bits(hsig))
    assert np.any(np.isnan(sig)) and np.nanmin(sig) == 0.5
    o = {**o, "its": 20}
    a = gqmap_gpu_mixture(o, I1, I2, seed=1, init_flow=flow, init_sigma=sig)
    b = gqmap_gpu_mixture(o, I1, I2, seed=1, state=initial_state(o, M, N, seed=1, flow=flow, sigma=sig))
    plain = gqmap_gpu_mixture(o, I1, I2, seed=1, init_flow=flow)
    assert a[0].shape == (M, N, 3, 2) and a[4].shape == (20,) and np.all(np.isfinite(a[4]))
    for x, y, what in zip(a, b, ("mu", "sigma", "alpha", "AEPE", "Energy", "logP")):
        np.testing.assert_array_equal(x, y, err_msg=what)
    assert not np.array_equal(a[4], plain[4])  # the widths reached the solve
