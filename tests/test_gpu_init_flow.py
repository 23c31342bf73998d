"""gqmap_init_state_flow on the device against its host formula
(initial_state(..., flow=f)), bit for bit, and the ground-truth-free path end
to end: block_match_init -> options ranges + init_flow."""
import ctypes as C

import numpy as np
import pytest

from tests import _golden as G
from tests._initflow import make_flow

pytestmark = pytest.mark.gpu

KEYS = G.STATE_KEYS


def problem(engine, L):
    """Golden frames with the golden's options: the mixture cases run on the
    24 x 32 corner of the super golden's 32 x 40 frames, the super case on the
    whole of them (node grid 8 x 10).  The golden ranges (about [-1.6, 1.4]) are
    narrower than the flow of make_flow ([-4, 4]), so clamping happens."""
    d = G.load("super_L3")
    if engine == "super":
        o = dict(d["opts"], L=L)
        return d["I1"], d["I2"], o, (8, 10)
    o = dict(G.load("mixture_L1" if L == 1 else "mixture_L3_T")["opts"], L=L)
    I1, I2 = (np.asfortranarray(d[k][:24, :32]) for k in ("I1", "I2"))
    return I1, I2, o, (24, 32)


def assert_state_equal(a, b, what=""):
    for k in KEYS:
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=f"{what} {k}")
    assert a.it == b.it and a.T == b.T


def as_fp32(st):
    for k in KEYS[:6]:
        setattr(st, k, np.asfortranarray(getattr(st, k).astype(np.float32).astype(np.float64)))
    return st


@pytest.mark.parametrize("engine,L,precision", [("mixture", 1, "fp64"), ("mixture", 3, "fp64"), ("super", 3, "fp64"),
                                                ("mixture", 3, "fp32"), ("super", 3, "fp32")])
def test_device_state_equals_host_formula(engine, L, precision):
    from gqmap_opticalflow_amd import Engine, initial_state
    I1, I2, o, (M, N) = problem(engine, L)
    f = make_flow(M, N, seed=L)
    with Engine(o, I1, I2, engine, precision) as e:
        assert (e.M, e.N) == (M, N)
        e.init_state_from_flow(f, seed=7)
        got = e.get_state()
        e.init_state(7)  # the plain init keeps its bits
        plain = e.get_state()
    want, base = initial_state(o, M, N, seed=7, flow=f), initial_state(o, M, N, seed=7)
    if precision == "fp32":
        want, base = as_fp32(want), as_fp32(base)
    assert_state_equal(got, want, "flow init")
    assert_state_equal(plain, base, "plain init")
    assert not np.array_equal(got.muu[:, :, 0], plain.muu[:, :, 0])


@pytest.mark.parametrize("engine,L", [("mixture", 3), ("super", 3)])
def test_three_iterations_equal_the_set_state_path(engine, L):
    """Both state buffers and the border ring are seeded: the iteration reads them."""
    from gqmap_opticalflow_amd import Engine, initial_state
    I1, I2, o, (M, N) = problem(engine, L)
    f = make_flow(M, N, seed=5)
    with Engine(o, I1, I2, engine) as e:
        e.init_state_from_flow(f, seed=2)
        d1, t1 = e.run(3)
        s1 = e.get_state()
    with Engine(o, I1, I2, engine) as e:
        e.set_state(initial_state(o, M, N, seed=2, flow=f))
        d2, t2 = e.run(3)
        s2 = e.get_state()
    assert d1 == d2 == 3
    np.testing.assert_array_equal(t1, t2)
    assert_state_equal(s1, s2, "after 3 iterations")


def test_two_tiles_take_their_columns_of_the_full_flow():
    from gqmap_opticalflow_amd import Engine, initial_state, tile_group_run
    I1, I2, o, (M, N) = problem("mixture", 3)
    f = make_flow(M, N, seed=9)
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
        # the ghost columns are seeded too: three lockstep iterations equal the whole grid's
        with Engine(o, I1, I2) as e:
            e.init_state_from_flow(f, seed=4)
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


def test_init_state_flow_before_set_images_is_a_state_error():
    from gqmap_opticalflow_amd import _lib
    from gqmap_opticalflow_amd.engine import make_options
    lib = _lib.load()
    opts = make_options(dict(L=1, minu=-1, maxu=1, minv=-1, maxv=1))
    ctx = C.c_void_p()
    assert lib.gqmap_create(C.byref(ctx), C.byref(opts), 0) == 0
    try:
        f = np.zeros((4, 4, 2), order="F")
        assert lib.gqmap_init_state(ctx, C.c_uint64(0)) == 5  # GQMAP_ERR_STATE
        assert lib.gqmap_init_state_flow(ctx, _lib.dptr(f), C.c_uint64(0)) == 5
        assert b"before gqmap_set_images" in lib.gqmap_last_error()
    finally:
        lib.gqmap_destroy(ctx)


def test_no_ground_truth_end_to_end():
    """Two frames and nothing else: range and start from block matching."""
    from gqmap_opticalflow_amd import Engine, block_match_init, gqmap_gpu_mixture
    from tests import _blockmatch_np as R
    I1, I2 = R.crop_pair((100, 200, 40, 48))
    flow, ranges = block_match_init(I1, I2)
    assert ranges == dict(minu=-7.0, maxu=7.0, minv=-7.0, maxv=7.0) and flow.shape == (40, 48, 2)
    hflow, _ = block_match_init(I1, I2, host=True)
    np.testing.assert_array_equal(flow, hflow)
    c2 = dict(K=9, temperature=0.0, drate=0.5, epsn=1e-6, lambdas=5.0, lambdad=1.0)  # optical_flow.m (config C2)
    o = {**c2, **ranges, "L": 1, "its": 5}
    mu, sigma, alpha, _, energy, _ = gqmap_gpu_mixture(o, I1, I2, init_flow=flow)
    assert mu.shape == (40, 48, 1, 2) and np.all(np.isfinite(energy)) and np.all(np.isfinite(mu))
    # without init_flow: today's path, bit for bit
    mu0, sigma0, _, _, energy0, _ = gqmap_gpu_mixture(o, I1, I2)
    with Engine(o, I1, I2) as e:
        e.init_state(0)
        _, tr = e.run(1)
        _, tr2 = e.run(4)
        st = e.get_state()
    np.testing.assert_array_equal(energy0, np.concatenate([tr[:, 0], tr2[:, 0]]))
    np.testing.assert_array_equal(mu0[..., 0], st.muu)
    np.testing.assert_array_equal(mu0[..., 1], st.muv)
    np.testing.assert_array_equal(sigma0[..., 0], st.sigu)
    assert not np.array_equal(energy, energy0)
