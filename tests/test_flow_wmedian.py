"""The weighted median filter without a device: the library's host model
(gqmap_flow_wmedian_host) against the numpy restatement of csrc/gqmap_wmedian.h
(tests/_wmedian_np.py) BIT FOR BIT, against plain numpy where the weights are
flat, closed forms on steps, stripes, outlier blocks and holes, the RubberWhale
crop, argument errors, flow_confidence and block_match_flow(median=).  The
kernel against the host model: tests/test_gpu_flow_wmedian.py."""
import ctypes as C
import re

import numpy as np
import pytest

from tests import _blockmatch_np as R
from tests import _codeobj
from tests import _wmedian_np as W
from tests._wmedian_np import bits


def host(flow, guide, r=2, sigma_s=2.0, sigma_c=10.0, passes=1, conf=None):
    from gqmap_opticalflow_amd import flow_wmedian
    return flow_wmedian(flow, guide, r, sigma_s, sigma_c, passes, conf, host=True)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def const(M, N, u, v):
    return np.asfortranarray(np.broadcast_to(np.array([u, v], dtype=np.float64), (M, N, 2)))


SHAPES = [(1, 1), (1, 64), (64, 1), (37, 70)]


# ---- the host model against the restatement ----------------------------------------------------

@pytest.mark.parametrize("r", [0, 1, 2, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_host_equals_the_restatement(shape, r):
    M, N = shape
    for flow, nans in ((W.noisy(M, N, 1), False), (W.special(M, N, 2), False), (W.special(M, N, 3), True)):
        guide = W.guide_of(M, N, 4, nans)
        for conf in (None, W.conf_of(M, N, 5, nans)):
            wants = W.wmedian(flow, guide, r, 0.5 * r + 1.0, 10.0, 3, conf, history=True)
            for passes in (1, 3):
                out, want = host(flow, guide, r, 0.5 * r + 1.0, 10.0, passes, conf), wants[passes - 1]
                assert same(out, want), (r, passes, conf is not None, nans, int((bits(out) != bits(want)).sum()))


def test_the_fields_are_not_vacuous():
    """The special field holds every special value, the filter moves most pixels and the guide and the
    confidence each change the result."""
    M, N = 37, 70
    f, g, c = W.special(M, N, 2), W.guide_of(M, N, 4), W.conf_of(M, N, 5)
    assert np.isnan(f).any() and np.isposinf(f).any() and np.isneginf(f).any()
    assert (bits(f) == 0).any() and (bits(f) == W.SIGN).any()
    out = host(f, g)
    assert (bits(out) != bits(f)).mean() > 0.5
    assert not same(out, host(f, np.zeros((M, N)))) and not same(out, host(f, g, conf=c))
    assert np.isnan(W.guide_of(M, N, 4, True)).any() and np.isnan(W.conf_of(M, N, 5, True)).any()
    assert (c == 0).any() and (c == 1e-6).any()


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_radius_zero_is_the_identity_and_a_constant_a_fixed_point(shape):
    M, N = shape
    f = W.special(M, N, 6)
    for conf in (None, W.conf_of(M, N, 5, True)):
        assert same(host(f, W.guide_of(M, N, 4, True), 0, 1.0, 10.0, 3, conf), f)
    k = const(M, N, 2.75, -0.0)
    for r in (1, 2, 8):
        assert same(host(k, W.guide_of(M, N, 4), r, 2.0, 10.0, 2, W.conf_of(M, N, 5)), k)


@pytest.mark.parametrize("r", [1, 2, 8])
def test_every_output_is_one_of_its_window(r):
    M, N = 37, 70
    f = W.special(M, N, 7)
    out = host(f, W.guide_of(M, N, 4), r, 2.0, 10.0, 1, W.conf_of(M, N, 5))
    for c in (0, 1):
        P = np.full((M + 2 * r, N + 2 * r), 1, dtype=np.uint64)  # the bits of a denormal the field does not hold
        P[r:r + M, r:r + N] = bits(f[:, :, c])
        found = np.zeros((M, N), dtype=bool)
        for dj in range(2 * r + 1):
            for di in range(2 * r + 1):
                found |= P[di:di + M, dj:dj + N] == bits(out[:, :, c])
        assert found.all()


@pytest.mark.parametrize("r", [1, 2, 8])
@pytest.mark.parametrize("shape", [(1, 64), (64, 1), (37, 70)], ids=str)
def test_flat_weights_give_the_plain_lower_median(shape, r):
    """sigma_s = 1e9 rounds every tap to 1.0; with a flat guide and no confidence every entry weighs 2^16, so the
    output is np.sort(window)[(n - 1) // 2] over the window cut at the frame: plain numpy, no model."""
    M, N = shape
    f = np.asfortranarray(np.random.default_rng(8).uniform(-4, 4, (M, N, 2)))
    f[::3, ::4, 0] = np.inf
    out = host(f, np.full((M, N), 7.0), r, 1e9, 10.0)
    for m in range(M):
        for n in range(N):
            win = f[max(m - r, 0):m + r + 1, max(n - r, 0):n + r + 1].reshape(-1, 2)
            want = np.sort(win, axis=0)[(win.shape[0] - 1) // 2]
            assert np.array_equal(out[m, n], want), (m, n)


# ---- closed forms ------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(37, 45), (12, 11)], ids=str)
def test_a_step_guide_keeps_the_motion_edge_and_removes_lattice_outliers(shape):
    M, N = shape
    n = np.arange(N)[None, :] + np.zeros((M, 1), dtype=int)
    right = n >= N // 2
    guide = np.where(right, 255.0, 0.0)
    clean = np.asfortranarray(np.stack([np.where(right, -2.0, 1.0), np.where(right, 3.0, 0.0)], axis=2))
    f = clean.copy(order="F")
    rng = np.random.default_rng(9)
    f[::5, ::5] = rng.uniform(-8, 8, f[::5, ::5].shape)
    f[6, 7, 0] = np.nan
    assert (f != clean).sum() > 10
    assert same(host(f, guide, 2, 2.0, 10.0), clean)


def test_a_stripe_survives_with_the_guide_and_not_without():
    M, N = 20, 23
    guide = np.zeros((M, N), order="F")
    guide[:, 10:12] = 255.0
    f = np.zeros((M, N, 2), order="F")
    f[:, 10:12, 0], f[:, 10:12, 1] = 4.0, -1.0
    assert same(host(f, guide, 2, 2.0, 10.0), f)
    flat = host(f, np.zeros((M, N)), 2, 2.0, 10.0)
    assert (flat != f).any(axis=2).sum() == 40 and np.all(flat == 0)


def test_a_confidence_of_zero_removes_an_outlier_block():
    M, N = 20, 23
    clean = const(M, N, 1.5, -0.5)
    f = clean.copy(order="F")
    f[8:12, 9:13] = np.random.default_rng(10).uniform(5, 9, (4, 4, 2))
    guide = np.full((M, N), 100.0)
    out = host(f, guide, 2, 2.0, 10.0)
    assert (out != clean).any(axis=2).sum() == 12
    for low in (0.0, 1e-6):  # 1e-6 < 2^-16: no weight either
        conf = np.ones((M, N))
        conf[8:12, 9:13] = low
        assert same(host(f, guide, 2, 2.0, 10.0, conf=conf), clean)


def test_nan_holes_are_filled_from_what_is_in_reach():
    M, N = 20, 23
    guide = np.full((M, N), 100.0)
    f = const(M, N, 1.5, -0.5).copy(order="F")
    f[8:11, 9:12] = np.nan
    assert same(host(f, guide, 2, 2.0, 10.0), const(M, N, 1.5, -0.5))
    f[6:13, 7:14] = np.nan
    out = host(f, guide, 2, 2.0, 10.0)
    left = np.isnan(out[:, :, 0])
    assert left.sum() == 9 and left[8:11, 9:12].all() and np.array_equal(left, np.isnan(out[:, :, 1]))
    assert same(host(f, guide, 2, 2.0, 10.0, 2), const(M, N, 1.5, -0.5))
    # a pixel that keeps its bits keeps its NaN payload
    lone = np.zeros((1, 1, 2))
    lone.view(np.uint64)[...] = 0x7FF8000000000123
    assert same(host(lone, np.zeros((1, 1)), 2), lone)


def test_passes_are_jacobi():
    M, N = 37, 70
    f, g, c = W.special(M, N, 2), W.guide_of(M, N, 4), W.conf_of(M, N, 5)
    step = f
    for _ in range(3):
        step = host(step, g, 2, 2.0, 10.0, 1, c)
    assert same(step, host(f, g, 2, 2.0, 10.0, 3, c))


# ---- RubberWhale ---------------------------------------------------------------------------------------

def test_the_filter_improves_the_integer_start_on_the_rubberwhale_crop():
    """Rows 100..299, columns 150..409, block_match_init(7, 7, 3, 1.7) as the integer start, AEPE over the known
    pixels 10 px inside the crop.  An independent numpy run gave 0.595 unfiltered, 0.525 after one pass of
    r = 2, sigma_s = 2, sigma_c = 10 and 0.396 after three passes of r = 7, sigma_s = 5, sigma_c = 10.  No band is
    asserted: the agreement with the restatement above is the gate."""
    from gqmap_opticalflow_amd import block_match_init
    I1, I2, gt = R.rubberwhale()
    sl = (slice(100, 300), slice(150, 410))
    A, B, T = np.asfortranarray(I1[sl]), np.asfortranarray(I2[sl]), gt[sl]
    start = block_match_init(A, B, 7, 7, 3, 1.7, host=True)[0]
    known = np.all(np.abs(T) <= 1e9, axis=2)
    known[:10], known[-10:], known[:, :10], known[:, -10:] = False, False, False, False
    epe = lambda f: np.sqrt(np.sum((T - f) ** 2, axis=2))[known].mean()
    a0, a1, a3 = epe(start), epe(host(start, A, 2, 2.0, 10.0)), epe(host(start, A, 7, 5.0, 10.0, 3))
    print(f"AEPE: integer start {a0:.4f}, one pass r=2 {a1:.4f}, three passes r=7 {a3:.4f}")
    assert a1 < a0 and a3 < a0


# ---- arguments -------------------------------------------------------------------------------------------

def test_bad_arguments_write_nothing():
    from gqmap_opticalflow_amd import _lib, flow_wmedian
    lib = _lib.load()
    M, N = 5, 6
    f, g, c = W.noisy(M, N, 1), W.guide_of(M, N), W.conf_of(M, N)
    out = np.full((M, N, 2), 7.0, order="F")
    D = _lib.dptr
    nan, inf = float("nan"), float("inf")
    for name, tail in (("gqmap_flow_wmedian_host", ()), ("gqmap_flow_wmedian", (None, 0))):
        fn = getattr(lib, name)
        for args in ((D(f), D(g), D(c), 0, N, 2, 2.0, 10.0, 1, D(out)), (D(f), D(g), D(c), M, 0, 2, 2.0, 10.0, 1, D(out)),
                     (D(f), D(g), D(c), M, N, -1, 2.0, 10.0, 1, D(out)), (D(f), D(g), D(c), M, N, 9, 2.0, 10.0, 1, D(out)),
                     (D(f), D(g), D(c), M, N, 2, 0.0, 10.0, 1, D(out)), (D(f), D(g), D(c), M, N, 2, nan, 10.0, 1, D(out)),
                     (D(f), D(g), D(c), M, N, 2, inf, 10.0, 1, D(out)), (D(f), D(g), D(c), M, N, 2, 2.0, 0.0, 1, D(out)),
                     (D(f), D(g), D(c), M, N, 2, 2.0, -1.0, 1, D(out)), (D(f), D(g), D(c), M, N, 2, 2.0, nan, 1, D(out)),
                     (D(f), D(g), D(c), M, N, 2, 2.0, inf, 1, D(out)), (D(f), D(g), D(c), M, N, 2, 2.0, 10.0, 0, D(out)),
                     (D(f), D(g), D(c), M, N, 2, 2.0, 10.0, 9, D(out)), (None, D(g), D(c), M, N, 2, 2.0, 10.0, 1, D(out)),
                     (D(f), None, D(c), M, N, 2, 2.0, 10.0, 1, D(out)), (D(f), D(g), D(c), M, N, 2, 2.0, 10.0, 1, None)):
            assert fn(*args, *tail) == 1
            assert name.encode() + b":" in lib.gqmap_last_error()
    assert np.all(out == 7.0)
    # a null conf is 1 everywhere
    assert lib.gqmap_flow_wmedian_host(D(f), D(g), None, M, N, 2, 2.0, 10.0, 1, D(out)) == 0
    assert same(out, host(f, g, conf=np.ones((M, N)))) and same(out, W.wmedian(f, g))
    for bad in (dict(flow=f[:, :, 0]), dict(guide=np.zeros((M, N + 1))), dict(conf=np.ones((M + 1, N))),
                dict(flow=np.zeros((M, N, 3)))):
        kw = dict(flow=f, guide=g, conf=c, host=True)
        kw.update(bad)
        with pytest.raises(ValueError):
            flow_wmedian(**kw)


# ---- flow_confidence and block_match_flow(median=) ------------------------------------------------------------

def test_flow_confidence():
    from gqmap_opticalflow_amd import flow_confidence
    sig = np.zeros((3, 4, 2))
    sig[..., 0], sig[..., 1] = 0.5, 1.5
    sig[1, 2, 1] = np.nan
    sig[0, 0] = 0.0
    c = flow_confidence(sig)
    assert c.shape == (3, 4) and c.dtype == np.float64 and c[0, 0] == 1.0 and np.isnan(c[1, 2])
    assert c[2, 3] == 1.0 / (1.0 + (0.25 + 2.25)) and flow_confidence(sig, 2.0)[2, 3] == 1.0 / (1.0 + 2.5 / 4.0)
    for bad in (dict(sigma=sig[..., 0]), dict(sigma=sig, s0=0.0), dict(sigma=sig, s0=float("nan"))):
        with pytest.raises(ValueError):
            flow_confidence(**bad)
    # a NaN confidence is no weight: the same as 0
    f, g = W.noisy(3, 4, 1), np.zeros((3, 4))
    assert same(host(f, g, conf=c), host(f, g, conf=np.where(np.isnan(c), 0.0, c)))


def test_block_match_flow_with_and_without_the_median():
    from gqmap_opticalflow_amd import block_match_flow, flow_confidence
    I1, I2 = R.crop_pair(R.CROPS[0])
    kw = dict(U=3, V=3, ft=2, sigma=1.0, denoise=dict(its=5), host=True)
    plain = block_match_flow(I1, I2, **kw)
    none = block_match_flow(I1, I2, median=None, **kw)
    assert len(plain) == len(none) == 3
    for x, y in zip(plain, none):
        assert x.dtype == y.dtype and same(x.astype(np.float64), y.astype(np.float64))
    mu, sg, cons = plain
    med = block_match_flow(I1, I2, median=dict(r=1, passes=2), **kw)
    assert same(med[0], host(mu, I1, r=1, passes=2)) and not same(med[0], mu)
    assert same(med[1], sg) and np.array_equal(med[2], cons)
    wsig = block_match_flow(I1, I2, median=dict(conf="sigma", sigma_c=20.0), **kw)
    assert same(wsig[0], host(mu, I1, sigma_c=20.0, conf=flow_confidence(sg)))
    arr = np.ones(cons.shape)
    assert same(block_match_flow(I1, I2, median=dict(conf=arr), **kw)[0], host(mu, I1))
    with pytest.raises(ValueError):
        block_match_flow(I1, I2, median=dict(conf="cost"), **kw)


# ---- the kernels' listing ------------------------------------------------------------------------------------

CU_LDS = 160 * 1024


@pytest.mark.skipif(not _codeobj.available(), reason="library or ROCm LLVM tools absent")
def test_kernels_have_no_scratch_and_fit_the_lds():
    """The gfx950 code object's metadata (tests/_codeobj.py): the eight documented instantiations,
    k_flow_wmedian_lane<R> (a lane per pixel, r = R = 0, 1, 2) and k_flow_wmedian<NE> (a wave per pixel, NE = 1..5
    entries per lane).  The staged tile is dynamic LDS, 32 W^2 bytes with W = 16 + 2r, on top of the taps and the
    result buffer the wave kernels hold statically."""
    from gqmap_opticalflow_amd import _lib
    seen = {k: v for k, v in _codeobj.kernels().items() if "k_flow_wmedian" in k}
    names = sorted(re.search(r"(k_flow_wmedian(?:_lane)?)ILi(\d+)E", k).groups() for k in seen)
    assert names == [("k_flow_wmedian", str(i)) for i in range(1, 6)] + [("k_flow_wmedian_lane", str(i)) for i in range(3)]
    lib = _lib.load()
    for fn in (lib.gqmap_debug_flow_wmedian_lds, lib.gqmap_debug_flow_wmedian_entries):
        fn.restype, fn.argtypes = C.c_int, [C.c_int]
    lib.gqmap_debug_flow_wmedian_tile.restype = C.c_int
    S = lib.gqmap_debug_flow_wmedian_tile()
    for r in range(9):
        assert lib.gqmap_debug_flow_wmedian_lds(r) == 32 * (S + 2 * r) ** 2
        assert lib.gqmap_debug_flow_wmedian_entries(r) == (0 if r <= 2 else -(-(2 * r + 1) ** 2 // 64))
    assert lib.gqmap_debug_flow_wmedian_lds(9) == -1 and lib.gqmap_debug_flow_wmedian_lds(-1) == -1
    for v in seen.values():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0
        assert lib.gqmap_debug_flow_wmedian_lds(8) + v["group_segment_fixed_size"] <= CU_LDS
