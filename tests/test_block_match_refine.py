"""Sub-pixel refinement of the block matcher, host model
(gqmap_block_match_refine_host) against the numpy restatement of
tests/_blockmatch_refine_np.py, and the Python layers on top: the seeded init
with a width (initial_state(flow=, sigma=)) and block_match_init(subpixel=,
sigma_from_cost=).  No device.

The restatement builds its cost volume in the header's own operation order, so
the comparison is BIT FOR BIT on flow, cost and curvature at every crop and
parameter set, ft = 0 and ft = 1 included; no tolerance is used."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import _blockmatch_np as R
from tests import _blockmatch_refine_np as F

H, SEP = 3, 2
NAN_BITS = 0x7FF8000000000000


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@functools.lru_cache(maxsize=None)
def model(crop, params, h=H, sep=SEP):
    """The refining host model on one crop, computed once and shared (read-only)."""
    from gqmap_opticalflow_amd import block_match
    out = block_match(*R.crop_pair(crop), *params, host=True, hypotheses=h, sep=sep, subpixel=True)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def multi(crop, params, h=H, sep=SEP):
    from gqmap_opticalflow_amd import block_match
    out = block_match(*R.crop_pair(crop), *params, host=True, hypotheses=h, sep=sep)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("params", R.PARAMS, ids=str)
@pytest.mark.parametrize("crop", R.CROPS, ids=str)
def test_host_model_equals_restatement_bit_for_bit(crop, params):
    flow, cost, curv = model(crop, params)
    rflow, rcurv, rcost, _ = F.reference(crop, params, H, SEP)
    assert flow.shape == rflow.shape and curv.shape == rcurv.shape and cost.shape == rcost.shape
    for got, want, what in ((flow, rflow, "flow"), (cost, rcost, "cost"), (curv, rcurv, "curv")):
        diff = bits(got) != bits(want)
        assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} entries differ"


@pytest.mark.parametrize("params", R.PARAMS, ids=str)
@pytest.mark.parametrize("crop", R.CROPS, ids=str)
def test_cost_and_picks_are_those_of_the_integer_matcher(crop, params):
    """cost keeps the bits of block_match(hypotheses=); the refined flow stays
    within half a pixel of the integer flow and on it where the curvature is 0;
    missing ranks are NaN / +Inf / 0 in the same places."""
    flow, cost, curv = model(crop, params)
    mflow, mcost = multi(crop, params)
    assert np.array_equal(bits(cost), bits(mcost))
    missing = np.isnan(mflow)
    assert np.array_equal(np.isnan(flow), missing)
    assert np.all(bits(flow)[missing] == NAN_BITS) and np.all(curv[missing] == 0)
    assert np.array_equal(np.isposinf(cost), missing[:, :, 0, :])
    d = (flow - mflow)[~missing]
    assert d.min() >= -0.5 and d.max() <= 0.5
    assert np.all(d[curv[~missing] == 0] == 0)
    assert np.all(curv >= 0)
    if params[2] > 0:  # a filtered cost surface of real frames has proper minima
        assert np.any(d != 0) and np.any(curv > 0)


def test_the_modes_agree_with_each_other():
    """What tests/test_gpu_block_match.py asks of the device at the same crop
    and parameters, here of the host model it is compared with."""
    from gqmap_opticalflow_amd import block_match
    crop, par = R.CROPS[3], (7, 7, 3, 1.7)
    flow, cost = block_match(*R.crop_pair(crop), *par, host=True)
    for ranked in (multi(crop, par, 1), multi(crop, par, 3)):
        assert np.array_equal(bits(flow), bits(ranked[0][..., 0])) and np.array_equal(bits(cost), bits(ranked[1][..., 0]))
    assert np.array_equal(bits(model(crop, par, 3)[1]), bits(multi(crop, par, 3)[1]))


def test_one_hypothesis_is_the_default_of_subpixel():
    from gqmap_opticalflow_amd import block_match
    A, B = R.crop_pair(R.CROPS[3])
    a = block_match(A, B, 3, 3, 2, 1.0, host=True, subpixel=True)
    b = block_match(A, B, 3, 3, 2, 1.0, host=True, subpixel=True, hypotheses=1)
    assert len(a) == 3 and a[0].shape == (33, 17, 2, 1) and a[1].shape == (33, 17, 1) and a[2].shape == (33, 17, 2, 1)
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y))
    three = model(R.CROPS[3], (3, 3, 2, 1.0))
    for x, y in zip(a, three):
        assert np.array_equal(bits(x[..., 0]), bits(y[..., 0]))  # rank 0 whatever H
    assert np.isnan(block_match(A, B, 3, 3, 2, 1.0, host=True, subpixel=True, timed=True)[3])


def test_closed_forms():
    from gqmap_opticalflow_amd import block_match
    A, B = R.crop_pair(R.CROPS[3])
    # U = V = 0: one displacement, no neighbour on either axis
    flow, cost, curv = block_match(A, B, 0, 0, 3, 1.7, host=True, hypotheses=2, subpixel=True)
    assert np.all(flow[:, :, :, 0] == 0) and np.all(curv == 0) and np.all(np.isfinite(cost[:, :, 0]))
    assert np.all(bits(flow[:, :, :, 1]) == NAN_BITS) and np.all(np.isposinf(cost[:, :, 1]))
    # U = 0, V > 0: only the column axis (plane 0, horizontal) can be refined
    flow, cost, curv = block_match(A, B, 0, 4, 3, 1.7, host=True, subpixel=True)
    mflow, _ = block_match(A, B, 0, 4, 3, 1.7, host=True, hypotheses=1)
    assert np.all(curv[:, :, 1] == 0) and np.all(flow[:, :, 1] == 0)
    assert np.any(curv[:, :, 0] > 0) and np.any(flow[:, :, 0] != mflow[:, :, 0])
    # zero frames: every cost is 0, den = 0 everywhere, nothing is refinable
    z = np.zeros((16, 16))
    for sep in (2, 3):
        flow, cost, curv = block_match(z, z, 1, 1, 1, 1.0, host=True, hypotheses=3, sep=sep, subpixel=True)
        mflow, mcost = block_match(z, z, 1, 1, 1, 1.0, host=True, hypotheses=3, sep=sep)
        assert np.array_equal(bits(flow), bits(mflow)) and np.array_equal(bits(cost), bits(mcost))
        assert np.all(curv == 0)
    assert np.all(np.isnan(flow[:, :, :, 1:]))  # sep = 3 in a 3 x 3 window: ranks 1, 2 are missing


def test_a_parabola_by_hand():
    """One pixel, ft = 0, so the cost is |A - B shifted| itself.  A = 10 and B's
    row (7, 9, 12): the costs over v = 0, 1, 2 are 3, 1, 2, so the pick is v0 = 1
    with den = (3 - 1) + (2 - 1) = 3 and delta = (3 - 2) / 6."""
    from gqmap_opticalflow_amd import block_match
    A = np.full((1, 3), 10.0, order="F")
    B = np.asfortranarray(np.array([[7.0, 9.0, 12.0]]))
    flow, cost, curv = block_match(A, B, 0, 1, 0, 1.0, host=True, subpixel=True)
    # pixel n = 1 sees B(n + v - 1) = 7, 9, 12
    assert cost[0, 1, 0] == 1.0 and curv[0, 1, 0, 0] == 3.0 and curv[0, 1, 1, 0] == 0.0
    assert flow[0, 1, 0, 0] == 0.0 - (3.0 - 2.0) / 6.0 and flow[0, 1, 1, 0] == 0.0
    # pixel n = 0 sees 0 (outside), 7, 9: costs 10, 3, 1, the pick v0 = 2 is on the window's edge
    assert cost[0, 0, 0] == 1.0 and flow[0, 0, 0, 0] == -1.0 and curv[0, 0, 0, 0] == 0.0


@pytest.mark.parametrize("kw", [dict(H=0), dict(H=5), dict(sep=0), dict(sep=66), dict(U=33), dict(ft=5),
                                dict(sigma=0.0), dict(M=0)], ids=str)
@pytest.mark.parametrize("entry", ["gqmap_block_match_refine_host", "gqmap_block_match_refine"])
def test_argument_errors_write_nothing(entry, kw):
    """The argument checks of gqmap_block_match_multi; the device entry point
    needs no device to apply them, launches nothing and leaves elapsed_ms alone."""
    from gqmap_opticalflow_amd import _lib
    lib = _lib.load()
    a = dict(H=2, sep=2, U=1, ft=1, sigma=1.0, M=4)
    a.update(kw)
    A = np.zeros((4, 4), order="F")
    flow = np.full((4, 4, 2, 4), 77.0, order="F")
    cost = np.full((4, 4, 4), 77.0, order="F")
    curv = np.full((4, 4, 2, 4), 77.0, order="F")
    ms = C.c_double(-1.0)
    args = [_lib.dptr(A), _lib.dptr(A), a["M"], 4, a["U"], 1, a["ft"], C.c_double(a["sigma"]), a["H"], a["sep"],
            _lib.dptr(flow), _lib.dptr(cost), _lib.dptr(curv)]
    if entry == "gqmap_block_match_refine":
        args += [C.cast(C.byref(ms), _lib._D), 0]
    assert getattr(lib, entry)(*args) == 1  # GQMAP_ERR_INVALID_ARG
    assert entry.encode() in lib.gqmap_last_error()
    assert np.all(flow == 77.0) and np.all(cost == 77.0) and np.all(curv == 77.0) and ms.value == -1.0


def test_cost_and_curv_may_be_null():
    from gqmap_opticalflow_amd import _lib
    lib = _lib.load()
    A, B = R.crop_pair(R.CROPS[4])
    flow = np.zeros((5, 7, 2, 2), order="F")
    assert lib.gqmap_block_match_refine_host(_lib.dptr(A), _lib.dptr(B), 5, 7, 3, 3, 2, 1.0, 2, 2, _lib.dptr(flow), None,
                                             None) == 0
    assert np.array_equal(bits(flow), bits(model(R.CROPS[4], (3, 3, 2, 1.0), 2, 2)[0]))


def test_whole_frame_subpixel_start_is_closer_to_the_ground_truth():
    """388 x 584 at the reference defaults: the known-pixel AEPE of the refined
    start is at least 0.05 below the integer start's (a numpy restatement gave
    0.40819 against 0.50003, a gain of 0.0918)."""
    from gqmap_opticalflow_amd import block_match_init
    I1, I2, gt = R.rubberwhale()
    whole, rng = block_match_init(I1, I2, host=True)
    fine, rng2 = block_match_init(I1, I2, subpixel=True, host=True)
    assert rng2 == rng == dict(minu=-7.0, maxu=7.0, minv=-7.0, maxv=7.0) and fine.shape == whole.shape == gt.shape
    assert np.abs(fine - whole).max() <= 0.5
    known = np.all(np.abs(gt) <= 1e9, axis=2)
    epe = lambda f: np.sqrt(np.sum((gt - f) ** 2, axis=2))[known].mean()
    a, b = epe(whole), epe(fine)
    print(f"integer start AEPE {a:.5f}, sub-pixel start AEPE {b:.5f}, gain {a - b:.5f}")
    assert a - b >= 0.05


# ---- initial_state(flow=, sigma=) -----------------------------------------------

def sigmas(M, N, Hs, seed, lo, hi):
    """Widths inside and outside [lo, hi], with one entry of every kind that keeps the draw."""
    rng = np.random.default_rng(seed)
    s = np.asfortranarray(rng.uniform(0.2, 3.0, (M, N, 2, Hs)))
    s[0, 1, 0, 0], s[1, 0, 1, 0], s[2, 2, 0, 0], s[3, 1, 1, 0], s[1, 3, 0, 0] = np.nan, 0.0, -1.5, np.inf, -np.inf
    s[4, 0, 0, 0], s[0, 4, 1, 0] = lo / 4, hi * 3  # clamped
    return s


def test_initial_state_takes_a_width_per_component():
    """The host copy of gqmap_init_state_seeded against the formula: finite
    entries > 0 clamped into sigu / sigv of component l < H; NaN, 0, negative
    and infinite entries keep the draw; later components, the means and every
    other plane are those of initial_state(flow=)."""
    from gqmap_opticalflow_amd import initial_state
    from tests._initflow import make_flow
    o = dict(L=3, minu=-2.0, maxu=3.0, minv=-1.0, maxv=0.5, sig_lo=0.4, sig_hi=2.5)
    M, N = 6, 5
    f = np.stack([make_flow(M, N, seed=s) for s in (1, 2)], axis=3)
    s = sigmas(M, N, 2, 5, 0.4, 2.5)
    base, got = initial_state(o, M, N, seed=3, flow=f), initial_state(o, M, N, seed=3, flow=f, sigma=s)
    kept = 0
    for l in range(2):
        for plane, pbase, x in ((got.sigu, base.sigu, s[:, :, 0, l]), (got.sigv, base.sigv, s[:, :, 1, l])):
            with np.errstate(invalid="ignore"):
                given = np.isfinite(x) & (x > 0)
            assert np.array_equal(plane[:, :, l][given], np.clip(x[given], 0.4, 2.5))
            assert np.array_equal(plane[:, :, l][~given], pbase[:, :, l][~given])
            kept += int((~given).sum())
    assert kept == 5
    assert got.sigu[4, 0, 0] == 0.4 and got.sigv[0, 4, 0] == 2.5
    assert np.all(base.sigu > 2.5)  # the draw is rand + (max - min): visibly not a clamped width
    for k in ("muu", "muv", "pn", "rou", "w", "alpha"):
        assert np.array_equal(getattr(got, k), getattr(base, k)), k
    assert np.array_equal(got.sigu[:, :, 2], base.sigu[:, :, 2]) and np.array_equal(got.sigv[:, :, 2], base.sigv[:, :, 2])
    # the engine's default bounds when the options name none: 0.01 and 23 (mixture)
    d = dict(L=3, minu=-2.0, maxu=3.0, minv=-1.0, maxv=0.5)
    wide = np.full((M, N, 2, 1), 100.0)
    wide[0, 0, 0, 0] = 1e-5
    st = initial_state(d, M, N, seed=3, flow=f[:, :, :, :1], sigma=wide)
    assert st.sigu[0, 0, 0] == 0.01 and st.sigu[1, 1, 0] == 23.0 and st.sigv[0, 0, 0] == 23.0
    assert initial_state(d, M, N, seed=3, engine="super", flow=f[:, :, :, :1], sigma=wide).sigv[0, 0, 0] == 25.0
    # H = 1 is the 3-D call
    one = initial_state(o, M, N, seed=3, flow=f[:, :, :, 0], sigma=s[:, :, :, 0])
    four = initial_state(o, M, N, seed=3, flow=f[:, :, :, :1], sigma=s[:, :, :, :1])
    assert np.array_equal(one.sigu, four.sigu) and np.array_equal(one.sigv, four.sigv)


def test_initial_state_without_sigma_keeps_its_bits():
    from gqmap_opticalflow_amd import initial_state
    from tests._initflow import make_flow
    o = dict(L=3, minu=-2.0, maxu=3.0, minv=-1.0, maxv=0.5)
    f = np.stack([make_flow(6, 5, seed=s) for s in (1, 2)], axis=3)
    a, b = initial_state(o, 6, 5, seed=3, flow=f), initial_state(o, 6, 5, seed=3, flow=f, sigma=None)
    nothing = initial_state(o, 6, 5, seed=3, flow=f, sigma=np.full(f.shape, np.nan))
    for k in ("muu", "muv", "sigu", "sigv", "pn", "rou", "w", "alpha"):
        assert np.array_equal(getattr(a, k), getattr(b, k)) and np.array_equal(getattr(a, k), getattr(nothing, k)), k
    with pytest.raises(ValueError):
        initial_state(o, 6, 5, seed=3, sigma=np.ones((6, 5, 2)))  # a width without a flow
    with pytest.raises(ValueError):
        initial_state(o, 6, 5, seed=3, flow=f, sigma=np.ones((6, 5, 2)))  # H differs


# ---- block_match_init(subpixel=, sigma_from_cost=) --------------------------------

PAR = (3, 3, 2, 1.0)


def test_block_match_init_sigma_is_the_formula():
    from gqmap_opticalflow_amd import block_match, block_match_init
    I1, I2 = R.crop_pair(R.CROPS[0])
    out, cost, curv = block_match(I1, I2, *PAR, host=True, hypotheses=3, subpixel=True)
    rng = dict(minu=-3.0, maxu=3.0, minv=-3.0, maxv=3.0)
    flow, ranges = block_match_init(I1, I2, *PAR, host=True, hypotheses=3, subpixel=True)
    assert ranges == rng and np.array_equal(flow, 0.0 - out)
    for lambdad, floor in ((1.0, 0.5), (4.0, 0.1)):
        flow2, ranges, sig = block_match_init(I1, I2, *PAR, host=True, hypotheses=3, subpixel=True,
                                              sigma_from_cost=True, lambdad=lambdad, sigma_min=floor)
        assert ranges == rng and np.array_equal(flow2, flow) and sig.shape == flow.shape
        pos = curv > 0
        assert pos.any() and (~pos).any()
        assert np.all(np.isnan(sig[~pos]))
        want = np.maximum(np.sqrt(1.0 / (lambdad * curv[pos])), floor)
        assert np.array_equal(sig[pos], want)
        assert sig[pos].min() == floor and np.any(sig[pos] > floor)
    # without hypotheses: three-dimensional, rank 0
    f1, _, s1 = block_match_init(I1, I2, *PAR, host=True, subpixel=True, sigma_from_cost=True)
    assert f1.shape == s1.shape == (40, 48, 2)
    _, _, s3 = block_match_init(I1, I2, *PAR, host=True, hypotheses=3, subpixel=True, sigma_from_cost=True)
    assert np.array_equal(f1, flow[..., 0]) and np.array_equal(s1, s3[..., 0], equal_nan=True)
    with pytest.raises(ValueError):
        block_match_init(I1, I2, *PAR, host=True, sigma_from_cost=True)


def test_super_nodes_sum_the_curvature_at_rank_0_and_take_the_cheapest_pixel_after():
    from gqmap_opticalflow_amd import block_match, block_match_init
    I1, I2 = R.crop_pair(R.CROPS[0])
    out, cost, curv = block_match(I1, I2, *PAR, host=True, hypotheses=3, subpixel=True)
    flow, _, sig = block_match_init(I1, I2, *PAR, engine="super", host=True, hypotheses=3, subpixel=True,
                                    sigma_from_cost=True)
    assert flow.shape == sig.shape == (10, 12, 2, 3)
    assert np.array_equal(flow[..., 0], (0.0 - out[..., 0]).reshape(10, 4, 12, 4, 2).mean(axis=(1, 3)))
    ksum = curv[..., 0].reshape(10, 4, 12, 4, 2).sum(axis=(1, 3))
    assert np.all(ksum > 0)
    assert np.array_equal(sig[..., 0], np.maximum(np.sqrt(1.0 / ksum), 0.5))
    for k in (1, 2):
        for i, j in ((0, 0), (3, 5), (9, 11)):
            blk = cost[4 * i:4 * i + 4, 4 * j:4 * j + 4, k]
            p = int(np.argmin(blk.ravel(order="F")))  # column-major order of the block, first on ties
            m, n = 4 * i + p % 4, 4 * j + p // 4
            assert np.array_equal(flow[i, j, :, k], 0.0 - out[m, n, :, k])
            kk = curv[m, n, :, k]
            with np.errstate(divide="ignore"):
                want = np.where(kk > 0, np.maximum(np.sqrt(1.0 / kk), 0.5), np.nan)
            assert np.array_equal(sig[i, j, :, k], want, equal_nan=True)
    # without sigma_from_cost the flows are the same
    flow2, _ = block_match_init(I1, I2, *PAR, engine="super", host=True, hypotheses=3, subpixel=True)
    assert np.array_equal(flow2, flow)
