"""The forward-backward check and the fill without a device: the library's host
models (gqmap_flow_consistency_host, gqmap_flow_fill_host) against the numpy
restatement of csrc/gqmap_flowcheck.h (tests/_flowcheck_np.py) BIT FOR BIT,
closed forms of both, argument errors, and block_match_init(consistency=,
fill=) on crops and on the whole RubberWhale pair.  The kernels against the
host models: tests/test_gpu_flow_check.py."""
import ctypes as C
import re

import numpy as np
import pytest

from tests import _blockmatch_np as R
from tests import _codeobj
from tests import _flowcheck_np as F
from tests._flowcheck_np import bits

NAN_BITS = 0x7FF8000000000000


def host_check(fwd, bwd, a1=0.01, a2=0.5):
    from gqmap_opticalflow_amd import flow_consistency
    return flow_consistency(fwd, bwd, a1, a2, host=True)


def host_fill(flow, mask, r=8, sigma=4.0, passes=2):
    from gqmap_opticalflow_amd import flow_fill
    return flow_fill(flow, mask, r, sigma, passes, host=True)


def const(M, N, u, v):
    return np.asfortranarray(np.broadcast_to(np.array([u, v], dtype=np.float64), (M, N, 2)))


# ---- host models against the restatement -----------------------------------------

@pytest.mark.parametrize("params", F.PARAMS, ids=str)
@pytest.mark.parametrize("crop", R.CROPS, ids=str)
def test_host_check_equals_the_restatement(crop, params):
    fwd, bwd = F.fields(crop, params)
    for a1, a2 in ((0.01, 0.5), (0.0, 0.05)):
        err, mask = host_check(fwd, bwd, a1, a2)
        rerr, rmask = F.check(fwd, bwd, a1, a2)
        assert np.array_equal(bits(err), bits(rerr))
        assert mask.dtype == bool and np.array_equal(mask, rmask)


@pytest.mark.parametrize("params", F.PARAMS, ids=str)
@pytest.mark.parametrize("crop", R.CROPS, ids=str)
def test_host_fill_equals_the_restatement(crop, params):
    fwd, bwd = F.fields(crop, params)
    mask = F.check(fwd, bwd, 0.01, 0.5)[1]
    for r in (0, 1, 8, 16):
        for passes in (1, 3):
            out, filled = host_fill(fwd, mask, r, 0.5 * r + 0.5, passes)
            rout, rfilled = F.fill(fwd, mask, r, 0.5 * r + 0.5, passes)
            assert np.array_equal(bits(out), bits(rout)), (r, passes)
            assert filled.dtype == np.uint8 and np.array_equal(filled, rfilled), (r, passes)


def test_the_crops_reject_and_refill_something():
    """The two tests above are not vacuous: the masks have both values and the fill fills."""
    fwd, bwd = F.fields(R.CROPS[0], F.PARAMS[0])
    mask = host_check(fwd, bwd)[1]
    assert 0 < (~mask).sum() < mask.size
    filled = host_fill(fwd, mask, 1, 1.0, 1)[1]
    assert (filled == 1).any() and (filled == 0).sum() == mask.sum()


# ---- closed forms of the check -----------------------------------------------------

def test_zero_flows_are_consistent():
    z = np.zeros((9, 7, 2), order="F")
    err, mask = host_check(z, z)
    assert np.all(err == 0) and mask.all()


def test_constant_flows_that_cancel():
    M, N = 9, 11
    err, mask = host_check(const(M, N, 2.0, -1.0), const(M, N, -2.0, 1.0))
    m, n = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    inside = (n + 2 <= N - 1) & (m - 1 >= 0)
    assert np.all(err[inside] == 0) and mask[inside].all()
    assert np.all(np.isposinf(err[~inside])) and not mask[~inside].any()
    assert inside.any() and (~inside).any()


def test_the_threshold_itself_is_consistent():
    """fwd = (1, 0), bwd = 0: e2 = 1, mag = 1, thr = a1 + a2."""
    M, N = 4, 5
    fwd, z = const(M, N, 1.0, 0.0), np.zeros((M, N, 2), order="F")
    err, mask = host_check(fwd, z, 0.0, 1.0)
    assert np.all(err[:, :N - 1] == 1) and mask[:, :N - 1].all() and not mask[:, N - 1].any()
    assert host_check(fwd, z, 0.5, 0.5)[1][:, :N - 1].all()
    assert not host_check(fwd, z, 0.0, np.nextafter(1.0, 0.0))[1].any()


def test_zero_thresholds_accept_exact_cancellation_only():
    M, N = 6, 6
    fwd = const(M, N, 0.5, 0.25)
    bwd = const(M, N, -0.5, -0.25).copy(order="F")
    bwd[2, 2, 0] = -0.5 + 2.0 ** -40  # every bilinear weight here is a multiple of 1/8: the residue survives
    err, mask = host_check(fwd, bwd, 0.0, 0.0)
    m, n = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    inside = (n <= N - 2) & (m <= M - 2)  # targets (m + 0.25, n + 0.5)
    touched = inside & (m >= 1) & (m <= 2) & (n >= 1) & (n <= 2)  # the four pixels that sample (2, 2)
    assert np.array_equal(mask, inside & ~touched)
    assert np.all(err[mask] == 0) and np.all(err[touched] > 0)


def test_nan_anywhere_is_inconsistent():
    M, N = 7, 8
    fwd, bwd = const(M, N, 0.5, 0.5).copy(order="F"), np.zeros((M, N, 2), order="F")
    bwd[3, 3, 0] = np.nan
    fwd[5, 1, 1] = np.nan
    err, mask = host_check(fwd, bwd)
    m, n = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    inside = (n <= N - 2) & (m <= M - 2)
    sampled = (m >= 2) & (m <= 3) & (n >= 2) & (n <= 3)  # cells m..m+1, n..n+1 hold (3, 3)
    want = inside & ~sampled
    want[5, 1] = False
    assert np.array_equal(mask, want)
    assert np.all(np.isnan(err[sampled])) and np.isposinf(err[5, 1]) and np.all(err[want] == 0.5)
    # a NaN in the other plane of bwd, and one whose bilinear weight is zero
    bwd2 = np.zeros((M, N, 2), order="F")
    bwd2[3, 3, 1] = np.nan
    assert np.array_equal(host_check(const(M, N, 0.5, 0.5), bwd2)[1], inside & ~sampled)
    assert not host_check(np.zeros((M, N, 2), order="F"), bwd2)[1][3, 3]


def test_a_target_on_the_last_row_and_column():
    M, N = 6, 9
    rng = np.random.default_rng(3)
    bwd = np.asfortranarray(rng.uniform(-1, 1, (M, N, 2)))
    m, n = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    fwd = np.asfortranarray(np.stack([(N - 1 - n).astype(np.float64), (M - 1 - m).astype(np.float64)], axis=2))
    err, mask = host_check(fwd, bwd, 0.0, 1e300)
    b0, b1 = bwd[M - 1, N - 1]
    want = (fwd[:, :, 0] + b0) ** 2 + (fwd[:, :, 1] + b1) ** 2
    assert np.array_equal(err, want) and mask.all()
    past = fwd.copy(order="F")
    past[2, 0, 0] = np.nextafter(past[2, 0, 0], np.inf)  # n = 0, m = 0: the sums n + u, m + v are exact
    past[0, 4, 1] = np.nextafter(past[0, 4, 1], np.inf)
    err2, mask2 = host_check(past, bwd, 0.0, 1e300)
    assert np.isposinf(err2[2, 0]) and np.isposinf(err2[0, 4]) and (~mask2).sum() == 2
    # a single pixel, a single row, a single column
    one = np.zeros((1, 1, 2), order="F")
    assert host_check(one, one)[1].all()
    row = np.zeros((1, 5, 2), order="F")
    row[0, :, 0] = 0.5
    e, k = host_check(row, np.zeros((1, 5, 2), order="F"), 0.0, 0.25)
    assert np.array_equal(e[0], [0.25] * 4 + [np.inf]) and np.array_equal(k[0], [True] * 4 + [False])


# ---- closed forms of the fill --------------------------------------------------------

def noisy(M, N, seed=0):
    return np.asfortranarray(np.random.default_rng(seed).uniform(-4, 4, (M, N, 2)))


def hole(M=64, N=64, lo=12, hi=52):
    mask = np.ones((M, N), dtype=bool)
    mask[lo:hi, lo:hi] = False
    return mask


def test_an_all_valid_mask_is_a_copy():
    f = noisy(33, 21)
    out, filled = host_fill(f, np.ones((33, 21), dtype=bool))
    assert np.array_equal(bits(out), bits(f)) and not filled.any()


def test_an_all_invalid_mask_leaves_the_input():
    f = noisy(33, 21)
    f[4, 4, 0] = np.nan
    out, filled = host_fill(f, np.zeros((33, 21), dtype=bool), 8, 4.0, 3)
    assert np.array_equal(bits(out), bits(f)) and np.all(filled == 255)


def test_radius_zero_fills_nothing():
    f = noisy(20, 24)
    mask = np.random.default_rng(1).uniform(size=(20, 24)) < 0.5
    out, filled = host_fill(f, mask, 0, 1.0, 2)
    assert np.array_equal(bits(out), bits(f)) and np.array_equal(filled, np.where(mask, 0, 255))


def test_what_invalid_pixels_store_reaches_nothing():
    f, mask = noisy(64, 64), hole()
    clean, filled = host_fill(f, mask, 8, 4.0, 2)
    dirty = f.copy(order="F")
    dirty[20:30, 20:50, 0], dirty[30:40, 12:52, 1], dirty[12, 12, :] = np.nan, np.inf, -np.inf
    out, filled2 = host_fill(dirty, mask, 8, 4.0, 2)
    done = filled != 255
    assert np.array_equal(filled, filled2) and (filled == 1).any() and (filled == 2).any() and (~done).any()
    assert np.array_equal(bits(out)[done], bits(clean)[done]) and np.all(np.isfinite(out[done]))
    assert np.array_equal(bits(out)[~done], bits(dirty)[~done])


def test_a_hole_wider_than_the_window_needs_several_passes():
    f, mask = noisy(64, 64), hole()
    out1, filled1 = host_fill(f, mask, 8, 4.0, 1)
    want = np.zeros((64, 64), dtype=np.uint8)
    want[12:52, 12:52], want[20:44, 20:44] = 1, 255
    assert np.array_equal(filled1, want) and (filled1 == 255).sum() == 24 * 24
    out3, filled3 = host_fill(f, mask, 8, 4.0, 3)
    want[20:44, 20:44], want[28:36, 28:36] = 2, 3
    assert np.array_equal(filled3, want) and not (filled3 == 255).any()
    # a pass is a pass: three passes are one pass applied three times
    step, st = f, mask
    for _ in range(3):
        step, fl = host_fill(step, st, 8, 4.0, 1)
        st = fl != 255
    assert np.array_equal(bits(step), bits(out3))
    # the refilled values lie within the range of the valid ones
    assert out3.min() >= f[mask].min() and out3.max() <= f[mask].max()


def test_a_constant_field_is_refilled_with_the_constant():
    """Within 1 ulp where the arithmetic grants it: a constant c = +-2^k scales
    every product and sum exactly, Y_S = c Y_V bit for bit, and the correctly
    rounded quotient is c.  For any other constant the fixed-order sums do not
    grant 1 ulp: Y_S and Y_V each carry 2 (2r + 2) roundings (a product and a sum
    per tap, rows and columns, all terms of one sign), so with k = 4r + 4 their
    quotient is within (2k + 1) u of c relatively, at most 2k + 2 ulp, per pass;
    a later pass averages values that are already that far off.  Measured on
    (2.75, -1.3), r = 8, three passes: 5 ulp."""
    mask = hole()
    out, filled = host_fill(const(64, 64, 2.0, -0.5), mask, 8, 4.0, 3)
    assert not (filled == 255).any()
    for c, v in ((0, 2.0), (1, -0.5)):
        ulps = np.abs(out[:, :, c] - v) / np.spacing(abs(v))
        print(f"c = {v}: largest deviation {ulps.max():.2f} ulp")
        assert ulps.max() <= 1.0
    r, passes = 8, 3
    out, filled = host_fill(const(64, 64, 2.75, -1.3), mask, r, 4.0, passes)
    for c, v in ((0, 2.75), (1, -1.3)):
        ulps = np.abs(out[:, :, c] - v) / np.spacing(abs(v))
        print(f"c = {v}: largest deviation {ulps.max():.2f} ulp")
        assert np.all(ulps[mask] == 0) and ulps.max() <= passes * (2 * (4 * r + 4) + 2)


# ---- arguments -------------------------------------------------------------------------

def test_bad_arguments_write_nothing():
    from gqmap_opticalflow_amd import _lib
    lib = _lib.load()
    M, N = 5, 6
    f, b = noisy(M, N, 1), noisy(M, N, 2)
    err = np.full((M, N), 7.0, order="F")
    mask = np.full((M, N), 9, dtype=np.uint8, order="F")
    D, U8 = _lib.dptr, _lib.u8ptr
    nan = float("nan")
    for name, tail in (("gqmap_flow_consistency_host", ()), ("gqmap_flow_consistency", (None, 0))):
        fn = getattr(lib, name)
        for args in ((D(f), D(b), 0, N, 0.01, 0.5, D(err), U8(mask)), (D(f), D(b), M, 0, 0.01, 0.5, D(err), U8(mask)),
                     (D(f), D(b), M, N, -0.01, 0.5, D(err), U8(mask)), (D(f), D(b), M, N, 0.01, nan, D(err), U8(mask)),
                     (D(f), D(b), M, N, float("inf"), 0.5, D(err), U8(mask)), (None, D(b), M, N, 0.01, 0.5, D(err), U8(mask)),
                     (D(f), None, M, N, 0.01, 0.5, D(err), U8(mask)), (D(f), D(b), M, N, 0.01, 0.5, None, None)):
            assert fn(*args, *tail) == 1
            assert name.encode() + b":" in lib.gqmap_last_error()
    assert np.all(err == 7.0) and np.all(mask == 9)
    out = np.full((M, N, 2), 7.0, order="F")
    k = np.ones((M, N), dtype=np.uint8, order="F")
    for name, tail in (("gqmap_flow_fill_host", ()), ("gqmap_flow_fill", (None, 0))):
        fn = getattr(lib, name)
        for args in ((D(f), U8(k), 0, N, 8, 4.0, 2, D(out), U8(mask)), (D(f), U8(k), M, N, -1, 4.0, 2, D(out), U8(mask)),
                     (D(f), U8(k), M, N, 17, 4.0, 2, D(out), U8(mask)), (D(f), U8(k), M, N, 8, 0.0, 2, D(out), U8(mask)),
                     (D(f), U8(k), M, N, 8, nan, 2, D(out), U8(mask)), (D(f), U8(k), M, N, 8, 4.0, 0, D(out), U8(mask)),
                     (D(f), U8(k), M, N, 8, 4.0, 9, D(out), U8(mask)), (None, U8(k), M, N, 8, 4.0, 2, D(out), U8(mask)),
                     (D(f), None, M, N, 8, 4.0, 2, D(out), U8(mask)), (D(f), U8(k), M, N, 8, 4.0, 2, None, U8(mask))):
            assert fn(*args, *tail) == 1
            assert name.encode() + b":" in lib.gqmap_last_error()
    assert np.all(out == 7.0) and np.all(mask == 9)
    from gqmap_opticalflow_amd import flow_consistency, flow_fill
    with pytest.raises(ValueError):
        flow_consistency(f, noisy(M, N + 1), host=True)
    with pytest.raises(ValueError):
        flow_fill(f, np.ones((M, N + 1)), host=True)


def test_outputs_may_be_null():
    from gqmap_opticalflow_amd import _lib
    lib = _lib.load()
    fwd, bwd = F.fields(R.CROPS[3], F.PARAMS[0])
    M, N, _ = fwd.shape
    err, mask = host_check(fwd, bwd)
    e = np.zeros((M, N), order="F")
    k = np.zeros((M, N), dtype=np.uint8, order="F")
    assert lib.gqmap_flow_consistency_host(_lib.dptr(fwd), _lib.dptr(bwd), M, N, 0.01, 0.5, _lib.dptr(e), None) == 0
    assert lib.gqmap_flow_consistency_host(_lib.dptr(fwd), _lib.dptr(bwd), M, N, 0.01, 0.5, None, _lib.u8ptr(k)) == 0
    assert np.array_equal(bits(e), bits(err)) and np.array_equal(k, mask.astype(np.uint8))
    out, _ = host_fill(fwd, mask)
    o = np.zeros((M, N, 2), order="F")
    assert lib.gqmap_flow_fill_host(_lib.dptr(fwd), _lib.u8ptr(k), M, N, 8, 4.0, 2, _lib.dptr(o), None) == 0
    assert np.array_equal(bits(o), bits(out))
    # any non-zero mask byte is "valid"
    assert lib.gqmap_flow_fill_host(_lib.dptr(fwd), _lib.u8ptr(np.asfortranarray(k * 200)), M, N, 8, 4.0, 2, _lib.dptr(o),
                                    None) == 0
    assert np.array_equal(bits(o), bits(out))


# ---- block_match_init(consistency=, fill=) -------------------------------------------------

PAR = (3, 3, 2, 1.0)


def test_without_consistency_nothing_changes():
    from gqmap_opticalflow_amd import block_match_init
    I1, I2 = R.crop_pair(R.CROPS[0])
    for kw in (dict(), dict(hypotheses=3), dict(subpixel=True), dict(hypotheses=3, subpixel=True, sigma_from_cost=True),
               dict(engine="super", hypotheses=2, subpixel=True, sigma_from_cost=True)):
        a = block_match_init(I1, I2, *PAR, host=True, **kw)
        b = block_match_init(I1, I2, *PAR, host=True, consistency=False, fill=False, fb_a1=0.3, fill_r=2, **kw)
        assert len(a) == len(b) == (3 if "sigma_from_cost" in kw else 2) and a[1] == b[1]
        for x, y in zip(a[::2], b[::2]):
            assert x.shape == y.shape and np.array_equal(bits(x), bits(y))
    with pytest.raises(ValueError):
        block_match_init(I1, I2, *PAR, host=True, fill=True)


def test_consistency_marks_the_ranks_on_the_pixel_grid():
    from gqmap_opticalflow_amd import block_match, block_match_init
    I1, I2 = R.crop_pair(R.CROPS[0])
    raw, rng, rsig = block_match_init(I1, I2, *PAR, host=True, hypotheses=3, subpixel=True, sigma_from_cost=True)
    flow, rng2, sig, cons = block_match_init(I1, I2, *PAR, host=True, hypotheses=3, subpixel=True, sigma_from_cost=True,
                                             consistency=True)
    assert rng2 == rng and flow.shape == sig.shape == raw.shape and cons.shape == (40, 48, 3) and cons.dtype == bool
    bwd = block_match_init(I2, I1, *PAR, host=True, subpixel=True)[0]
    for k in range(3):
        want = F.check(raw[:, :, :, k], bwd, 0.01, 0.5)[1]
        assert np.array_equal(cons[:, :, k], want)
        assert 0 < want.sum() < want.size
        both = np.broadcast_to(want[:, :, None], (40, 48, 2))
        assert np.array_equal(bits(flow[:, :, :, k])[both], bits(raw[:, :, :, k])[both])
        assert np.all(bits(flow[:, :, :, k])[~both] == NAN_BITS) and np.all(np.isnan(sig[:, :, :, k][~both]))
        assert np.array_equal(bits(sig[:, :, :, k])[both], bits(rsig[:, :, :, k])[both])
    assert not cons[np.isnan(raw[:, :, 0, :])].any()  # a missing rank is inconsistent
    # other thresholds reach the check
    loose = block_match_init(I1, I2, *PAR, host=True, hypotheses=3, subpixel=True, consistency=True, fb_a2=50.0)[-1]
    assert loose.sum() > cons.sum()
    # without hypotheses: rank 0 alone, three- and two-dimensional; the integer matcher too
    f1, _, c1 = block_match_init(I1, I2, *PAR, host=True, subpixel=True, consistency=True)
    assert f1.shape == (40, 48, 2) and np.array_equal(c1, cons[:, :, 0]) and np.array_equal(bits(f1), bits(flow[..., 0]))
    fi, _, ci = block_match_init(I1, I2, *PAR, host=True, consistency=True)
    ri, bi = block_match_init(I1, I2, *PAR, host=True)[0], block_match_init(I2, I1, *PAR, host=True)[0]
    assert np.array_equal(ci, F.check(ri, bi, 0.01, 0.5)[1]) and np.array_equal(fi[ci], ri[ci]) and np.all(np.isnan(fi[~ci]))


def test_fill_replaces_rank_zero_only():
    from gqmap_opticalflow_amd import block_match_init
    I1, I2 = R.crop_pair(R.CROPS[0])
    kw = dict(host=True, hypotheses=3, subpixel=True, sigma_from_cost=True, consistency=True)
    raw = block_match_init(I1, I2, *PAR, host=True, hypotheses=3, subpixel=True)[0]
    flow, _, sig, cons = block_match_init(I1, I2, *PAR, **kw)
    for r, passes in ((2, 1), (8, 2)):
        ff, _, fsig, fcons = block_match_init(I1, I2, *PAR, fill=True, fill_r=r, fill_sigma=1.5, fill_passes=passes, **kw)
        want, state = F.fill(raw[:, :, :, 0], cons[:, :, 0], r, 1.5, passes)
        want[state == 255] = np.nan
        assert np.array_equal(fcons, cons) and np.array_equal(bits(fsig), bits(sig))  # a filled flow keeps the wide draw
        assert np.array_equal(bits(ff[:, :, :, 0]), bits(want)) and (state >= 1).any()
        assert np.array_equal(bits(ff[:, :, :, 1:]), bits(flow[:, :, :, 1:]))
        assert np.all(np.isnan(fsig[:, :, :, 0][~cons[:, :, 0]]))


def test_super_nodes_under_consistency():
    """24 x 20: rank 0 of a node is the mean over the block's pixels that are
    not NaN, its curvature the sum over the consistent pixels; ranks k >= 1 take
    the cheapest pixel among the consistent ones."""
    from gqmap_opticalflow_amd import block_match, block_match_init
    I1, I2 = (np.asfortranarray(a[:24, :20]) for a in R.crop_pair(R.CROPS[0]))
    out, cost, curv = block_match(I1, I2, *PAR, host=True, hypotheses=3, subpixel=True)
    raw = 0.0 - out
    kw = dict(host=True, hypotheses=3, subpixel=True, sigma_from_cost=True, consistency=True)
    pflow, _, _, cons = block_match_init(I1, I2, *PAR, **kw)
    nflow, rng, nsig, ncons = block_match_init(I1, I2, *PAR, engine="super", **kw)
    assert nflow.shape == nsig.shape == (6, 5, 2, 3) and ncons.shape == (24, 20, 3) and np.array_equal(ncons, cons)
    filled = block_match_init(I1, I2, *PAR, engine="super", fill=True, fill_r=1, fill_sigma=1.0, fill_passes=1, **kw)
    pfill = block_match_init(I1, I2, *PAR, fill=True, fill_r=1, fill_sigma=1.0, fill_passes=1, **kw)[0]
    # rank 0: block sums over (rows, columns) of the block, as the node rule of the plain start
    blocks = lambda x: x.reshape(6, 4, 5, 4, 2)
    ok = np.broadcast_to(cons[:, :, None, 0], (24, 20, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        count = blocks(ok).sum(axis=(1, 3))
        want = np.where(count > 0, blocks(np.where(ok, raw[..., 0], 0.0)).sum(axis=(1, 3)) / count, np.nan)
        ksum = blocks(np.where(ok, curv[..., 0], 0.0)).sum(axis=(1, 3))
        wsig = np.where(ksum > 0, np.maximum(np.sqrt(1.0 / ksum), 0.5), np.nan)
        known = ~np.isnan(pfill[..., 0])
        kcount = blocks(known).sum(axis=(1, 3))
        wfill = np.where(kcount > 0, blocks(np.where(known, pfill[..., 0], 0.0)).sum(axis=(1, 3)) / kcount, np.nan)
    assert np.array_equal(nflow[..., 0], want, equal_nan=True) and np.array_equal(nsig[..., 0], wsig, equal_nan=True)
    assert np.array_equal(filled[0][..., 0], wfill, equal_nan=True) and np.array_equal(filled[2][..., 0], wsig, equal_nan=True)
    assert (count < 16).any() and (kcount > count).any()
    i, j = np.argwhere((count[:, :, 0] > 0) & (count[:, :, 0] < 16))[0]  # one node by hand, to a rounding
    sel = cons[4 * i:4 * i + 4, 4 * j:4 * j + 4, 0]
    np.testing.assert_allclose(nflow[i, j, :, 0], raw[4 * i:4 * i + 4, 4 * j:4 * j + 4, :, 0][sel].mean(axis=0), rtol=1e-14)
    for i in range(6):
        for j in range(5):
            blk = (slice(4 * i, 4 * i + 4), slice(4 * j, 4 * j + 4))
            for k in (1, 2):
                ck = np.where(cons[blk + (k,)], cost[blk + (k,)], np.inf)
                p = int(np.argmin(ck.ravel(order="F")))
                m, n = 4 * i + p % 4, 4 * j + p // 4
                if cons[m, n, k]:
                    assert np.array_equal(nflow[i, j, :, k], raw[m, n, :, k])
                    kk = curv[m, n, :, k]
                    with np.errstate(divide="ignore"):
                        assert np.array_equal(nsig[i, j, :, k], np.where(kk > 0, np.maximum(np.sqrt(1.0 / kk), 0.5), np.nan),
                                              equal_nan=True)
                else:  # no consistent pixel in the block at this rank
                    assert not cons[blk + (k,)].any()
                    assert np.all(np.isnan(nflow[i, j, :, k])) and np.all(np.isnan(nsig[i, j, :, k]))
    assert (~cons[:, :, 0]).any() and (~cons[:, :, 1]).any()
    # a block with no consistent pixel at all
    gone = block_match_init(I1, I2, *PAR, engine="super", fb_a2=0.0, fb_a1=0.0, **kw)
    none = ~gone[3][:, :, 0].reshape(6, 4, 5, 4).any(axis=(1, 3))
    assert none.any() and np.all(np.isnan(gone[0][:, :, :, 0][none])) and np.all(np.isnan(gone[2][:, :, :, 0][none]))


def test_whole_frame_check_separates_and_the_fill_improves_the_start():
    """Full RubberWhale, (7, 7, 3, 1.7), sub-pixel rank 0, a1 = 0.01, a2 = 0.5,
    fill r = 8, sigma = 4, two passes; AEPE over the known pixels.  An
    independent numpy run gave: consistent share 0.924, AEPE 0.4082 over all
    pixels, 0.2557 over the consistent ones, 0.2995 after the fill."""
    from gqmap_opticalflow_amd import block_match_init
    I1, I2, gt = R.rubberwhale()
    raw, _ = block_match_init(I1, I2, subpixel=True, host=True)
    flow, _, cons = block_match_init(I1, I2, subpixel=True, host=True, consistency=True)
    fill, _, cons2 = block_match_init(I1, I2, subpixel=True, host=True, consistency=True, fill=True)
    assert cons.shape == gt.shape[:2] and np.array_equal(cons, cons2)
    assert np.array_equal(bits(flow)[cons], bits(raw)[cons]) and np.all(np.isnan(flow[~cons]))
    assert np.array_equal(bits(fill)[cons], bits(raw)[cons])
    known = np.all(np.abs(gt) <= 1e9, axis=2)
    epe = lambda f, sel: np.sqrt(np.sum((gt - f) ** 2, axis=2))[sel].mean()
    share = cons.mean()
    a_all, a_cons, a_rej, a_fill = epe(raw, known), epe(raw, known & cons), epe(raw, known & ~cons), epe(fill, known)
    print(f"consistent share {share:.4f}; AEPE all {a_all:.4f}, consistent {a_cons:.4f}, rejected {a_rej:.4f}, "
          f"filled start {a_fill:.4f}; NaN left at rank 0: {int(np.isnan(fill).sum())}")
    assert share >= 0.85
    assert a_all - a_cons >= 0.10
    assert a_all - a_fill >= 0.05
    assert not np.isnan(fill).any()


# ---- the kernels' listing ------------------------------------------------------------------

CU_LDS = 160 * 1024


@pytest.mark.skipif(not _codeobj.available(), reason="library or ROCm LLVM tools absent")
def test_kernels_have_no_scratch_and_the_fill_fits_the_lds():
    """The gfx950 code object's metadata (tests/_codeobj.py).  The fill's tile is dynamic LDS, 8 W (3 W + 32) bytes with
    W = 32 + 2r, on top of what the kernel holds statically."""
    from gqmap_opticalflow_amd import _lib
    seen = {k: (v["private_segment_fixed_size"], v["group_segment_fixed_size"], v["vgpr_spill_count"])
            for k, v in _codeobj.kernels().items() if re.search(r"k_flow_(check|fill)", k)}
    check = [v for k, v in seen.items() if "k_flow_check" in k]
    fill = [v for k, v in seen.items() if "k_flow_fill" in k]
    assert len(check) == 1 and len(fill) == 1, sorted(seen)
    for scratch, _, spills in check + fill:
        assert scratch == 0 and spills == 0
    assert check[0][1] == 0
    lib = _lib.load()
    lib.gqmap_debug_flow_fill_lds.restype, lib.gqmap_debug_flow_fill_lds.argtypes = C.c_int, [C.c_int]
    lib.gqmap_debug_flow_fill_tile.restype = C.c_int
    S = lib.gqmap_debug_flow_fill_tile()
    for r in range(17):
        W = S + 2 * r
        assert lib.gqmap_debug_flow_fill_lds(r) == 8 * W * (3 * W + S)
    assert lib.gqmap_debug_flow_fill_lds(16) + fill[0][1] <= CU_LDS
    assert lib.gqmap_debug_flow_fill_lds(17) == -1
