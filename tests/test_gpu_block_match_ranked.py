"""gqmap_block_match_window_multi and gqmap_block_match_pyramid_multi (the HIP
kernel k_block_match_window, RANKED) against their host models: one header
(csrc/gqmap_blockmatch.h) behind both, so flow, cost and curvature of every rank
agree BIT FOR BIT, NaN patterns included, whatever the tile width and the chunk
extent; the host models are checked against numpy in
tests/test_block_match_ranked.py."""
import ctypes as C

import numpy as np
import pytest

from tests import _blockmatch_np as R
from tests import _blockmatch_ranked_np as K
from tests import _blockmatch_window_np as W
from tests._blockmatch_gpu import NAN_BITS, assert_bit_equal, bits, force_cols

pytestmark = pytest.mark.gpu

HS = ((2, 1), (3, 2), (4, 3))  # (H, sep)


def force_chunk(cu, cv):
    from gqmap_opticalflow_amd import _lib
    f = _lib.load().gqmap_debug_block_match_chunk
    f.restype, f.argtypes = C.c_int, [C.c_int, C.c_int]
    assert f(cu, cv) == 0


def both(A, B, win, ft, sigma, H, sep, subpixel):
    from gqmap_opticalflow_amd import block_match_window
    kw = dict(subpixel=subpixel, hypotheses=H, sep=sep)
    return block_match_window(A, B, win, ft, sigma, **kw), block_match_window(A, B, win, ft, sigma, host=True, **kw)


def both_pyramid(A, B, params, levels, r, k, H, sep, subpixel):
    from gqmap_opticalflow_amd import block_match_pyramid
    kw = dict(levels=levels, r=r, k=k, subpixel=subpixel, hypotheses=H, sep=sep)
    return block_match_pyramid(A, B, *params, **kw), block_match_pyramid(A, B, *params, host=True, **kw)


def rank(out, j):
    return [a[..., j] for a in out]


def windows_97x130(kind, H):
    return K.make_ranked_windows(97, 130, 7, 7, kind, H, seed=3)


@pytest.mark.parametrize("subpixel", [False, True], ids=["integer", "subpixel"])
@pytest.mark.parametrize("hs", HS, ids=str)
@pytest.mark.parametrize("kind", W.KINDS)
@pytest.mark.parametrize("params", R.PARAMS[:3], ids=str)
@pytest.mark.parametrize("crop", R.CROPS, ids=str)
def test_kernel_equals_host_model(crop, params, kind, hs, subpixel):
    """40 x 48, 33 x 17 and 5 x 7: the smallest are a tile with mostly empty lanes."""
    assert_bit_equal(*both(*R.crop_pair(crop), K.windows(crop, params, kind, hs[0]), params[2], params[3], *hs, subpixel))


@pytest.mark.parametrize("kind", W.KINDS)
@pytest.mark.parametrize("cols", [0, 8, 16, 32])
def test_several_tiles_with_partial_tiles_at_every_tile_width(cols, kind):
    """97 x 130: four tile rows, the last tile of each row and column partial;
    8, 16, 32 force each instantiation."""
    A, B = W.pair_97x130()
    try:
        force_cols(cols)
        for subpixel in (False, True):
            assert_bit_equal(*both(A, B, windows_97x130(kind, 3), 3, 1.7, 3, 2, subpixel))
    finally:
        force_cols(0)


@pytest.mark.parametrize("kind", W.KINDS)
@pytest.mark.parametrize("chunk", [(5, 5), (1, 1), (3, 65)], ids=str)
def test_a_window_over_several_chunks(chunk, kind):
    """The chunk extent forced: picks and their neighbours cross chunk borders,
    and the exclusion by an earlier rank's pick is applied in chunks that do not
    hold that pick."""
    A, B = W.pair_97x130()
    win = windows_97x130(kind, 4)
    try:
        force_chunk(*chunk)
        for subpixel in (False, True):
            assert_bit_equal(*both(A, B, win, 3, 1.7, 4, 2, subpixel))
        if chunk == (5, 5):
            force_cols(8)
            assert_bit_equal(*both(A, B, win, 3, 1.7, 4, 3, True))
    finally:
        force_chunk(0, 0)
        force_cols(0)


@pytest.mark.parametrize("shape", [(1, 1), (64, 1), (1, 64)], ids=str)
def test_degenerate_images(shape):
    I1, I2, _ = R.rubberwhale()
    M, N = shape
    A, B = (np.asfortranarray(a[120:120 + M, 250:250 + N]) for a in (I1, I2))
    rng = np.random.default_rng(M + 2 * N)
    lo, ext = rng.integers(-4, 3, (M, N, 2, 3)), rng.integers(-1, 4, (M, N, 2, 3))  # extent -1: empty
    win = np.asfortranarray(np.stack([lo[:, :, 0], lo[:, :, 0] + ext[:, :, 0], lo[:, :, 1], lo[:, :, 1] + ext[:, :, 1]],
                                     axis=2).astype(np.int32))
    assert win.shape == (M, N, 4, 3)
    assert_bit_equal(*both(A, B, win, 3, 1.7, 3, 2, True))
    assert_bit_equal(*both(A, B, W.constant_window(M, N, 7, 7), 3, 1.7, 3, 2, True))
    for levels in (1, 2, 3):
        assert_bit_equal(*both_pyramid(A, B, (7, 7, 3, 1.7), levels, 1, 1, 3, 2, True))


def test_every_window_of_every_rank_empty():
    A, B = R.crop_pair(R.CROPS[3])
    win = np.zeros((33, 17, 4, 3), dtype=np.int32, order="F")
    win[:, :, 0] = 1
    dev, host = both(A, B, win, 3, 1.7, 3, 2, True)
    assert_bit_equal(dev, host)
    assert np.all(bits(dev[0]) == NAN_BITS) and np.all(np.isposinf(dev[1])) and np.all(dev[2] == 0)


def test_only_rank_0_empty():
    """A missing rank excludes nothing: ranks 1 and 2 are what ranks 0 and 1 of the two boxes alone would be."""
    crop, par = R.CROPS[3], R.PARAMS[2]
    A, B = R.crop_pair(crop)
    win = np.array(K.windows(crop, par, "mixed", 3))
    win[:, :, :, 0] = np.array((1, 0, 1, 0))
    dev, host = both(A, B, win, par[2], par[3], 3, 2, True)
    assert_bit_equal(dev, host)
    assert np.all(bits(dev[0][..., 0]) == NAN_BITS) and np.all(np.isposinf(dev[1][..., 0]))
    two = both(A, B, np.asfortranarray(win[..., 1:]), par[2], par[3], 2, 2, True)[0]
    assert_bit_equal([a[..., 1:] for a in dev], two)
    assert not np.all(np.isnan(dev[0][..., 1:]))


@pytest.mark.parametrize("kind", W.KINDS)
def test_identities_1_and_2_on_the_device(kind):
    """H = 1, and rank 0 of any H and sep, are gqmap_block_match_window on box 0, device against device."""
    from gqmap_opticalflow_amd import block_match_window
    A, B = W.pair_97x130()
    for subpixel in (False, True):
        plain = block_match_window(A, B, windows_97x130(kind, 1)[..., 0], 3, 1.7, subpixel=subpixel)
        one = block_match_window(A, B, windows_97x130(kind, 1), 3, 1.7, subpixel=subpixel, hypotheses=1)
        assert_bit_equal(rank(one, 0), plain)
        for H, sep in HS:
            win = windows_97x130(kind, H)
            ranked = block_match_window(A, B, win, 3, 1.7, subpixel=subpixel, hypotheses=H, sep=sep)
            assert_bit_equal(rank(ranked, 0), block_match_window(A, B, win[..., 0], 3, 1.7, subpixel=subpixel))


@pytest.mark.parametrize("params,hs", [((7, 7, 3, 1.7), (3, 2)), ((12, 12, 3, 1.7), (4, 3)), ((32, 32, 4, 2.0), (4, 2)),
                                       ((5, 2, 0, 1.0), (2, 1)), ((0, 0, 3, 1.7), (2, 1)), ((3, 3, 2, 1.0), (3, 7))],
                         ids=str)
def test_identity_3_on_the_device(params, hs):
    """All boxes [-U, U] x [-V, V]: gqmap_block_match_multi and gqmap_block_match_refine
    at the same H and sep, device against device, missing ranks included (U = 0,
    and sep = 7 at U = 3).  (32, 32, 4, 2.0) at H = 4 is the largest chunk."""
    from gqmap_opticalflow_amd import block_match, block_match_pyramid, block_match_window
    A, B = R.crop_pair(R.CROPS[0])
    U, V, ft, sigma = params
    H, sep = hs
    win = W.constant_window(*A.shape, U, V)
    multi = block_match(A, B, *params, hypotheses=H, sep=sep)
    fine = block_match(A, B, *params, hypotheses=H, sep=sep, subpixel=True)
    assert_bit_equal(block_match_window(A, B, win, ft, sigma, hypotheses=H, sep=sep), multi)
    assert_bit_equal(block_match_window(A, B, win, ft, sigma, subpixel=True, hypotheses=H, sep=sep), fine)
    assert_bit_equal(block_match_pyramid(A, B, *params, levels=1, subpixel=True, hypotheses=H, sep=sep), fine)


def test_identity_3_on_nan_frames_on_the_device():
    from gqmap_opticalflow_amd import block_match, block_match_window
    A = np.full((6, 5), np.nan, order="F")
    for H, sep in HS:
        got = block_match_window(A, A, W.constant_window(6, 5, 2, 1), 1, 1.0, subpixel=True, hypotheses=H, sep=sep)
        assert_bit_equal(got, block_match(A, A, 2, 1, 1, 1.0, hypotheses=H, sep=sep, subpixel=True))


@pytest.mark.parametrize("subpixel", [False, True], ids=["integer", "subpixel"])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("levels,r,k", [(1, 1, 1), (2, 1, 1), (2, 0, 0), (3, 1, 1), (3, 2, 2)])
def test_pyramid_equals_host_model(levels, r, k, H, subpixel):
    """97 x 130 (49 x 65, 25 x 33 above it) and 5 x 7 (3 x 4, 2 x 2); rank 0 is the plain pyramid on the device."""
    from gqmap_opticalflow_amd import block_match_pyramid
    A, B = W.pair_97x130()
    dev, host = both_pyramid(A, B, (7, 7, 3, 1.7), levels, r, k, H, 2, subpixel)
    assert_bit_equal(dev, host)
    assert_bit_equal(rank(dev, 0), block_match_pyramid(A, B, 7, 7, 3, 1.7, levels=levels, r=r, k=k, subpixel=subpixel))
    assert_bit_equal(*both_pyramid(*R.crop_pair(R.CROPS[4]), (3, 3, 2, 1.0), levels, r, k, H, 2, subpixel))


def test_a_search_beyond_32():
    """U = V = 40 over two levels (20 at the coarsest): out of the plain matcher's reach."""
    A, B = W.pair_97x130()
    assert_bit_equal(*both_pyramid(A, B, (40, 40, 3, 1.7), 2, 1, 1, 3, 2, True))


def test_cost_and_curv_may_be_null_and_elapsed_ms():
    from gqmap_opticalflow_amd import _lib, block_match_pyramid, block_match_window
    lib = _lib.load()
    crop, par = R.CROPS[4], R.PARAMS[2]
    A, B = R.crop_pair(crop)
    win = K.windows(crop, par, "mixed", 3)
    flow = np.zeros((5, 7, 2, 3), order="F")
    assert lib.gqmap_block_match_window_multi(_lib.dptr(A), _lib.dptr(B), win.ctypes.data_as(C.POINTER(C.c_int)), 5, 7,
                                              par[2], par[3], 3, 2, 1, _lib.dptr(flow), None, None, None, 0) == 0
    want = block_match_window(A, B, win, par[2], par[3], subpixel=True, host=True, hypotheses=3)[0]
    assert np.array_equal(bits(flow), bits(want))
    assert lib.gqmap_block_match_pyramid_multi(_lib.dptr(A), _lib.dptr(B), 5, 7, 3, 3, par[2], par[3], 2, 1, 1, 3, 2, 1,
                                               _lib.dptr(flow), None, None, None, 0) == 0
    want = block_match_pyramid(A, B, *par, levels=2, subpixel=True, host=True, hypotheses=3)[0]
    assert np.array_equal(bits(flow), bits(want))
    for out in (block_match_window(A, B, win, par[2], par[3], timed=True, hypotheses=3),
                block_match_pyramid(A, B, *par, levels=3, subpixel=True, timed=True, hypotheses=3)):
        assert np.isfinite(out[-1]) and out[-1] > 0


def test_block_match_init_on_the_ranked_pyramid():
    from gqmap_opticalflow_amd import block_match_init
    I1, I2 = W.pair_97x130()
    I1, I2 = np.asfortranarray(I1[:96, :128]), np.asfortranarray(I2[:96, :128])
    kw = dict(pyr_ranked=True, hypotheses=3, levels=2, subpixel=True, sigma_from_cost=True, consistency=True, fill=True)
    dev, host = block_match_init(I1, I2, **kw), block_match_init(I1, I2, host=True, **kw)
    assert dev[1] == host[1] == dict(minu=-9.0, maxu=9.0, minv=-9.0, maxv=9.0)
    assert dev[0].shape == dev[2].shape == (96, 128, 2, 3) and dev[3].shape == (96, 128, 3) and len(dev) == len(host) == 4
    for d, h in zip((dev[0], dev[2], dev[3]), (host[0], host[2], host[3])):
        assert np.array_equal(d, h, equal_nan=True)
    assert not np.all(np.isnan(dev[0][..., 1:]))
    kw = dict(engine="super", **kw)
    dev, host = block_match_init(I1, I2, **kw), block_match_init(I1, I2, host=True, **kw)
    assert dev[0].shape == dev[2].shape == (24, 32, 2, 3) and len(dev) == len(host) == 4
    for d, h in zip((dev[0], dev[2], dev[3]), (host[0], host[2], host[3])):
        assert np.array_equal(d, h, equal_nan=True)
