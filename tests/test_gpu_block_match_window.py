"""gqmap_block_match_window and gqmap_block_match_pyramid (HIP kernels) against
their host models: one header (csrc/gqmap_blockmatch.h) behind both, so flow,
cost and curvature agree BIT FOR BIT, NaN patterns included, whatever the tile
width and the chunk extent; the host models are checked against numpy in
tests/test_block_match_window.py."""
import ctypes as C

import numpy as np
import pytest

from tests import _blockmatch_np as R
from tests import _blockmatch_window_np as W
from tests._blockmatch_gpu import NAN_BITS, assert_bit_equal, bits, force_cols

pytestmark = pytest.mark.gpu


def force_chunk(cu, cv):
    from gqmap_opticalflow_amd import _lib
    f = _lib.load().gqmap_debug_block_match_chunk
    f.restype, f.argtypes = C.c_int, [C.c_int, C.c_int]
    assert f(cu, cv) == 0


def both(A, B, win, ft, sigma, subpixel):
    from gqmap_opticalflow_amd import block_match_window
    return (block_match_window(A, B, win, ft, sigma, subpixel=subpixel),
            block_match_window(A, B, win, ft, sigma, subpixel=subpixel, host=True))


def both_pyramid(A, B, params, levels, r, k, subpixel):
    from gqmap_opticalflow_amd import block_match_pyramid
    return (block_match_pyramid(A, B, *params, levels=levels, r=r, k=k, subpixel=subpixel),
            block_match_pyramid(A, B, *params, levels=levels, r=r, k=k, subpixel=subpixel, host=True))


def windows_97x130(kind):
    return W.make_windows(97, 130, 7, 7, kind, seed=3)


@pytest.mark.parametrize("subpixel", [False, True], ids=["integer", "subpixel"])
@pytest.mark.parametrize("kind", W.KINDS)
@pytest.mark.parametrize("params", R.PARAMS[:3], ids=str)
@pytest.mark.parametrize("crop", R.CROPS, ids=str)
def test_kernel_equals_host_model(crop, params, kind, subpixel):
    assert_bit_equal(*both(*R.crop_pair(crop), W.windows(crop, params, kind), params[2], params[3], subpixel))


@pytest.mark.parametrize("kind", W.KINDS)
@pytest.mark.parametrize("cols", [0, 8, 16, 32])
def test_several_tiles_with_partial_tiles_at_every_tile_width(cols, kind):
    """97 x 130: four tile rows, the last tile of each row and column partial;
    8, 16, 32 force each instantiation.  halves: the two boxes 40 apart meet
    inside one tile (column 65), whose union box holds a gap that no pixel wants."""
    A, B = W.pair_97x130()
    try:
        force_cols(cols)
        for subpixel in (False, True):
            assert_bit_equal(*both(A, B, windows_97x130(kind), 3, 1.7, subpixel))
    finally:
        force_cols(0)


@pytest.mark.parametrize("kind", W.KINDS)
@pytest.mark.parametrize("chunk", [(5, 5), (1, 1), (3, 65)], ids=str)
def test_a_window_over_several_chunks(chunk, kind):
    """The chunk extent forced: at 5 x 5 a window spans several chunks on both
    axes, so the pick crosses chunk borders, ties (the window off the frame)
    resolve across them, and the neighbours of a pick lie in other chunks."""
    A, B = W.pair_97x130()
    win = windows_97x130(kind)
    try:
        force_chunk(*chunk)
        for subpixel in (False, True):
            assert_bit_equal(*both(A, B, win, 3, 1.7, subpixel))
        if chunk == (5, 5):
            force_cols(8)
            assert_bit_equal(*both(A, B, win, 3, 1.7, True))
    finally:
        force_chunk(0, 0)
        force_cols(0)


@pytest.mark.parametrize("shape", [(1, 1), (64, 1), (1, 64)], ids=str)
def test_degenerate_images(shape):
    I1, I2, _ = R.rubberwhale()
    M, N = shape
    A, B = (np.asfortranarray(a[120:120 + M, 250:250 + N]) for a in (I1, I2))
    rng = np.random.default_rng(M + 2 * N)
    lo, ext = rng.integers(-4, 3, (M, N, 2)), rng.integers(-1, 4, (M, N, 2))  # extent -1: empty
    win = np.asfortranarray(np.stack([lo[..., 0], lo[..., 0] + ext[..., 0], lo[..., 1], lo[..., 1] + ext[..., 1]],
                                     axis=2).astype(np.int32))
    assert_bit_equal(*both(A, B, win, 3, 1.7, True))
    assert_bit_equal(*both(A, B, W.constant_window(M, N, 7, 7), 3, 1.7, True))
    for levels in (1, 2, 3):
        assert_bit_equal(*both_pyramid(A, B, (7, 7, 3, 1.7), levels, 1, 1, True))


def test_every_window_empty():
    A, B = R.crop_pair(R.CROPS[3])
    win = np.zeros((33, 17, 4), dtype=np.int32, order="F")
    win[:, :, 0] = 1
    dev, host = both(A, B, win, 3, 1.7, True)
    assert_bit_equal(dev, host)
    assert np.all(bits(dev[0]) == NAN_BITS) and np.all(np.isposinf(dev[1])) and np.all(dev[2] == 0)


def test_cost_and_curv_may_be_null_and_elapsed_ms():
    from gqmap_opticalflow_amd import _lib, block_match_pyramid, block_match_window
    lib = _lib.load()
    crop, par = R.CROPS[4], R.PARAMS[2]
    A, B = R.crop_pair(crop)
    win = W.windows(crop, par, "mixed")
    flow = np.zeros((5, 7, 2), order="F")
    assert lib.gqmap_block_match_window(_lib.dptr(A), _lib.dptr(B), win.ctypes.data_as(C.POINTER(C.c_int)), 5, 7, par[2],
                                        par[3], 1, _lib.dptr(flow), None, None, None, 0) == 0
    assert np.array_equal(bits(flow), bits(block_match_window(A, B, win, par[2], par[3], subpixel=True, host=True)[0]))
    assert lib.gqmap_block_match_pyramid(_lib.dptr(A), _lib.dptr(B), 5, 7, 3, 3, par[2], par[3], 2, 1, 1, 1,
                                         _lib.dptr(flow), None, None, None, 0) == 0
    assert np.array_equal(bits(flow), bits(block_match_pyramid(A, B, *par, levels=2, subpixel=True, host=True)[0]))
    for out in (block_match_window(A, B, win, par[2], par[3], timed=True),
                block_match_pyramid(A, B, *par, levels=3, subpixel=True, timed=True)):
        assert np.isfinite(out[-1]) and out[-1] > 0


@pytest.mark.parametrize("params", [(7, 7, 3, 1.7), (12, 12, 3, 1.7), (32, 32, 4, 2.0), (5, 2, 0, 1.0), (0, 0, 3, 1.7)],
                         ids=str)
def test_a_constant_box_is_the_plain_matcher_on_the_device(params):
    """The anchor, device against device: gqmap_block_match and
    gqmap_block_match_refine at H = 1.  (32, 32, 4, 2.0) is the largest chunk."""
    from gqmap_opticalflow_amd import block_match, block_match_window
    A, B = R.crop_pair(R.CROPS[0])
    U, V, ft, sigma = params
    win = W.constant_window(*A.shape, U, V)
    assert_bit_equal(block_match_window(A, B, win, ft, sigma), block_match(A, B, *params))
    fine = block_match(A, B, *params, subpixel=True)
    assert_bit_equal(block_match_window(A, B, win, ft, sigma, subpixel=True), [a[..., 0] for a in fine])


@pytest.mark.parametrize("subpixel", [False, True], ids=["integer", "subpixel"])
@pytest.mark.parametrize("levels,r,k", [(1, 1, 1), (2, 1, 1), (2, 0, 0), (3, 1, 1), (3, 2, 2)])
def test_pyramid_equals_host_model(levels, r, k, subpixel):
    """97 x 130 (49 x 65, 25 x 33 above it) and 5 x 7 (3 x 4, 2 x 2)."""
    assert_bit_equal(*both_pyramid(*W.pair_97x130(), (7, 7, 3, 1.7), levels, r, k, subpixel))
    assert_bit_equal(*both_pyramid(*R.crop_pair(R.CROPS[4]), (3, 3, 2, 1.0), levels, r, k, subpixel))


def test_one_level_is_the_plain_matcher_on_the_device():
    from gqmap_opticalflow_amd import block_match, block_match_pyramid
    A, B = W.pair_97x130()
    par = (7, 7, 3, 1.7)
    assert_bit_equal(block_match_pyramid(A, B, *par, levels=1), block_match(A, B, *par))
    assert_bit_equal(block_match_pyramid(A, B, *par, levels=1, subpixel=True),
                     [a[..., 0] for a in block_match(A, B, *par, subpixel=True)])


def test_a_search_beyond_32():
    """U = V = 40 over two levels (20 at the coarsest): out of the plain matcher's reach."""
    A, B = W.pair_97x130()
    assert_bit_equal(*both_pyramid(A, B, (40, 40, 3, 1.7), 2, 1, 1, True))


def test_block_match_init_on_the_pyramid():
    from gqmap_opticalflow_amd import block_match_init
    I1, I2 = W.pair_97x130()
    I1, I2 = np.asfortranarray(I1[:96, :128]), np.asfortranarray(I2[:96, :128])
    kw = dict(levels=2, subpixel=True, sigma_from_cost=True)
    dev, host = block_match_init(I1, I2, **kw), block_match_init(I1, I2, host=True, **kw)
    assert dev[1] == host[1] == dict(minu=-9.0, maxu=9.0, minv=-9.0, maxv=9.0)
    assert dev[0].shape == dev[2].shape == (96, 128, 2)
    assert np.array_equal(bits(dev[0]), bits(host[0])) and np.array_equal(bits(dev[2]), bits(host[2]))
    kw = dict(engine="super", consistency=True, fill=True, **kw)
    dev, host = block_match_init(I1, I2, **kw), block_match_init(I1, I2, host=True, **kw)
    assert dev[0].shape == (24, 32, 2) and len(dev) == len(host) == 4
    for d, h in zip((dev[0], dev[2], dev[3]), (host[0], host[2], host[3])):
        assert np.array_equal(d, h, equal_nan=True)
