"""gqmap_block_match (HIP kernel) against gqmap_block_match_host: the two
compile one header (csrc/gqmap_blockmatch.h), so flow and cost agree BIT FOR
BIT, ties included.  The host model itself is checked against the numpy
restatement in tests/test_block_match.py."""
import ctypes as C

import numpy as np
import pytest

from tests import _blockmatch_np as R
from tests._blockmatch_gpu import assert_bit_equal, bits, both, force_cols

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("params", R.PARAMS, ids=str)
@pytest.mark.parametrize("crop", R.CROPS, ids=str)
def test_kernel_equals_host_model(crop, params):
    A, B = R.crop_pair(crop)
    assert_bit_equal(*both(A, B, params))


def test_largest_lds_window():
    A, B = R.crop_pair(R.CROPS[0])
    assert_bit_equal(*both(A, B, (32, 32, 4, 2.0)))


@pytest.mark.parametrize("cols", [0, 8, 16, 32])
def test_several_tiles_with_partial_tiles_at_every_tile_width(cols):
    """97 x 130: four tile rows and 17 / 9 / 5 tile columns, the last of each
    partial.  cols = 0 is the library's own choice; 8, 16, 32 force each
    kernel instantiation (the choice follows the grid size and never changes a
    result), the widest one also at the largest window."""
    I1, I2, _ = R.rubberwhale()
    A, B = (np.asfortranarray(a[60:157, 210:340]) for a in (I1, I2))
    try:
        force_cols(cols)
        assert_bit_equal(*both(A, B, (7, 7, 3, 1.7)))
        if cols == 32:
            assert_bit_equal(*both(*R.crop_pair(R.CROPS[0]), (32, 32, 4, 2.0)))
    finally:
        force_cols(0)


@pytest.mark.parametrize("cols", [8, 16, 32])
def test_the_modes_agree_with_each_other_on_the_device(cols):
    """The three modes are one kernel template, so what a change to it could
    break silently is their agreement.  33 x 17: two tile rows, the second with
    one live row, and a partial tile column at every width.  The host model
    satisfies the same identities (tests/test_block_match_refine.py)."""
    from gqmap_opticalflow_amd import block_match
    A, B = R.crop_pair(R.CROPS[3])
    par = (7, 7, 3, 1.7)
    try:
        force_cols(cols)
        single = block_match(A, B, *par)
        one = block_match(A, B, *par, hypotheses=1)
        mflow, mcost = block_match(A, B, *par, hypotheses=3, sep=2)
        _, rcost, _ = block_match(A, B, *par, hypotheses=3, sep=2, subpixel=True)
        assert_bit_equal(single, (one[0][..., 0], one[1][..., 0]))
        assert_bit_equal(single, (mflow[..., 0], mcost[..., 0]))
        assert np.array_equal(bits(rcost), bits(mcost))
        assert_bit_equal(*both(A, B, par, hypotheses=1, subpixel=True))
    finally:
        force_cols(0)


@pytest.mark.parametrize("shape", [(1, 1), (64, 1), (1, 64)], ids=str)
def test_degenerate_images(shape):
    I1, I2, _ = R.rubberwhale()
    M, N = shape
    A, B = (np.asfortranarray(a[120:120 + M, 250:250 + N]) for a in (I1, I2))
    assert_bit_equal(*both(A, B, (7, 7, 3, 1.7)))


def test_elapsed_ms_and_closed_forms():
    from gqmap_opticalflow_amd import block_match
    A, B = R.crop_pair(R.CROPS[0])
    flow, cost, ms = block_match(A, B, timed=True)
    assert np.isfinite(ms) and ms > 0
    assert_bit_equal((flow, cost), block_match(A, B, host=True))
    z = np.zeros((16, 16))
    flow, cost = block_match(z, z, 2, 3, 1, 1.0)
    assert np.all(flow[:, :, 0] == 3) and np.all(flow[:, :, 1] == 2) and np.all(cost == 0)
    flow, _ = block_match(A, B, 0, 0, 3, 1.7)
    assert np.all(flow == 0)


@pytest.mark.parametrize("kw", [dict(U=33), dict(ft=5), dict(sigma=0.0), dict(sigma=float("nan")), dict(M=0)], ids=str)
def test_argument_errors_launch_nothing(kw):
    from gqmap_opticalflow_amd import _lib
    lib = _lib.load()
    a = dict(M=4, N=4, U=1, V=1, ft=1, sigma=1.0)
    a.update(kw)
    A = np.zeros((4, 4), order="F")
    flow = np.full((4, 4, 2), 77.0, order="F")
    cost = np.full((4, 4), 77.0, order="F")
    ms = C.c_double(-1.0)
    s = lib.gqmap_block_match(_lib.dptr(A), _lib.dptr(A), a["M"], a["N"], a["U"], a["V"], a["ft"],
                              C.c_double(a["sigma"]), _lib.dptr(flow), _lib.dptr(cost),
                              C.cast(C.byref(ms), _lib._D), 0)
    assert s == 1  # GQMAP_ERR_INVALID_ARG
    assert b"gqmap_block_match" in lib.gqmap_last_error()
    assert np.all(flow == 77.0) and np.all(cost == 77.0) and ms.value == -1.0  # nothing ran, nothing written
