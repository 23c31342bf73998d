"""gqmap_flow_wmedian (HIP kernel) against its host model: one header
(csrc/gqmap_wmedian.h) behind both, so the filtered flows agree BIT FOR BIT, NaN
patterns included; the host model itself is checked against numpy in
tests/test_flow_wmedian.py.  Then block_match_flow(median=) on the device
against host=True."""
import numpy as np
import pytest

from tests import _wmedian_np as W
from tests._wmedian_np import bits

pytestmark = pytest.mark.gpu


def both(flow, guide, r=2, sigma_s=2.0, sigma_c=10.0, passes=1, conf=None):
    from gqmap_opticalflow_amd import flow_wmedian
    dev = flow_wmedian(flow, guide, r, sigma_s, sigma_c, passes, conf)
    host = flow_wmedian(flow, guide, r, sigma_s, sigma_c, passes, conf, host=True)
    diff = bits(dev) != bits(host)
    assert not diff.any(), f"{int(diff.sum())} of {diff.size} entries differ (r={r} passes={passes} conf={conf is not None})"
    return host


@pytest.fixture(scope="module")
def big():
    """The 97 x 130 crop of tests/test_gpu_flow_check.py: with 16 x 16 tiles seven tile rows and nine tile
    columns, the last of each partial.  Its sub-pixel flow, I1 as guide."""
    from tests.test_gpu_flow_check import crop_fields
    A, B, fwd, _ = crop_fields()
    return A, B, fwd


@pytest.mark.parametrize("shape", [(1, 1), (64, 1), (1, 64)], ids=str)
def test_degenerate_fields(shape):
    M, N = shape
    for r in (0, 1, 2, 5, 8):
        both(W.noisy(M, N, 1), W.guide_of(M, N, 4), r, 0.5 * r + 1.0, 10.0, 2)
        both(W.special(M, N, 3), W.guide_of(M, N, 4, True), r, 0.5 * r + 1.0, 10.0, 2, W.conf_of(M, N, 5, True))


@pytest.mark.parametrize("r", [0, 1, 2, 3, 4, 5, 6, 7, 8])
def test_partial_tiles_in_both_directions(r):
    """37 x 70: three tile rows and five tile columns, the last of each partial.  Every radius: a lane per pixel
    up to r = 2, above it a wave per pixel with one to five entries per lane."""
    M, N = 37, 70
    for flow, nans in ((W.noisy(M, N, 1), False), (W.special(M, N, 3), True)):
        for conf in (None, W.conf_of(M, N, 5, nans)):
            out = both(flow, W.guide_of(M, N, 4, nans), r, 0.5 * r + 1.0, 10.0, 1, conf)
            assert (r == 0) == np.array_equal(bits(out), bits(flow))


@pytest.mark.parametrize("r", [0, 1, 2, 5, 8])
def test_the_crop(big, r):
    A, _, fwd = big
    M, N = A.shape
    conf = W.conf_of(M, N, 5, True)
    for flow in (fwd, W.special(M, N, 3)):
        for passes in (1, 3):
            for c in (None, conf):
                both(flow, A, r, 0.5 * r + 1.0, 10.0, passes, c)


def test_an_outlier_block_and_a_hole_across_a_tile_corner():
    """Tiles are 16 x 16: the block and the hole each cover a corner shared by four of them."""
    M, N = 48, 48
    clean = np.asfortranarray(np.broadcast_to(np.array([1.5, -0.5]), (M, N, 2)))
    f = clean.copy(order="F")
    f[14:18, 14:18] = np.random.default_rng(10).uniform(5, 9, (4, 4, 2))
    f[29:36, 28:35] = np.nan
    guide = np.full((M, N), 100.0)
    out = both(f, guide)
    assert (out[:24, :24] != clean[:24, :24]).any(axis=2).sum() == 12 and np.isnan(out[:, :, 0]).sum() == 9
    conf = np.ones((M, N))
    conf[14:18, 14:18] = 0.0
    assert np.array_equal(both(f, guide, passes=2, conf=conf), clean)
    both(f, guide, 8, 4.0, 10.0, 2, conf)


def test_elapsed_ms():
    from gqmap_opticalflow_amd import flow_wmedian
    f, g = W.special(37, 70, 3), W.guide_of(37, 70, 4)
    out, ms = flow_wmedian(f, g, passes=2, timed=True)
    assert np.isfinite(ms) and ms > 0
    assert np.array_equal(bits(out), bits(flow_wmedian(f, g, passes=2, host=True)))


def test_block_match_flow_median_on_the_device_equals_host(big):
    from gqmap_opticalflow_amd import block_match_flow
    A, B, _ = big
    kw = dict(denoise=dict(its=5), median=dict(r=2, passes=2, conf="sigma"))
    dev, host = block_match_flow(A, B, **kw), block_match_flow(A, B, host=True, **kw)
    for x, y, what in zip(dev, host, ("flow", "sigma", "consistent")):
        assert np.array_equal(bits(x.astype(np.float64)), bits(y.astype(np.float64))), what
    assert not np.array_equal(bits(dev[0]), bits(block_match_flow(A, B, host=True, denoise=dict(its=5))[0]))
