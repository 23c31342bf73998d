"""gqmap_flow_consistency and gqmap_flow_fill (HIP kernels) against their host
models: one header (csrc/gqmap_flowcheck.h) behind both, so err, mask, the
filled flow and the fill states agree BIT FOR BIT, NaN patterns included; the
host models themselves are checked against numpy in tests/test_flow_check.py.
Then block_match_init(consistency=True, fill=True) on the device against
host=True, and one short solve seeded with its output."""
import numpy as np
import pytest

from tests import _blockmatch_np as R
from tests import _flowcheck_np as F
from tests._blockmatch_gpu import problem
from tests._flowcheck_np import bits

pytestmark = pytest.mark.gpu


def check_both(fwd, bwd, a1=0.01, a2=0.5):
    from gqmap_opticalflow_amd import flow_consistency
    dev, host = flow_consistency(fwd, bwd, a1, a2), flow_consistency(fwd, bwd, a1, a2, host=True)
    assert np.array_equal(bits(dev[0]), bits(host[0])), f"err: {int((bits(dev[0]) != bits(host[0])).sum())} differ"
    assert np.array_equal(dev[1], host[1])
    return host


def fill_both(flow, mask, r=8, sigma=4.0, passes=2):
    from gqmap_opticalflow_amd import flow_fill
    dev, host = flow_fill(flow, mask, r, sigma, passes), flow_fill(flow, mask, r, sigma, passes, host=True)
    diff = bits(dev[0]) != bits(host[0])
    assert not diff.any(), f"flow: {int(diff.sum())} of {diff.size} entries differ (r={r} passes={passes})"
    assert np.array_equal(dev[1], host[1]), (r, passes)
    return host


def crop_fields(subpixel=True):
    """The 97 x 130 crop: with the fill's 32 x 32 tiles four tile rows and five tile
    columns, the last of each partial."""
    from gqmap_opticalflow_amd import block_match_init
    I1, I2, _ = R.rubberwhale()
    A, B = (np.asfortranarray(a[60:157, 210:340]) for a in (I1, I2))
    return (A, B, block_match_init(A, B, host=True, subpixel=subpixel)[0],
            block_match_init(B, A, host=True, subpixel=subpixel)[0])


@pytest.fixture(scope="module")
def big():
    return crop_fields()


def noisy(M, N, seed=0):
    return np.asfortranarray(np.random.default_rng(seed).uniform(-4, 4, (M, N, 2)))


def hole(M=64, N=64, lo=12, hi=52):
    mask = np.ones((M, N), dtype=bool)
    mask[lo:hi, lo:hi] = False
    return mask


@pytest.mark.parametrize("params", F.PARAMS, ids=str)
@pytest.mark.parametrize("crop", R.CROPS, ids=str)
def test_kernels_equal_host_models(crop, params):
    fwd, bwd = F.fields(crop, params)
    mask = check_both(fwd, bwd)[1]
    check_both(fwd, bwd, 0.0, 0.05)
    for r, passes in ((0, 1), (1, 3), (8, 1), (8, 3), (16, 1), (16, 3)):
        fill_both(fwd, mask, r, 0.5 * r + 0.5, passes)


def test_several_tiles_with_partial_tiles(big):
    _, _, fwd, bwd = big
    err, mask = check_both(fwd, bwd)
    assert 0 < (~mask).sum() < mask.size
    for r in (0, 1, 8, 16):
        out, filled = fill_both(fwd, mask, r, 4.0, 2)
        assert (r == 0) == (not (filled == 1).any())


@pytest.mark.parametrize("shape", [(1, 1), (64, 1), (1, 64)], ids=str)
def test_degenerate_fields(shape):
    M, N = shape
    fwd, bwd = noisy(M, N, 1) / 8, noisy(M, N, 2) / 8
    mask = check_both(fwd, bwd)[1]
    check_both(np.zeros((M, N, 2)), np.zeros((M, N, 2)))
    for r in (0, 1, 16):
        fill_both(fwd, mask, r, 2.0, 2)
        fill_both(fwd, np.arange(M * N).reshape(M, N) % 3 == 0, r, 2.0, 2)


def test_nan_flows_and_targets_on_the_frame_edge():
    M, N = 37, 70
    m, n = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    fwd = np.asfortranarray(np.stack([(N - 1 - n).astype(np.float64), (M - 1 - m).astype(np.float64)], axis=2))
    bwd = noisy(M, N, 4)
    check_both(fwd, bwd, 0.0, 1e300)
    fwd[3, 5, 0], fwd[20, 66, 1], bwd[M - 1, N - 1, 1] = np.nan, np.inf, np.nan
    err, mask = check_both(fwd, bwd, 0.0, 1e300)
    assert not mask.any() and np.isposinf(err[3, 5]) and np.isposinf(err[20, 66]) and np.isnan(err[0, 0])


@pytest.mark.parametrize("r", [0, 1, 8, 16])
def test_fill_masks_of_every_kind(r):
    """All valid (every tile copies through), all invalid, a checkerboard, and
    NaN / Inf payloads at the invalid pixels; r = 16 is the largest LDS window."""
    M, N = 70, 45
    f = noisy(M, N)
    m, n = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    out, filled = fill_both(f, np.ones((M, N), dtype=bool), r)
    assert np.array_equal(bits(out), bits(f)) and not filled.any()
    out, filled = fill_both(f, np.zeros((M, N), dtype=bool), r)
    assert np.array_equal(bits(out), bits(f)) and np.all(filled == 255)
    board = (m + n) % 2 == 0
    out, filled = fill_both(f, board, r)
    assert np.all(filled[~board] == (255 if r == 0 else 1))
    dirty = f.copy(order="F")
    dirty[:, :, 0][~board], dirty[::3, :, 1] = np.nan, np.inf
    out2, _ = fill_both(dirty, board, r)
    if r:
        assert np.array_equal(bits(out2[:, :, 0]), bits(out[:, :, 0])) and np.all(np.isfinite(out2[:, :, 0]))


@pytest.mark.parametrize("passes", [1, 2, 3])
def test_the_wide_hole_pass_by_pass(passes):
    f, mask = noisy(64, 64), hole()
    f[mask == 0] = np.nan
    out, filled = fill_both(f, mask, 8, 4.0, passes)
    left = {1: 24 * 24, 2: 8 * 8, 3: 0}[passes]
    assert (filled == 255).sum() == left and filled.max() == (255 if left else 3)
    assert np.isnan(out[:, :, 0]).sum() == left


def test_a_hole_across_a_tile_corner():
    """Tiles are 32 x 32: the hole covers the corner shared by four of them, so each
    tile fills its part from a halo that reaches into the other three."""
    f = noisy(80, 80, 5)
    mask = np.ones((80, 80), dtype=bool)
    mask[25:40, 27:38] = False
    mask[60:70, 30:34] = False  # and one astride a single edge
    f[~mask] = np.nan
    for r, passes in ((4, 1), (8, 1), (16, 2)):
        out, filled = fill_both(f, mask, r, 3.0, passes)
        assert (filled == 1).any() and (r == 4) == (filled == 255).any()


def test_elapsed_ms():
    from gqmap_opticalflow_amd import flow_consistency, flow_fill
    fwd, bwd = F.fields(R.CROPS[0], F.PARAMS[0])
    err, mask, ms = flow_consistency(fwd, bwd, timed=True)
    assert np.isfinite(ms) and ms > 0
    out, filled, ms = flow_fill(fwd, mask, timed=True)
    assert np.isfinite(ms) and ms > 0
    assert np.array_equal(bits(out), bits(flow_fill(fwd, mask, host=True)[0]))


def test_outputs_may_be_null():
    from gqmap_opticalflow_amd import _lib, flow_consistency, flow_fill
    lib = _lib.load()
    fwd, bwd = F.fields(R.CROPS[3], F.PARAMS[0])
    M, N, _ = fwd.shape
    err, mask = flow_consistency(fwd, bwd, host=True)
    e, k = np.zeros((M, N), order="F"), np.zeros((M, N), dtype=np.uint8, order="F")
    assert lib.gqmap_flow_consistency(_lib.dptr(fwd), _lib.dptr(bwd), M, N, 0.01, 0.5, _lib.dptr(e), None, None, 0) == 0
    assert lib.gqmap_flow_consistency(_lib.dptr(fwd), _lib.dptr(bwd), M, N, 0.01, 0.5, None, _lib.u8ptr(k), None, 0) == 0
    assert np.array_equal(bits(e), bits(err)) and np.array_equal(k, mask.astype(np.uint8))
    o = np.zeros((M, N, 2), order="F")
    assert lib.gqmap_flow_fill(_lib.dptr(fwd), _lib.u8ptr(k), M, N, 8, 4.0, 2, _lib.dptr(o), None, None, 0) == 0
    assert np.array_equal(bits(o), bits(flow_fill(fwd, mask, host=True)[0]))


def test_block_match_init_on_the_device_equals_host(big):
    from gqmap_opticalflow_amd import block_match_init
    A, B, _, _ = big
    kw = dict(consistency=True, fill=True, hypotheses=3, subpixel=True, sigma_from_cost=True)
    flow, rng, sig, cons = block_match_init(A, B, **kw)
    hflow, hrng, hsig, hcons = block_match_init(A, B, host=True, **kw)
    assert rng == hrng and flow.shape == sig.shape == (97, 130, 2, 3) and cons.shape == (97, 130, 3)
    assert np.array_equal(bits(flow), bits(hflow)) and np.array_equal(bits(sig), bits(hsig)) and np.array_equal(cons, hcons)
    assert 0 < cons[:, :, 0].sum() < cons[:, :, 0].size and np.isnan(flow[:, :, :, 1:]).any()
    nflow, _, nsig, ncons = block_match_init(A[:96, :128], B[:96, :128], engine="super", **kw)
    hn = block_match_init(A[:96, :128], B[:96, :128], engine="super", host=True, **kw)
    assert nflow.shape == (24, 32, 2, 3) and ncons.shape == (96, 128, 3)
    assert np.array_equal(bits(nflow), bits(hn[0])) and np.array_equal(bits(nsig), bits(hn[2])) and np.array_equal(ncons, hn[3])


def test_short_solve_seeded_with_the_checked_and_filled_start():
    """24 x 20, L = 3, 20 iterations through the public solver: bit for bit the
    solve started from set_state(initial_state(flow=, sigma=))."""
    from gqmap_opticalflow_amd import block_match_init, gqmap_gpu_mixture, initial_state
    I1, I2, o, (M, N) = problem("mixture")
    flow, ranges, sig, cons = block_match_init(I1, I2, consistency=True, fill=True, hypotheses=3, subpixel=True,
                                               sigma_from_cost=True)
    assert flow.shape == sig.shape == (M, N, 2, 3) and cons.shape == (M, N, 3) and (~cons).any()
    assert np.all(np.isnan(sig[np.broadcast_to(~cons[:, :, None, :], sig.shape)]))
    o = {**o, "its": 20}
    a = gqmap_gpu_mixture(o, I1, I2, seed=1, init_flow=flow, init_sigma=sig)
    b = gqmap_gpu_mixture(o, I1, I2, seed=1, state=initial_state(o, M, N, seed=1, flow=flow, sigma=sig))
    assert a[0].shape == (M, N, 3, 2) and a[4].shape == (20,) and np.all(np.isfinite(a[4]))
    for x, y, what in zip(a, b, ("mu", "sigma", "alpha", "AEPE", "Energy", "logP")):
        np.testing.assert_array_equal(x, y, err_msg=what)
