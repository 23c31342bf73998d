"""Block-matching initialiser, host model (gqmap_block_match_host) against the
literal numpy restatement of legacy/optical_flow_temp.m:13-32
(tests/_blockmatch_np.py).  No device.

Tolerances.  Costs are at most 255 and the filter weights sum to 1; 49 fp64
terms give an error near 50 * 2^-53 * 255 = 1.4e-12, so 1e-10 leaves two orders
of margin for the separable form and the rounding of the weights.  The argmin
is compared exactly wherever the restatement's two smallest costs differ by
more than 1e-9 (ten times the cost tolerance)."""
import numpy as np
import pytest

from tests import _blockmatch_np as R

COST_TOL = 1e-10
GAP_TOL = 1e-9
# parameter set -> crops on which the restatement has no pair of best costs closer than GAP_TOL
INDEX_CASES = {
    (7, 7, 3, 1.7): R.CROPS,
    (12, 12, 3, 1.7): R.CROPS,
    (3, 3, 2, 1.0): tuple(c for c in R.CROPS if c[:2] != (0, 0)),  # (0,0,..) has one exact tie
}


def model(A, B, params):
    from gqmap_opticalflow_amd import block_match
    return block_match(A, B, *params, host=True)


def chosen_cost(vol, flow, U, V):
    """The restatement's cost at the displacement a flow names."""
    u0, v0 = U - flow[:, :, 1].astype(int), V - flow[:, :, 0].astype(int)
    return np.take_along_axis(vol, (u0 + v0 * (2 * U + 1))[:, :, None], axis=2)[:, :, 0]


@pytest.mark.parametrize("params", R.PARAMS, ids=str)
@pytest.mark.parametrize("crop", R.CROPS, ids=str)
def test_host_model_cost_matches_restatement(crop, params):
    U, V = params[:2]
    flow, cost = model(*R.crop_pair(crop), params)
    _, rcost, vol, _ = R.reference(crop, params)
    assert np.all(flow == np.round(flow))
    assert np.all(np.abs(flow[:, :, 0]) <= V) and np.all(np.abs(flow[:, :, 1]) <= U)
    assert np.max(np.abs(cost - rcost)) <= COST_TOL
    assert np.max(np.abs(chosen_cost(vol, flow, U, V) - rcost)) <= COST_TOL


@pytest.mark.parametrize("params,crop", [(p, c) for p, cs in INDEX_CASES.items() for c in cs], ids=str)
def test_host_model_index_matches_restatement(params, crop):
    flow, _ = model(*R.crop_pair(crop), params)
    rflow, _, _, gap = R.reference(crop, params)
    assert not np.any(gap <= GAP_TOL), f"{int(np.sum(gap <= GAP_TOL))} near-ties, smallest gap {gap.min():.3g}"
    assert np.array_equal(flow, rflow)


@pytest.mark.parametrize("crop", R.CROPS, ids=str)
def test_ft0_is_exact_with_ties_to_the_first_index(crop):
    params = (5, 2, 0, 1.0)
    flow, cost = model(*R.crop_pair(crop), params)
    rflow, rcost, _, _ = R.reference(crop, params)
    assert np.array_equal(cost, rcost)
    assert np.array_equal(flow, rflow)


def test_closed_form_ties_and_padding():
    from gqmap_opticalflow_amd import block_match
    z = np.zeros((16, 16))
    flow, cost = block_match(z, z, 2, 3, 1, 1.0, host=True)
    assert np.all(flow[:, :, 0] == 3) and np.all(flow[:, :, 1] == 2) and np.all(cost == 0)
    c = np.full((24, 24), 100.0)
    U = V = 2
    ft = 1
    flow, cost = block_match(c, c, U, V, ft, 1.0, host=True)
    b = U + ft
    assert np.all(flow[b:-b, b:-b, 0] == V) and np.all(flow[b:-b, b:-b, 1] == U)
    assert np.all(cost[b:-b, b:-b] == 0)
    A, B = R.crop_pair(R.CROPS[3])
    flow, cost = block_match(A, B, 0, 0, 3, 1.7, host=True)
    assert np.all(flow == 0)
    assert np.max(np.abs(cost - R.block_match(A, B, 0, 0, 3, 1.7)[1])) <= COST_TOL


@pytest.mark.parametrize("kw", [dict(U=33), dict(V=33), dict(U=-1), dict(ft=5), dict(sigma=0.0),
                                dict(sigma=float("nan")), dict(sigma=float("inf")), dict(M=0)], ids=str)
def test_argument_errors(kw):
    import ctypes as C

    from gqmap_opticalflow_amd import _lib
    lib = _lib.load()
    a = dict(M=4, N=4, U=1, V=1, ft=1, sigma=1.0)
    a.update(kw)
    A = np.zeros((4, 4), order="F")
    flow = np.zeros((4, 4, 2), order="F")
    s = lib.gqmap_block_match_host(_lib.dptr(A), _lib.dptr(A), a["M"], a["N"], a["U"], a["V"], a["ft"],
                                   C.c_double(a["sigma"]), _lib.dptr(flow), None)
    assert s == 1  # GQMAP_ERR_INVALID_ARG
    assert lib.gqmap_last_error()


def test_whole_frame_beats_zero_flow_without_ground_truth():
    """388 x 584 at the reference defaults, oriented by block_match_init: the
    AEPE against the GT (unknown pixels excluded) is below 0.6 x the zero-flow
    AEPE (restatement: 0.500 against 1.256, ratio 0.40)."""
    from gqmap_opticalflow_amd import block_match_init
    I1, I2, gt = R.rubberwhale()
    flow, rng = block_match_init(I1, I2, host=True)
    assert rng == dict(minu=-7.0, maxu=7.0, minv=-7.0, maxv=7.0)
    assert flow.shape == gt.shape and np.all(flow == np.round(flow))
    assert np.all(np.abs(flow[:, :, 0]) <= 7) and np.all(np.abs(flow[:, :, 1]) <= 7)
    known = np.all(np.abs(gt) <= 1e9, axis=2)
    epe = np.sqrt(np.sum((gt - flow) ** 2, axis=2))[known].mean()
    zero = np.sqrt(np.sum(gt ** 2, axis=2))[known].mean()
    print(f"block-matching AEPE {epe:.4f}, zero-flow AEPE {zero:.4f}, ratio {epe / zero:.3f}")
    assert epe < 0.6 * zero
