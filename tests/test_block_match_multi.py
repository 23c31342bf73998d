"""Several hypotheses per pixel, host model (gqmap_block_match_multi_host)
against the numpy restatement of the greedy rule on the full cost volume
(tests/_blockmatch_multi_np.py), and the Python layers on top.  No device.

Tolerances as in tests/test_block_match.py: costs within 1e-10 (49 fp64 terms
of at most 255 err near 1.4e-12); picks compared exactly only where the
restatement's best and second-best ALLOWED costs differ by more than 1e-9 at
every rank, which the index test asserts first."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import _blockmatch_multi_np as G
from tests import _blockmatch_np as R

COST_TOL = 1e-10
GAP_TOL = 1e-9
SEPS = (1, 2, 3)
INDEX_PARAMS = ((7, 7, 3, 1.7), (12, 12, 3, 1.7))


@functools.lru_cache(maxsize=None)
def model(crop, params, H, sep):
    """The host model on one crop, computed once and shared (read-only)."""
    from gqmap_opticalflow_amd import block_match
    out = block_match(*R.crop_pair(crop), *params, host=True, hypotheses=H, sep=sep)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("sep", SEPS)
@pytest.mark.parametrize("params", R.PARAMS, ids=str)
@pytest.mark.parametrize("crop", R.CROPS, ids=str)
def test_rank0_keeps_the_bits_of_the_single_hypothesis_call(crop, params, sep):
    from gqmap_opticalflow_amd import block_match
    flow, cost = model(crop, params, 3, sep)
    flow1, cost1 = block_match(*R.crop_pair(crop), *params, host=True)
    assert flow.shape == flow1.shape + (3,) and cost.shape == cost1.shape + (3,)
    assert np.array_equal(flow[..., 0].view(np.uint64), flow1.view(np.uint64))
    assert np.array_equal(cost[..., 0].view(np.uint64), cost1.view(np.uint64))


@pytest.mark.parametrize("sep", SEPS)
@pytest.mark.parametrize("params", R.PARAMS, ids=str)
@pytest.mark.parametrize("crop", R.CROPS, ids=str)
def test_costs_match_restatement_given_the_models_own_picks(crop, params, sep):
    """Holds with or without ties: every existing rank's displacement is
    allowed given the model's own earlier picks, costs what the restatement's
    volume says there, and no more than the smallest allowed cost."""
    U, V = params[:2]
    flow, cost = model(crop, params, 3, sep)
    vol = R.reference(crop, params)[2]
    idx = G.flow_to_index(flow, U, V)
    for k in range(3):
        ok = G.allowed_after([idx[:, :, j] for j in range(k)], U, V, sep, vol.shape[:2])
        has = idx[:, :, k] >= 0
        assert np.array_equal(has, ok.any(axis=2)), f"rank {k}: exists where something is allowed, and only there"
        assert np.all(np.isinf(cost[:, :, k][~has])) and np.all(cost[:, :, k][~has] > 0)
        assert np.all(np.isnan(flow[:, :, :, k][~has]))
        pick = np.where(has, idx[:, :, k], 0)[:, :, None]
        assert np.all(np.take_along_axis(ok, pick, axis=2)[:, :, 0][has]), f"rank {k}: pick not allowed"
        at_pick = np.take_along_axis(vol, pick, axis=2)[:, :, 0]
        least = np.where(ok, vol, np.inf).min(axis=2)
        assert np.max(np.abs(cost[:, :, k] - at_pick)[has], initial=0.0) <= COST_TOL
        assert np.max((cost[:, :, k] - least)[has], initial=-np.inf) <= COST_TOL


@pytest.mark.parametrize("sep", SEPS)
@pytest.mark.parametrize("params", INDEX_PARAMS, ids=str)
@pytest.mark.parametrize("crop", R.CROPS, ids=str)
def test_picks_match_restatement(crop, params, sep):
    flow, _ = model(crop, params, 3, sep)
    ridx, _, gap = G.reference(crop, params, 3, sep)
    assert not np.any(gap <= GAP_TOL), f"{int(np.sum(gap <= GAP_TOL))} near-ties, smallest gap {gap.min():.3g}"
    assert not np.any(ridx < 0), "a missing rank in the restatement"
    assert np.array_equal(G.flow_to_index(flow, *params[:2]), ridx)


@pytest.mark.parametrize("sep", SEPS)
@pytest.mark.parametrize("crop", R.CROPS, ids=str)
def test_ft0_is_exact_with_ties_to_the_first_index(crop, sep):
    params = (5, 2, 0, 1.0)
    flow, cost = model(crop, params, 3, sep)
    ridx, rcost, _ = G.reference(crop, params, 3, sep)
    assert np.array_equal(cost, rcost)
    assert np.array_equal(G.flow_to_index(flow, 5, 2), ridx)


def test_closed_forms():
    from gqmap_opticalflow_amd import block_match
    z = np.zeros((16, 16))
    flow, cost = block_match(z, z, 1, 1, 1, 1.0, host=True, hypotheses=3, sep=2)
    assert np.all(cost == 0)
    for k, lin in enumerate((0, 2, 6)):  # all costs tie: the first allowed index each time
        assert np.all(G.flow_to_index(flow, 1, 1)[:, :, k] == lin), k
    flow, cost = block_match(z, z, 1, 1, 1, 1.0, host=True, hypotheses=3, sep=3)
    assert np.all(G.flow_to_index(flow, 1, 1)[:, :, 0] == 0) and np.all(cost[:, :, 0] == 0)
    assert np.all(np.isnan(flow[:, :, :, 1:])) and np.all(np.isposinf(cost[:, :, 1:]))
    A, B = R.crop_pair(R.CROPS[3])
    flow, cost = block_match(A, B, 0, 0, 3, 1.7, host=True, hypotheses=2)
    assert np.all(flow[:, :, :, 0] == 0) and np.all(np.isfinite(cost[:, :, 0]))
    assert np.all(np.isnan(flow[:, :, :, 1])) and np.all(np.isposinf(cost[:, :, 1]))
    # one bit pattern for every missing entry
    assert np.all(flow[:, :, :, 1].view(np.uint64) == 0x7FF8000000000000)


@pytest.mark.parametrize("kw", [dict(H=0), dict(H=5), dict(sep=0), dict(sep=66)], ids=str)
@pytest.mark.parametrize("entry", ["gqmap_block_match_multi_host", "gqmap_block_match_multi"])
def test_argument_errors_write_nothing(entry, kw):
    """Both entry points reject H and sep before anything else: the device one
    needs no device to do so, launches nothing and leaves elapsed_ms alone."""
    from gqmap_opticalflow_amd import _lib
    lib = _lib.load()
    a = dict(H=2, sep=2)
    a.update(kw)
    A = np.zeros((4, 4), order="F")
    flow = np.full((4, 4, 2, 4), 77.0, order="F")
    cost = np.full((4, 4, 4), 77.0, order="F")
    ms = C.c_double(-1.0)
    args = [_lib.dptr(A), _lib.dptr(A), 4, 4, 1, 1, 1, C.c_double(1.0), a["H"], a["sep"], _lib.dptr(flow),
            _lib.dptr(cost)]
    if entry == "gqmap_block_match_multi":
        args += [C.cast(C.byref(ms), _lib._D), 0]
    assert getattr(lib, entry)(*args) == 1  # GQMAP_ERR_INVALID_ARG
    assert entry.encode() in lib.gqmap_last_error()
    assert np.all(flow == 77.0) and np.all(cost == 77.0) and ms.value == -1.0


def test_python_layer_rejects_bad_hypothesis_counts():
    from gqmap_opticalflow_amd import block_match, initial_state
    from gqmap_opticalflow_amd._lib import GqmapError
    z = np.zeros((4, 4))
    for H in (0, 5):
        with pytest.raises(ValueError):
            block_match(z, z, 1, 1, 1, 1.0, host=True, hypotheses=H)
    with pytest.raises(GqmapError, match="gqmap_block_match_multi_host"):
        block_match(z, z, 1, 1, 1, 1.0, host=True, hypotheses=2, sep=66)
    o = dict(L=3, minu=-2.0, maxu=2.0, minv=-2.0, maxv=2.0)
    with pytest.raises(ValueError):  # H = L + 1
        initial_state(o, 4, 4, flow=np.zeros((4, 4, 2, 4)))


def test_initial_state_takes_one_flow_per_component():
    """The host copy of gqmap_init_state_flows: slice l into component l,
    clamped; NaN keeps the draw; H = 1 is the 3-D call."""
    from gqmap_opticalflow_amd import initial_state
    from tests._initflow import make_flow
    o = dict(L=3, minu=-2.0, maxu=3.0, minv=-1.0, maxv=0.5)
    M, N = 6, 5
    f = np.stack([make_flow(M, N, seed=s) for s in (1, 2)], axis=3)
    f[2, 2, :, 1] = np.nan
    base, got = initial_state(o, M, N, seed=3), initial_state(o, M, N, seed=3, flow=f)
    for l in range(2):
        for plane, pbase, x, lo, hi in ((got.muu, base.muu, f[:, :, 0, l], -2.0, 3.0),
                                        (got.muv, base.muv, f[:, :, 1, l], -1.0, 0.5)):
            with np.errstate(invalid="ignore"):
                known = ~(np.isnan(x) | (np.abs(x) > 1e9))
            assert np.array_equal(plane[:, :, l][known], np.clip(x[known], lo, hi))
            assert np.array_equal(plane[:, :, l][~known], pbase[:, :, l][~known])
    for k in ("sigu", "sigv", "pn", "rou", "w", "alpha"):
        assert np.array_equal(getattr(got, k), getattr(base, k)), k
    assert np.array_equal(got.muu[:, :, 2], base.muu[:, :, 2]) and np.array_equal(got.muv[:, :, 2], base.muv[:, :, 2])
    one, three_d = initial_state(o, M, N, seed=3, flow=f[:, :, :, :1]), initial_state(o, M, N, seed=3, flow=f[:, :, :, 0])
    assert np.array_equal(one.muu, three_d.muu) and np.array_equal(one.muv, three_d.muv)


def test_block_match_init_without_hypotheses_is_unchanged_and_with_them_negates():
    from gqmap_opticalflow_amd import block_match, block_match_init
    I1, I2 = R.crop_pair(R.CROPS[0])
    out, _ = block_match(I1, I2, 3, 3, 2, 1.0, host=True)
    rng = dict(minu=-3.0, maxu=3.0, minv=-3.0, maxv=3.0)
    flow, ranges = block_match_init(I1, I2, 3, 3, 2, 1.0, host=True)
    assert ranges == rng and flow.shape == (40, 48, 2) and np.array_equal(flow, 0.0 - out)
    sflow, ranges = block_match_init(I1, I2, 3, 3, 2, 1.0, engine="super", host=True)
    assert ranges == rng and np.array_equal(sflow, (0.0 - out).reshape(10, 4, 12, 4, 2).mean(axis=(1, 3)))
    # sep = 7 > 2U: ranks 1, 2 are missing and stay NaN through the negation
    multi, ranges = block_match_init(I1, I2, 3, 3, 2, 1.0, host=True, hypotheses=3, sep=7)
    assert ranges == rng and multi.shape == (40, 48, 2, 3)
    assert np.array_equal(multi[..., 0], flow) and np.all(np.isnan(multi[..., 1:]))
    multi, _ = block_match_init(I1, I2, 3, 3, 2, 1.0, host=True, hypotheses=3)
    mo, _ = block_match(I1, I2, 3, 3, 2, 1.0, host=True, hypotheses=3)
    assert np.array_equal(multi, 0.0 - mo) and np.all(np.isfinite(multi))
    smulti, _ = block_match_init(I1, I2, 3, 3, 2, 1.0, engine="super", host=True, hypotheses=3)
    assert smulti.shape == (10, 12, 2, 3) and np.array_equal(smulti[..., 0], sflow)  # component 0 whatever H


def test_super_nodes_take_the_cheapest_pixels_hypothesis_not_a_mean():
    """One 4 x 8 image = two nodes, built by hand.  Rank 0: the block mean.
    Rank 1: node 0 has a unique cheapest pixel, node 1 a tie that goes to the
    first pixel in column-major order of the block.  Rank 2: node 0 has one
    pixel with that rank, node 1 none."""
    from gqmap_opticalflow_amd.engine import _super_hypotheses
    M, N, H = 4, 8, 3
    rng = np.random.default_rng(0)
    flow = np.asfortranarray(rng.integers(-7, 8, (M, N, 2, H)).astype(np.float64))
    cost = np.asfortranarray(rng.uniform(10, 20, (M, N, H)))
    cost[2, 1, 1] = 1.0                     # node 0, rank 1: pixel (2, 1)
    cost[3, 4, 1] = cost[1, 5, 1] = 2.0     # node 1, rank 1: tie; (3, 4) is index 3, (1, 5) index 5
    flow[:, :, :, 2], cost[:, :, 2] = np.nan, np.inf
    flow[0, 3, :, 2], cost[0, 3, 2] = (5.0, -6.0), 12.0  # node 0, rank 2: the only pixel that has it
    want = np.full((1, 2, 2, H), np.nan)
    want[0, 0, :, 0], want[0, 1, :, 0] = flow[:, :4, :, 0].mean(axis=(0, 1)), flow[:, 4:, :, 0].mean(axis=(0, 1))
    want[0, 0, :, 1], want[0, 1, :, 1] = flow[2, 1, :, 1], flow[3, 4, :, 1]
    want[0, 0, :, 2] = (5.0, -6.0)
    got = _super_hypotheses(flow, cost)
    assert got.shape == want.shape
    np.testing.assert_array_equal(got, want)
