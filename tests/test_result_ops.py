"""The references of tests/_result_ops_np.py are sound, and they bite.

The device tests (tests/test_gpu_result_ops.py) hold k_mixture_map,
k_projsplx and k_flow_color to the C restatement (oracle/gqmap_oracle.c) bit
for bit -- and a mistake made in both would be invisible there.  So the
restatement is held here to references that share no code with either: the
MAP properties P1..P3 (map_properties), the longdouble projection, the numpy
flowToColor.  The planted-error tests show the property checker rejecting
wrong maps: a checker that accepts everything checks nothing.
"""
import functools
import warnings

import numpy as np
import pytest

from tests import _result_ops_np as R


def _map(oracle_lib, fam):
    return oracle_lib.get_map(fam["alpha"], fam["muu"], fam["sigu"], fam["muv"], fam["sigv"], det_exp=True)


def assert_map_properties(mp, fam, what=""):
    for name, p in zip(("P1", "P2", "P3"), R.map_properties_uv(mp, fam)):
        assert p.all(), f"{what}: {name} fails on {int((~p).sum())} of {p.size} entries, first at {np.argwhere(~p)[0]}"


@pytest.mark.parametrize("name", R.FAMILIES)
def test_restated_map_has_the_properties(oracle_lib, name):
    fam = R.FAMILIES[name]()
    mp = _map(oracle_lib, fam)
    assert_map_properties(mp, fam, name)
    if name in R.EXACT:
        np.testing.assert_array_equal(mp, R.exact_answer(name))
    if name == "sym_pair":
        c = R.sym_pair_centre(fam)
        assert np.all(np.abs(mp - c) <= 3.0 * R.tol1(c)), np.abs(mp - c).max()


def test_families_take_the_paths_they_are_for(oracle_lib):
    # interior: the search result, not a mean; far: exp underflows to zero between the means
    for L in (3, 5):
        fam = R.interior(L)
        mp = _map(oracle_lib, fam)
        on_mean = R.is_a_mean(mp[:, :, 0], fam["muu"]) | R.is_a_mean(mp[:, :, 1], fam["muv"])
        assert on_mean.mean() < 0.5  # (side components 5 sigma away move the peak by less than TolX)
    fam = R.far()
    z = (fam["muu"][:, :, 0] - fam["muu"][:, :, 1]) / fam["sigu"][:, :, 1]
    e = -0.5 * z * z
    assert -762 < e.min() < -745 < e.max() < -647
    assert R.M * R.N % 256 != 0 and [m * n for m, n in R.CROPS] == [1, 7, 7, 256, 258]


def test_properties_reject_a_shifted_map(oracle_lib):
    fam = R.random(3)
    mp = _map(oracle_lib, fam)
    off = ~np.stack([R.is_a_mean(mp[:, :, 0], fam["muu"]), R.is_a_mean(mp[:, :, 1], fam["muv"])], axis=2)
    assert off.sum() > 100
    for shift in (1e-3, -1e-3):
        p3 = R.map_properties_uv(mp + shift, fam)[2]
        rejected = (~p3)[off].mean()
        assert rejected >= 0.9, (shift, rejected)


def test_properties_reject_the_least_likely_mean():
    fam = R.interior(3)
    p1, p2, p3 = R.map_properties_uv(R.least_likely_mean(fam), fam)
    assert not p1.any()
    assert p2.all() and p3.all()  # (a mean: only P1 can tell)


@functools.lru_cache(maxsize=None)
def restated_projsplx(n, kind):
    """oracle.projsplx of every column of proj_input(n, kind) (shared, left unchanged)."""
    from oracle import oracle
    Y = R.proj_input(n, kind)
    X = np.asfortranarray(np.stack([oracle.projsplx(Y[:, c]) for c in range(Y.shape[1])], axis=1))
    X.setflags(write=False)
    return X


@pytest.mark.parametrize("n", R.PROJ_N)
def test_restated_projsplx_vs_longdouble(oracle_lib, n):
    worst = [0.0, 0.0]
    for kind in R.PROJ_KINDS:
        e, s = R.check_projection(restated_projsplx(n, kind), R.proj_input(n, kind))
        worst = [max(worst[0], e), max(worst[1], s)]
    print(f"projsplx n={n}: error / bound {worst[0]:.3g}, |sum - 1| / bound {worst[1]:.3g}")
    # the vectorised reference is the column-by-column one
    Y = R.proj_input(n, "ties")[:, :50]
    np.testing.assert_array_equal(R.projsplx_ld(Y), np.stack([R.projsplx_ld(Y[:, c]) for c in range(50)], axis=1))


def test_projsplx_longdouble_known_answers():
    np.testing.assert_array_equal(R.projsplx_ld([2.0, 0.0, 0.0]), [1.0, 0.0, 0.0])
    np.testing.assert_array_equal(R.projsplx_ld([5.0]), [1.0])
    assert np.max(np.abs(R.projsplx_ld([1.0, 1.0, 1.0, 1.0]) - 0.25)) < 1e-18
    y = np.array([0.2, 0.3, 0.5])
    assert np.max(np.abs(R.projsplx_ld(y) - y)) < 1e-16


@pytest.mark.parametrize("name", R.flow_cases())
def test_restated_flow_to_color_vs_numpy(oracle_lib, name):
    from oracle import gqmap_np
    flow, max_flow = R.flow_cases()[name]
    img, flo, stats, unk = oracle_lib.flow_to_color(flow, max_flow)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # (nanmax of the all-NaN field)
        rimg, rflo, rstats, runk = gqmap_np.flow_to_color(flow, max_flow)
    np.testing.assert_array_equal(img, rimg)
    np.testing.assert_array_equal(flo, rflo)
    np.testing.assert_array_equal(stats, np.array(rstats))
    np.testing.assert_array_equal(unk, runk)
    if name.startswith("mixed"):
        assert unk[:2, 0].all() and unk.sum() == 2 and np.isnan(flo[2:4, 0, 0]).all()
        assert not img[:4, 0].any()
