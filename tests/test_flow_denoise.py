"""Weighted flow denoising without a device: the library's host model
(gqmap_flow_denoise_host) against the numpy restatement of csrc/gqmap_denoise.h
(tests/_flow_denoise_np.py) and, in the reference's special case, against the C
restatement of legacy/gqmap_cpu.m (oracle.cpu_run), BIT FOR BIT: every
comparison is assert_array_equal on mu, sigma, rou and the trace, and its_done
(the trace's length) must be equal.  Then the refusals, and the full RubberWhale
pair through the host models.  The kernels against the host model:
tests/test_gpu_flow_denoise.py."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests import _blockmatch_np as R
from tests import _flow_denoise_np as D

NAMES = ("mu", "sigma", "rou", "trace")


@functools.lru_cache(maxsize=None)
def rule():
    from gqmap_opticalflow_amd import gauss_hermite
    return gauss_hermite(9)


def host(flow, var, mu0, sigma0, options, scatter, **kw):
    from gqmap_opticalflow_amd import flow_denoise
    return flow_denoise(flow, var, mu0, sigma0, options, scatter=scatter, host=True, return_trace=True, **kw)


def same(got, want, what=""):
    assert got[3].shape[0] == want[3].shape[0], f"its_done {what}"
    for a, b, k in zip(got, want, NAMES):
        np.testing.assert_array_equal(a, b, err_msg=f"{k} {what}")


def finite_flow(shape):
    flow, _, _, sigma0 = D.fields(shape)
    return np.asfortranarray(np.where(np.isfinite(flow), flow, 0.5)), sigma0


# ---- the reference's engine is the special case ------------------------------------------

@pytest.mark.parametrize("dta", [np.inf, 2.5])
@pytest.mark.parametrize("c", [1.0, 0.7])
@pytest.mark.parametrize("shape", D.SHAPES, ids=str)
def test_constant_field_reference_scatter_is_the_oracle(oracle_lib, shape, c, dta):
    X, W = rule()
    flow, sigma0 = finite_flow(shape)
    o = dict(its=30, K=9, var=c, gama=1.0, dta=dta)
    ref = oracle_lib.cpu_run(o, flow, sigma0, X, W)
    field = np.full(flow.shape, c, order="F")
    same(D.run_options(flow, field, None, sigma0, X, W, o, "reference"), ref, "restatement, field")
    same(host(flow, field, None, sigma0, dict(o, var=123.0), "reference"), ref, "host model, field")
    same(host(flow, None, None, sigma0, o, "reference"), ref, "host model, scalar var")
    same(D.run_options(flow, None, None, sigma0, X, W, o, "reference"), ref, "restatement, scalar var")


# ---- the new territory -------------------------------------------------------------------

@pytest.mark.parametrize("dta", [np.inf, 2.5])
@pytest.mark.parametrize("gama", [1.0, 1.3])
@pytest.mark.parametrize("scatter", ["reference", "adjoint"])
@pytest.mark.parametrize("shape", D.SHAPES, ids=str)
def test_host_model_equals_the_restatement(shape, scatter, gama, dta):
    X, W = rule()
    flow, var, mu0, sigma0 = D.fields(shape)
    seen = D.observed(flow, var)
    assert (~seen).any() and np.isnan(flow).any()
    if min(shape) > 3:
        assert seen.any() and all(k.any() for k in (np.isposinf(var), np.isnan(var), var == 0, var == -1))
    o = dict(its=30, K=9, gama=gama, dta=dta)
    want = D.run_options(flow, var, mu0, sigma0, X, W, o, scatter)
    same(host(flow, var, mu0, sigma0, o, scatter), want)
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all()


@pytest.mark.parametrize("scatter", ["reference", "adjoint"])
def test_a_whole_layer_unobserved(scatter):
    """Layer 1 has no observation at all: it is moved by its edges alone, layer 0 as ever."""
    X, W = rule()
    flow, var, mu0, sigma0 = D.fields((37, 41), layer_off=True)
    assert not D.observed(flow, var)[:, :, 1].any()
    o = dict(its=30, K=9, gama=1.3, dta=2.5)
    want = D.run_options(flow, var, mu0, sigma0, X, W, o, scatter)
    got = host(flow, var, mu0, sigma0, o, scatter)
    same(got, want)
    assert np.isfinite(got[0]).all() and not np.array_equal(got[0][:, :, 1], mu0[:, :, 1])


@pytest.mark.parametrize("scatter", ["reference", "adjoint"])
@pytest.mark.parametrize("shape", D.SHAPES, ids=str)
def test_unobserved_entries_do_not_leak(shape, scatter):
    """What flow and var hold at an unobserved entry (NaN, +Inf, 0, -1, 1e300) reaches nothing."""
    flow, var, mu0, sigma0 = D.fields(shape)
    f2, v2 = D.scrub(flow, var)
    assert not np.array_equal(f2, flow, equal_nan=True) and not np.array_equal(v2, var, equal_nan=True)
    o = dict(its=30, K=9, gama=1.3, dta=2.5)
    same(host(f2, v2, mu0, sigma0, o, scatter), host(flow, var, mu0, sigma0, o, scatter))
    X, W = rule()
    same(D.run_options(f2, v2, mu0, sigma0, X, W, o, scatter), D.run_options(flow, var, mu0, sigma0, X, W, o, scatter))


# ---- stop rule, thread count ---------------------------------------------------------------

@pytest.mark.parametrize("scatter", ["reference", "adjoint"])
def test_the_stop_rule_fires_inside_the_run(scatter):
    X, W = rule()
    flow, var, mu0, sigma0 = D.fields((37, 41))
    o = dict(its=30, K=9, min_its=10)
    full = D.run_options(flow, var, mu0, sigma0, X, W, o, scatter)[3]
    tor = float(full[9:20, 0].mean())  # crossed somewhere in iterations 10..20
    first = next(i + 1 for i in range(9, 30) if full[i, 0] < tor)
    want = D.run_options(flow, var, mu0, sigma0, X, W, dict(o, tor=tor), scatter)
    got = host(flow, var, mu0, sigma0, dict(o, tor=tor), scatter)
    same(got, want)
    assert 10 <= got[3].shape[0] < 30 and got[3].shape[0] == first
    assert got[3][-1, 0] < tor


def test_the_thread_count_shows_in_no_result():
    flow, var, mu0, sigma0 = D.fields((37, 41))
    o = dict(its=12, K=9, gama=1.3, dta=2.5)
    old = os.environ.get("GQMAP_HOST_THREADS")
    runs = []
    try:
        for t in ("1", "3", "7", "64"):
            os.environ["GQMAP_HOST_THREADS"] = t
            runs.append(host(flow, var, mu0, sigma0, o, "adjoint"))
            runs.append(host(flow[:, :3], var[:, :3], mu0[:, :3], sigma0[:, :3], o, "reference"))
    finally:
        if old is None:
            del os.environ["GQMAP_HOST_THREADS"]
        else:
            os.environ["GQMAP_HOST_THREADS"] = old
    for r in runs[2::2]:
        same(r, runs[0])
    for r in runs[3::2]:
        same(r, runs[1])


def test_the_library_rng_draws_sigma0():
    from gqmap_opticalflow_amd import rand_uniform
    flow, var, mu0, _ = D.fields((5, 7))
    o = dict(its=3, K=9)
    sg0 = np.asfortranarray(rand_uniform(4, 3, 70).reshape((5, 7, 2), order="F") + 2)
    same(host(flow, var, mu0, None, o, "adjoint", seed=4), host(flow, var, mu0, sg0, o, "adjoint"))


# ---- refusals ------------------------------------------------------------------------------

def test_a_start_that_is_not_finite_is_refused():
    from gqmap_opticalflow_amd import _lib
    flow, var, mu0, sigma0 = D.fields((5, 7))
    assert np.isnan(flow).any()
    o = dict(its=2, K=9)
    for bad in (np.nan, np.inf, -np.inf):
        m = mu0.copy(order="F")
        m[4, 6, 1] = bad
        with pytest.raises(_lib.GqmapError, match="mu0 must be finite"):
            host(flow, var, m, sigma0, o, "adjoint")
    with pytest.raises(_lib.GqmapError, match="flow is the start"):
        host(flow, var, None, sigma0, o, "adjoint")
    # the outputs of a refused call are untouched
    lib = _lib.load()
    co = _lib.GqmapCpuOptions()
    lib.gqmap_cpu_options_default(C.byref(co))
    out = [np.full((5, 7, 2), 7.0, order="F"), np.full((5, 7, 2), 7.0, order="F"), np.full((5, 7, 2, 2), 7.0, order="F")]
    rc = lib.gqmap_flow_denoise_host(C.byref(co), _lib.dptr(flow), _lib.dptr(var), None, 5, 7, None, C.c_uint64(0), 1,
                                     *map(_lib.dptr, out), None, None)
    assert rc == 1 and all(np.all(a == 7.0) for a in out)


def test_the_step_bound():
    from gqmap_opticalflow_amd import flow_denoise
    flow, _, mu0, sigma0 = D.fields((5, 7))
    var = np.full(flow.shape, 0.25, order="F")
    with pytest.raises(ValueError, match="unstable"):  # 0.1 (4 + 32) = 3.6
        flow_denoise(flow, var, mu0, sigma0, dict(its=2, gama=0.25), host=True)
    flow_denoise(flow, var, mu0, sigma0, dict(its=2, gama=0.25), host=True, check_step=False)
    # the smallest OBSERVED variance counts: a tiny one on an unobserved entry does not
    f2, v2 = flow.copy(order="F"), np.full(flow.shape, 1.0, order="F")
    f2[1, 1, 0], v2[1, 1, 0] = np.nan, 1e-9
    flow_denoise(f2, v2, mu0, sigma0, dict(its=2), host=True)
    v2[2, 2, 0] = 1e-9
    with pytest.raises(ValueError, match="unstable"):
        flow_denoise(f2, v2, mu0, sigma0, dict(its=2), host=True)
    with pytest.raises(ValueError, match="unstable"):  # var=None: the scalar option; 0.1 (12 + 8) = 2
        flow_denoise(np.zeros((4, 4, 2)), None, None, sigma0[:4, :4], dict(its=2, var=1.0 / 12), host=True)
    flow_denoise(np.zeros((4, 4, 2)), None, None, sigma0[:4, :4], dict(its=2, var=1.0 / 11), host=True)


def test_shapes_and_arguments():
    from gqmap_opticalflow_amd import _lib, flow_denoise
    flow, var, mu0, sigma0 = D.fields((5, 7))
    for kw in (dict(var=var[:, :, 0]), dict(mu0=mu0[:4]), dict(sigma0=sigma0[:, :6])):
        with pytest.raises(ValueError):
            flow_denoise(flow, **dict(dict(var=var, mu0=mu0, sigma0=sigma0), **kw), host=True)
    with pytest.raises(ValueError):
        flow_denoise(flow[:, :, 0], host=True)
    with pytest.raises(ValueError):
        flow_denoise(flow, var, mu0, sigma0, scatter="transpose", host=True)
    lib = _lib.load()
    co = _lib.GqmapCpuOptions()
    lib.gqmap_cpu_options_default(C.byref(co))
    out = [np.full((5, 7, 2), 7.0, order="F"), np.full((5, 7, 2), 7.0, order="F"), np.full((5, 7, 2, 2), 7.0, order="F")]
    D_ = _lib.dptr
    good = dict(o=C.byref(co), flow=D_(mu0), M=5, N=7, scatter=1, mu=D_(out[0]))
    for kw in (dict(o=None), dict(flow=None), dict(mu=None), dict(M=1), dict(N=1), dict(scatter=2), dict(scatter=-1)):
        a = dict(good, **kw)
        rc = lib.gqmap_flow_denoise_host(a["o"], a["flow"], D_(var), None, a["M"], a["N"], D_(sigma0), C.c_uint64(0),
                                         a["scatter"], a["mu"], D_(out[1]), D_(out[2]), None, None)
        assert rc == 1, kw
    for K, its in ((0, 2), (17, 2), (9, 0)):
        co.K, co.its = K, its
        rc = lib.gqmap_flow_denoise_host(C.byref(co), D_(mu0), D_(var), None, 5, 7, D_(sigma0), C.c_uint64(0), 1,
                                         *map(D_, out), None, None)
        assert rc == 1, (K, its)
    assert all(np.all(a == 7.0) for a in out)


# ---- the whole RubberWhale pair through the host models ------------------------------------------

def test_rubberwhale_the_adjoint_scatter_improves_its_start_and_the_reference_does_not():
    """Full RubberWhale, (7, 7, 3, 1.7), the refilled sub-pixel start; K = 9, 40
    iterations, sigma0 from the library RNG, AEPE over the known pixels.  One
    pair at untuned knobs.  Measured with the restatement's arithmetic: start
    0.2995; var = 1 everywhere: adjoint 0.2649 (0.0346 below the start), reference
    scatter 0.3940; weighted (var = sigma^2, rejected pixels unobserved) 0.2865."""
    from gqmap_opticalflow_amd import block_match_flow, block_match_init, flow_denoise
    I1, I2, gt = R.rubberwhale()
    start, _, sig, cons = block_match_init(I1, I2, host=True, subpixel=True, sigma_from_cost=True, consistency=True,
                                           fill=True)
    known = np.all(np.abs(gt) <= 1e9, axis=2)
    epe = lambda f: np.sqrt(np.sum((gt - f) ** 2, axis=2))[known].mean()
    assert not np.isnan(start).any()
    a_start = epe(start)
    flat, _, c1 = block_match_flow(I1, I2, host=True, weighted=False, var_default=1.0, denoise=dict(its=40))
    ref, _, c2 = block_match_flow(I1, I2, host=True, weighted=False, var_default=1.0,
                                  denoise=dict(its=40, scatter="reference"))
    wgt, wsig, c3 = block_match_flow(I1, I2, host=True)
    a_flat, a_ref, a_wgt = epe(flat), epe(ref), epe(wgt)
    print(f"AEPE start {a_start:.4f}; var = 1: adjoint {a_flat:.4f}, reference scatter {a_ref:.4f}; weighted {a_wgt:.4f}")
    assert all(np.array_equal(c, cons) for c in (c1, c2, c3))
    assert a_start - a_flat >= 0.025
    assert a_ref > a_start
    assert a_wgt < a_start
    # block_match_flow is the composition it documents
    ones = np.ones(start.shape, order="F")
    np.testing.assert_array_equal(flat, flow_denoise(start, ones, start, options=dict(its=40), host=True)[0])
    with np.errstate(invalid="ignore"):
        var = np.where(np.isfinite(sig), sig * sig, 1.0)
    mu, sg, _ = flow_denoise(np.where(cons[:, :, None], start, np.nan), var, start, options=dict(its=40), host=True)
    np.testing.assert_array_equal(wgt, mu)
    np.testing.assert_array_equal(wsig, sg)
    assert (~cons).any() and np.isnan(sig).any()
