"""Weighted flow denoising on the device (gqmap_flow_denoise,
gqmap_flow_denoise_device) against the library's host model, which
tests/test_flow_denoise.py pins to the numpy restatement and to the C
restatement of legacy/gqmap_cpu.m: the same fp64 operations in the same order,
so BIT FOR BIT -- assert_array_equal on mu, sigma, rou and the trace, equal
its_done, no tolerance anywhere.  2MN is no multiple of 64 on the ragged
shapes."""
import ctypes as C

import numpy as np
import pytest

from tests import _blockmatch_np as R
from tests import _flow_denoise_np as D

pytestmark = pytest.mark.gpu

NAMES = ("mu", "sigma", "rou", "trace")


def run(flow, var, mu0, sigma0, options, scatter, host, **kw):
    from gqmap_opticalflow_amd import flow_denoise
    return flow_denoise(flow, var, mu0, sigma0, options, scatter=scatter, host=host, return_trace=True, **kw)


def same(got, want, what=""):
    assert got[3].shape[0] == want[3].shape[0], f"its_done {what}"
    for a, b, k in zip(got, want, NAMES):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=f"{k} {what}")


def finite_flow(shape):
    flow, _, _, sigma0 = D.fields(shape)
    return np.asfortranarray(np.where(np.isfinite(flow), flow, 0.5)), sigma0


def to_dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.asfortranarray(a)).to("cuda:0")


@pytest.mark.parametrize("c", [1.0, 0.7])
@pytest.mark.parametrize("shape", D.SHAPES, ids=str)
def test_constant_field_reference_scatter_is_gqmap_cpu(shape, c):
    """The reference's engine is the special case: the host model, the existing entry
    gqmap_cpu and the kernels with a constant variance field (and with none)."""
    from gqmap_opticalflow_amd import gqmap_cpu
    flow, sigma0 = finite_flow(shape)
    assert (shape[0] * shape[1] * 2) % 64 != 0
    field = np.full(flow.shape, c, order="F")
    for dta in (np.inf, 2.5):
        o = dict(its=30, K=9, var=c, gama=1.0, dta=dta)
        old = gqmap_cpu(o, flow, sigma0=sigma0, return_trace=True)
        same(run(flow, field, None, sigma0, dict(o, var=123.0), "reference", False), old, f"field, dta={dta}")
        same(run(flow, None, None, sigma0, o, "reference", False), old, f"scalar var, dta={dta}")
        same(run(flow, field, None, sigma0, o, "reference", True), old, f"host model, dta={dta}")


@pytest.mark.parametrize("scatter", ["reference", "adjoint"])
@pytest.mark.parametrize("shape", D.SHAPES, ids=str)
def test_kernels_equal_the_host_model(shape, scatter):
    flow, var, mu0, sigma0 = D.fields(shape)
    assert (~D.observed(flow, var)).any()
    for gama in (1.0, 1.3):
        for dta in (np.inf, 2.5):
            o = dict(its=30, K=9, gama=gama, dta=dta)
            same(run(flow, var, mu0, sigma0, o, scatter, False), run(flow, var, mu0, sigma0, o, scatter, True),
                 f"gama={gama} dta={dta}")
    # K as a run-time value, a scalar variance that is not 1, and a NaN flow without a field
    o = dict(its=12, K=7, var=0.6, gama=1.3, dta=2.5)
    same(run(flow, var, mu0, sigma0, o, scatter, False), run(flow, var, mu0, sigma0, o, scatter, True), "K=7")
    same(run(flow, None, mu0, sigma0, o, scatter, False), run(flow, None, mu0, sigma0, o, scatter, True), "no field")


@pytest.mark.parametrize("scatter", ["reference", "adjoint"])
def test_a_whole_layer_unobserved(scatter):
    flow, var, mu0, sigma0 = D.fields((37, 41), layer_off=True)
    assert not D.observed(flow, var)[:, :, 1].any()
    o = dict(its=30, K=9, gama=1.3, dta=2.5)
    got = run(flow, var, mu0, sigma0, o, scatter, False)
    same(got, run(flow, var, mu0, sigma0, o, scatter, True))
    f2, v2 = D.scrub(flow, var)
    same(run(f2, v2, mu0, sigma0, o, scatter, False), got, "unobserved entries rewritten")


@pytest.mark.parametrize("scatter", ["reference", "adjoint"])
def test_the_stop_rule_fires_inside_the_run(scatter):
    flow, var, mu0, sigma0 = D.fields((37, 41))
    o = dict(its=30, K=9, min_its=10)
    full = run(flow, var, mu0, sigma0, o, scatter, True)[3]
    tor = float(full[9:20, 0].mean())
    got = run(flow, var, mu0, sigma0, dict(o, tor=tor), scatter, False)
    same(got, run(flow, var, mu0, sigma0, dict(o, tor=tor), scatter, True))
    assert 10 <= got[3].shape[0] < 30


def test_device_arrays_same_bits_as_host_arrays():
    """gqmap_flow_denoise_device: inputs resident on the device, outputs left there;
    with a given sigma0 and with the library RNG.  The inputs are left as they were."""
    from gqmap_opticalflow_amd import flow_denoise_device
    flow, var, mu0, sigma0 = D.fields((37, 41))
    dev = [to_dev(a) for a in (flow, var, mu0, sigma0)]
    assert dev[0].stride() == (1, 37, 37 * 41)
    o = dict(its=30, K=9, gama=1.3, dta=2.5, min_its=10, tor=0.2)
    for scatter in ("reference", "adjoint"):
        h = run(flow, var, mu0, sigma0, o, scatter, False)
        d = flow_denoise_device(dev[0], dev[1], dev[2], dev[3], o, scatter=scatter, return_trace=True)
        same([x.cpu().numpy() for x in d], h, scatter)
        h = run(flow, var, mu0, None, o, scatter, False, seed=5)
        d = flow_denoise_device(dev[0], dev[1], dev[2], None, o, scatter=scatter, seed=5, return_trace=True)
        same([x.cpu().numpy() for x in d], h, scatter + ", library RNG")
    # without a field and without a start of its own: the flow is the start
    ff, _ = finite_flow((37, 41))
    same([x.cpu().numpy() for x in flow_denoise_device(to_dev(ff), None, None, dev[3], o, return_trace=True)],
         run(ff, None, None, sigma0, o, "adjoint", False), "flow alone")
    for t, a in zip(dev, (flow, var, mu0, sigma0)):
        np.testing.assert_array_equal(t.cpu().numpy(), a)


def _raw_call(o, flow, var, mu0, mu, sigma, rou, M=8, N=9):
    from gqmap_opticalflow_amd._lib import load
    return load().gqmap_flow_denoise_device(C.byref(o), flow, var, mu0, M, N, None, C.c_uint64(0), 1, mu, sigma, rou,
                                            None, None, 0)


def test_device_arrays_refuse_host_pointers_and_overlaps():
    import torch
    from gqmap_opticalflow_amd import flow_denoise_device, legacy
    from gqmap_opticalflow_amd._lib import load
    M, N = 8, 9
    n = M * N * 2
    with pytest.raises(ValueError):  # row-major device tensor
        flow_denoise_device(torch.zeros((M, N, 2), dtype=torch.float64, device="cuda"))
    with pytest.raises(TypeError):  # host tensor
        flow_denoise_device(torch.from_numpy(np.zeros((M, N, 2), order="F")))
    o = legacy.cpu_options({"its": 2})
    buf = torch.ones(8 * n, dtype=torch.float64, device="cuda")
    base = buf.data_ptr()
    f_, v_, m0_, mu_, sg_, rou_ = (base + 8 * n * i for i in range(6))  # rou takes two slots
    assert _raw_call(o, f_, v_, m0_, mu_, sg_, rou_) == 0, load().gqmap_last_error()
    assert _raw_call(o, f_, None, None, mu_, sg_, rou_) == 0, load().gqmap_last_error()
    # the C-ABI itself refuses host pointers, in every input slot
    h = np.ones((M, N, 2), order="F")
    for args in ((h.ctypes.data, v_, m0_), (f_, h.ctypes.data, m0_), (f_, v_, h.ctypes.data)):
        assert _raw_call(o, *args, mu_, sg_, rou_) == 1
        assert b"device memory" in load().gqmap_last_error()
    # ... and outputs that overlap var or mu0 (partial overlaps included)
    for args, who in (((f_, v_, m0_, v_, sg_, rou_), b"var"), ((f_, v_, m0_, mu_, v_ + 8 * n - 8, rou_ + 8 * n), b"var"),
                      ((f_, v_, m0_, m0_, sg_, rou_), b"mu0"), ((f_, v_, m0_, rou_, rou_ + 8 * n, m0_ + 8 * n - 8), b"mu0"),
                      ((f_, v_, m0_, f_ + 8, sg_, rou_), b"flow")):
        assert _raw_call(o, *args) == 1
        msg = load().gqmap_last_error()
        assert b"overlap" in msg and who in msg, msg


def test_a_start_that_is_not_finite_is_refused_by_the_check_kernel():
    """Every array is on the device, so only a kernel can have looked: the call
    returns GQMAP_ERR_INVALID_ARG and mu, sigma, rou and the trace keep their bits."""
    import torch
    from gqmap_opticalflow_amd import _lib, flow_denoise_device, legacy
    flow, var, mu0, sigma0 = D.fields((37, 41))
    M, N = 37, 41
    o = legacy.cpu_options({"its": 3})
    out = [torch.full((M * N * k,), 7.0, dtype=torch.float64, device="cuda") for k in (2, 2, 4)]
    trace = torch.full((9,), 7.0, dtype=torch.float64, device="cuda")
    lib = _lib.load()
    for where, bad in (((36, 40, 1), np.nan), ((0, 0, 0), np.inf), ((17, 3, 1), -np.inf)):
        m = mu0.copy(order="F")
        m[where] = bad
        d = [to_dev(a) for a in (flow, var, m, sigma0)]
        rc = lib.gqmap_flow_denoise_device(C.byref(o), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), M, N,
                                           d[3].data_ptr(), C.c_uint64(0), 1, *[t.data_ptr() for t in out],
                                           trace.data_ptr(), None, 0)
        assert rc == 1 and b"mu0 must be finite" in lib.gqmap_last_error()
        assert all(bool((t == 7.0).all()) for t in out + [trace])
        with pytest.raises(_lib.GqmapError, match="mu0 must be finite"):
            flow_denoise_device(*d, options=dict(its=3))
        with pytest.raises(_lib.GqmapError, match="mu0 must be finite"):  # the host-array entry, the same kernel
            run(flow, var, m, sigma0, dict(its=3), "adjoint", False)
    d = [to_dev(a) for a in (flow, var, sigma0)]  # the flow holds NaN: it cannot be the start
    rc = lib.gqmap_flow_denoise_device(C.byref(o), d[0].data_ptr(), d[1].data_ptr(), None, M, N, d[2].data_ptr(),
                                       C.c_uint64(0), 1, *[t.data_ptr() for t in out], trace.data_ptr(), None, 0)
    assert rc == 1 and b"flow is the start" in lib.gqmap_last_error()
    assert all(bool((t == 7.0).all()) for t in out + [trace])


@pytest.mark.parametrize("weighted", [True, False])
def test_block_match_flow_device_equals_host(weighted):
    """The 96 x 128 crop of RubberWhale at rows 100:196, columns 200:328; U = V = 7, 20 iterations."""
    from gqmap_opticalflow_amd import block_match_flow
    I1, I2, _ = R.rubberwhale()
    I1, I2 = (np.asfortranarray(a[100:196, 200:328]) for a in (I1, I2))
    kw = dict(U=7, V=7, weighted=weighted, denoise=dict(its=20))
    dev = block_match_flow(I1, I2, host=False, **kw)
    ref = block_match_flow(I1, I2, host=True, **kw)
    for a, b, k in zip(dev, ref, ("flow", "sigma", "consistent")):
        np.testing.assert_array_equal(a, b, err_msg=k)
    assert dev[0].shape == (96, 128, 2) and np.isfinite(dev[0]).all() and 0 < (~dev[2]).sum() < dev[2].size
