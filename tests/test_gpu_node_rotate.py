"""The node quadrature loop (node_sums, pipelined and rotated forms) on the GPU.

A 40 x 56 crop of the RubberWhale pair: three tile rows with a partial last
one (8 node rows), four tile columns with a partial last one (8 columns), and
integer pixel values, so the fp64 mixture engine takes the binary16 pair store
of the padded frame.  Three iterations at K = 9 and at K = 2 (the smallest the
options accept), fp64 and fp32, as a dataflow launch and with one launch per
iteration: state and trace bit for bit against the CPU model (oracle.emu_run),
which runs the straight loop of the same header.  Then one coarse-to-fine
level of the same size at 2 and 4 lanes per node, where the loop runs with
dk = Q and, at K = 2 and Q = 4, every lane holds a single sample: the default
execution form bit for bit against one direct launch per iteration.
"""
import functools

import numpy as np
import pytest

from tests import _golden as G
from tests.test_gpu_parity import _assert_bit_exact, _emulate, _policy

pytestmark = pytest.mark.gpu

ROWS, COLS, R0, C0 = 40, 56, 150, 200
ITS = 3
K_MIN = 2  # gqmap_create: K in [2, KMAX]


@functools.lru_cache(maxsize=None)
def _crop():
    from gqmap_opticalflow_amd import flow_to_color, flowio
    I1, I2, gt = flowio.load_pair("rubberwhale")
    _, _, (minu, maxu, minv, maxv), _ = flow_to_color(gt)
    I1 = np.asfortranarray(I1[R0:R0 + ROWS, C0:C0 + COLS])
    I2 = np.asfortranarray(I2[R0:R0 + ROWS, C0:C0 + COLS])
    assert np.array_equal(I1, np.round(I1)) and np.array_equal(I2, np.round(I2))  # the pair store's condition
    return I1, I2, dict(minu=minu, maxu=maxu, minv=minv, maxv=maxv)


def _mixture_opts(K):
    return dict(_crop()[2], K=K, L=1, temperature=0.0, drate=0.5, epsn=1e-6, lambdad=1.0, lambdas=5.0, split=1)


@functools.lru_cache(maxsize=None)
def _model(K, precision):
    """The CPU model's run from the seeded initial state (shared, left unchanged)."""
    from gqmap_opticalflow_amd import initial_state
    I1, I2, _ = _crop()
    o = _mixture_opts(K)
    st = initial_state(o, ROWS, COLS, seed=0)
    return _emulate(o, I1, I2, st, ITS, precision, 1)


@pytest.mark.parametrize("flow", [1, 0], ids=["dataflow", "per_launch"])
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("K", [9, K_MIN])
def test_mixture_bit_exact_vs_cpu_model(K, precision, flow):
    from gqmap_opticalflow_amd import Engine, initial_state
    I1, I2, _ = _crop()
    o = _mixture_opts(K)
    e_done, e_tr, e_T, ost = _model(K, precision)
    with _policy(**(dict(flow=1) if flow else dict(flow=0, graph=0))):
        eng = Engine(o, I1, I2, "mixture", precision)
    with eng:
        assert eng.info().split == 1
        assert eng.dataflow() == bool(flow)
        eng.set_state(initial_state(o, ROWS, COLS, seed=0))
        done, tr = eng.run(ITS)
        g = eng.get_state()
    assert done == ITS
    _assert_bit_exact(g, tr, done, e_done, e_tr, ost)
    assert g.T == e_T


def _ctf_run(o, direct):
    from gqmap_opticalflow_amd import Engine
    I1, I2, _ = _crop()
    pol = dict(flow=0, persist=0, graph=0) if direct else {}
    with _policy(**pol):
        eng = Engine(o, I1, I2, "ctf", "fp64")
    with eng:
        assert eng.info().split == o["split"]
        eng.init_state(3)
        done, tr = eng.run(ITS)
        return done, tr, eng.get_state()


@pytest.mark.parametrize("K", [9, K_MIN])
@pytest.mark.parametrize("Q", [2, 4])
def test_ctf_level_lanes_per_node_bit_exact_vs_per_launch(Q, K):
    from gqmap_opticalflow_amd import ctf_options
    lim = _crop()[2]
    o = ctf_options(its=ITS, **lim)
    o["K"], o["split"] = K, Q
    d0, t0, s0 = _ctf_run(o, True)
    d1, t1, s1 = _ctf_run(o, False)
    assert d0 == d1 == ITS
    np.testing.assert_array_equal(t1, t0)
    for k in G.STATE_KEYS:
        np.testing.assert_array_equal(getattr(s1, k), getattr(s0, k), err_msg=k)
    assert s1.it == s0.it and s1.T == s0.T
