"""The halo edge job of the plain dataflow item (iter_tile HALO) on the GPU.

Two crops of the RubberWhale pair with integer pixel values, so the fp64
mixture engine takes the binary16 pair store of the padded frame -- the
kernel whose halo job GQ_FLOW_HALO shapes:

  48 x 40  3 x 3 tiles: full 16 x 16 tiles with halo edges from above and from
           the left, and a right column of 8 node columns (tiles whose waves
           2 and 3 hold no valid node);
  36 x 40  a last tile row of 4 node rows: its tiles run as grouped items (a
           tile per wave, each wave its own halo job), the rows above as plain
           items, in one launch.

Three iterations at K = 9, 2, 3 and 11 (40, 2, 4 and 60 mirror pairs: at
K = 2 two of the chain's four slices are empty; K = 2 and 3 end without /
with the centre point), fp64, as a dataflow launch: state and trace bit for
bit against the CPU model (oracle.emu_run) and against one launch per
iteration.  Then one coarse-to-fine level of 48 x 40 at one lane per node
against direct launches, and the stop rule firing inside the launch.
"""
import functools

import numpy as np
import pytest

from tests import _golden as G
from tests.test_gpu_parity import _assert_bit_exact, _emulate, _policy

pytestmark = pytest.mark.gpu

R0, C0 = 150, 200
CROPS = [(48, 40), (36, 40)]
KS = [9, 2, 3, 11]
ITS = 3


@functools.lru_cache(maxsize=None)
def _crop(rows, cols):
    from gqmap_opticalflow_amd import flow_to_color, flowio
    I1, I2, gt = flowio.load_pair("rubberwhale")
    _, _, (minu, maxu, minv, maxv), _ = flow_to_color(gt)
    I1 = np.asfortranarray(I1[R0:R0 + rows, C0:C0 + cols])
    I2 = np.asfortranarray(I2[R0:R0 + rows, C0:C0 + cols])
    assert np.array_equal(I1, np.round(I1)) and np.array_equal(I2, np.round(I2))  # the pair store's condition
    return I1, I2, dict(minu=minu, maxu=maxu, minv=minv, maxv=maxv)


def _mixture_opts(rows, cols, K, **kw):
    return dict(_crop(rows, cols)[2], K=K, L=1, temperature=0.0, drate=0.5, epsn=1e-6, lambdad=1.0, lambdas=5.0,
                split=1, **kw)


def _run(rows, cols, o, its, flow, start=None):
    from gqmap_opticalflow_amd import Engine, initial_state
    I1, I2, _ = _crop(rows, cols)
    with _policy(**(dict(flow=1) if flow else dict(flow=0, graph=0))):
        eng = Engine(o, I1, I2, "mixture", "fp64")
    with eng:
        assert eng.info().split == 1
        assert eng.dataflow() == bool(flow)
        eng.set_state(initial_state(o, rows, cols, seed=0) if start is None else start.copy())
        done, tr = eng.run(its)
        return done, tr, eng.get_state()


@functools.lru_cache(maxsize=None)
def _per_launch(rows, cols, K):
    """One launch per iteration (shared, left unchanged)."""
    return _run(rows, cols, _mixture_opts(rows, cols, K), ITS, False)


@functools.lru_cache(maxsize=None)
def _dataflow(rows, cols, K):
    return _run(rows, cols, _mixture_opts(rows, cols, K), ITS, True)


def _same(a, b):
    (d0, t0, s0), (d1, t1, s1) = a, b
    assert d0 == d1
    np.testing.assert_array_equal(t1, t0)
    for k in G.STATE_KEYS:
        np.testing.assert_array_equal(getattr(s1, k), getattr(s0, k), err_msg=k)
    assert s1.it == s0.it and s1.T == s0.T


def test_crops_have_the_tiles_they_are_for():
    assert (-(-48 // 16), -(-40 // 16), 40 % 16) == (3, 3, 8)
    assert 36 - 2 * 16 == 4  # at most 4 node rows: the last tile row is grouped (k_iter_flow GRP)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("rows,cols", CROPS)
def test_dataflow_bit_exact_vs_cpu_model(rows, cols, K):
    from gqmap_opticalflow_amd import initial_state
    I1, I2, _ = _crop(rows, cols)
    o = _mixture_opts(rows, cols, K)
    e_done, e_tr, e_T, ost = _emulate(o, I1, I2, initial_state(o, rows, cols, seed=0), ITS, "fp64", 1)
    done, tr, g = _dataflow(rows, cols, K)
    assert done == ITS
    _assert_bit_exact(g, tr, done, e_done, e_tr, ost)
    assert g.T == e_T


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("rows,cols", CROPS)
def test_dataflow_bit_exact_vs_per_launch(rows, cols, K):
    a, b = _per_launch(rows, cols, K), _dataflow(rows, cols, K)
    assert a[0] == b[0] == ITS
    _same(a, b)


def test_ctf_level_bit_exact_vs_direct_launches():
    from gqmap_opticalflow_amd import Engine, ctf_options
    rows, cols = 48, 40
    I1, I2, lim = _crop(rows, cols)
    o = ctf_options(its=ITS, **lim)
    o["split"] = 1
    out = []
    for pol, flow in ((dict(flow=0, persist=0, graph=0), False), (dict(flow=1), True)):
        with _policy(**pol):
            eng = Engine(o, I1, I2, "ctf", "fp64")
        with eng:
            assert eng.info().split == 1
            assert eng.dataflow() == flow
            eng.init_state(3)
            done, tr = eng.run(ITS)
            out.append((done, tr, eng.get_state()))
    assert out[0][0] == out[1][0] == ITS
    _same(*out)


def test_stop_rule_inside_the_launch():
    """The stop rule (sum|dmu| < tor) met at row k of one dataflow launch:
    tor just above a value of the trace that lies below every earlier one
    (the threshold form of tests/test_gpu_flow.py), so items of iteration
    k + 1 are in flight when finalize(k) stops the run."""
    rows, cols, its = 48, 40, 40
    o = _mixture_opts(rows, cols, 9)
    # sum|dmu| first climbs from the seeded state: start past its peak, where it falls
    _, tr0, _ = _run(rows, cols, o, its, False)
    warm = int(np.argmax(tr0[:its - 8, 1])) + 1
    start = _run(rows, cols, o, warm, False)[2]
    its -= warm
    _, tr, _ = _run(rows, cols, o, its, False, start=start)
    run_min = np.minimum.accumulate(tr[:, 1])
    ks = [k for k in range(2, its) if tr[k, 1] < run_min[k - 1]]
    assert ks, f"no new minimum of sum|dmu| in rows [2, {its}): {tr[:, 1]}"
    k = ks[len(ks) // 2]
    tor = float(tr[k, 1]) * (1 + 1e-12)
    assert int(np.argmax(tr[:, 1] < tor)) == k and k + 1 < its
    o = _mixture_opts(rows, cols, 9, tor=tor)
    a = _run(rows, cols, o, its, False, start=start)
    b = _run(rows, cols, o, its, True, start=start)
    assert a[0] == b[0] == k + 1
    _same(a, b)
