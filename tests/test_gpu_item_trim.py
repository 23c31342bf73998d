"""The trimmed fp64 mixture item of the dataflow launch on the GPU
(k_iter_flow<double, vvo2_t, 0, 1>; gqmap_tuning.h GQ_TAP_BIAS, GQ_EDGE_ADDR32).

The item reads its taps through biased bases -- a cell is iy + M2 ix on a base
lowered by M2 + 1 elements, the second column pair on a base of its own --,
loads its edge operands at 32-bit element offsets and reduces its exact
partial sums over a wave by DPP row operations (GQ_FIXSUM_DPP; the totals feed
the trace).  Address arithmetic and the order of integer additions changed,
so every bit must be what it was: state, trace and MAP flow against the CPU
model (oracle.emu_run) and against one launch per iteration.

The crops of tests/test_gpu_tap_lut.py (RubberWhale, integer pixel values):
40 x 56 -- full 16 x 16 tiles, a right column of 8 node columns -- and 36 x 40,
whose last tile row of 4 node rows runs as grouped items beside plain ones.
K = 9, 2, 3 at 12 iterations, from the seeded start and from a start whose
means sit on minu / maxu / minv / maxv, so that samples clamp to columns 1 and
No and rows 1 and Mo: cell (1, 1) is the biased base's first element and cell
(Mo, No) the last one a gather reaches.  Then the stop rule firing inside a
launch, and a frame outside the tap table's range, which takes the pair
store's kernel.
"""
import functools

import numpy as np
import pytest

from tests import _golden as G
from tests.test_gpu_parity import _assert_bit_exact, _emulate, _policy
from tests.test_gpu_tap_lut import CROPS, _crop, _lib, _opts

pytestmark = pytest.mark.gpu

KS = [9, 2, 3]
ITS = 12


def _start(rows, cols, K, kind):
    """seeded: the library's draw; edges: its means moved onto the flow range's
    ends -- columns left of the middle at minu, the others at maxu, rows above
    the middle at minv, the others at maxv."""
    from gqmap_opticalflow_amd import initial_state
    o = _opts(rows, cols, K)
    st = initial_state(o, rows, cols, seed=0)
    if kind == "edges":
        st.muu[:, :cols // 2] = o["minu"]
        st.muu[:, cols // 2:] = o["maxu"]
        st.muv[:rows // 2] = o["minv"]
        st.muv[rows // 2:] = o["maxv"]
    return st


def _run(rows, cols, o, its, mode, start, kind="plain"):
    """mode: 'launch' one launch per iteration, 'flow' the dataflow launch by
    default.  Returns (done, trace, state, MAP flow, offset store in use)."""
    from gqmap_opticalflow_amd import Engine
    I1, I2, _ = _crop(rows, cols, kind)
    with _policy(**(dict(flow=0, graph=0) if mode == "launch" else dict(flow=1))):
        eng = Engine(o, I1, I2, "mixture", "fp64")
    with eng:
        assert eng.info().split == 1
        assert eng.dataflow() == (mode != "launch")
        tap = _lib().gqmap_debug_tap_lut(eng.ctx)
        eng.set_state(start.copy())
        done, tr = eng.run(its)
        assert _lib().gqmap_debug_persist_off(eng.ctx) == 0  # (no fall-back to one launch per iteration)
        return done, tr, eng.get_state(), eng.map(), tap


@functools.lru_cache(maxsize=None)
def _ref(rows, cols, K, mode, start="seeded", kind="plain"):
    """(shared, left unchanged)"""
    return _run(rows, cols, _opts(rows, cols, K), ITS, mode, _start(rows, cols, K, start), kind)


@functools.lru_cache(maxsize=None)
def _cpu(rows, cols, K, start="seeded", kind="plain"):
    I1, I2, _ = _crop(rows, cols, kind)
    o = _opts(rows, cols, K)
    return _emulate(o, I1, I2, _start(rows, cols, K, start), ITS, "fp64", 1)


def _same(a, b):
    assert a[0] == b[0]
    np.testing.assert_array_equal(b[1], a[1])
    for k in G.STATE_KEYS:
        np.testing.assert_array_equal(getattr(b[2], k), getattr(a[2], k), err_msg=k)
    assert b[2].it == a[2].it and b[2].T == a[2].T
    np.testing.assert_array_equal(b[3], a[3], err_msg="MAP flow")


def _vs_cpu_model(got, cpu):
    e_done, e_tr, e_T, ost = cpu
    assert got[0] == ITS
    _assert_bit_exact(got[2], got[1], got[0], e_done, e_tr, ost)
    assert got[2].T == e_T
    # L = 1: the MAP flow is the component's mean
    np.testing.assert_array_equal(got[3], np.stack([ost.muu[:, :, 0], ost.muv[:, :, 0]], axis=2), err_msg="MAP flow")


def test_edge_start_clamps_at_both_ends_of_both_axes():
    """The start the extremes are for: in the first iteration samples of the
    nodes next to each border lie beyond it (mean on the range's end, sigma 3
    and more)."""
    for rows, cols in CROPS:
        o = _opts(rows, cols, 9)
        st = _start(rows, cols, 9, "edges")
        assert o["minu"] < -1 and o["maxu"] > 1 and o["minv"] < -1 and o["maxv"] > 1
        # node (m, n) samples around column n + 1 + mu_u, row m + 1 + mu_v (1-based)
        assert 2 + st.muu[5, 1, 0] < 1 and cols - 1 + st.muu[5, cols - 2, 0] > cols
        assert 2 + st.muv[1, 5, 0] < 1 and rows - 1 + st.muv[rows - 2, 5, 0] > rows


@pytest.mark.parametrize("start", ["seeded", "edges"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("rows,cols", CROPS)
def test_trimmed_item_bit_exact_vs_cpu_model(rows, cols, K, start):
    got = _ref(rows, cols, K, "flow", start)
    assert got[4] == 1
    _vs_cpu_model(got, _cpu(rows, cols, K, start))


@pytest.mark.parametrize("start", ["seeded", "edges"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("rows,cols", CROPS)
def test_trimmed_item_bit_exact_vs_per_launch(rows, cols, K, start):
    a, b = _ref(rows, cols, K, "launch", start), _ref(rows, cols, K, "flow", start)
    assert a[0] == ITS and b[4] == 1
    _same(a, b)


def test_stop_rule_inside_the_launch():
    """tor just above a value of sum|dmu| that lies below every earlier one
    (the form of tests/test_gpu_tap_lut.py): finalize(k) stops the run while
    items of iteration k + 1 are in flight."""
    rows, cols, its = 40, 56, 40
    o = _opts(rows, cols, 9)
    seed = _start(rows, cols, 9, "seeded")
    _, tr0, *_ = _run(rows, cols, o, its, "launch", seed)
    warm = int(np.argmax(tr0[:its - 8, 1])) + 1  # sum|dmu| first climbs from the seeded state: start past its peak
    start = _run(rows, cols, o, warm, "launch", seed)[2]
    its -= warm
    _, tr, *_ = _run(rows, cols, o, its, "launch", start)
    run_min = np.minimum.accumulate(tr[:, 1])
    ks = [k for k in range(2, its) if tr[k, 1] < run_min[k - 1]]
    assert ks, f"no new minimum of sum|dmu| in rows [2, {its}): {tr[:, 1]}"
    k = ks[len(ks) // 2]
    tor = float(tr[k, 1]) * (1 + 1e-12)
    assert int(np.argmax(tr[:, 1] < tor)) == k and k + 1 < its
    o = _opts(rows, cols, 9, tor=tor)
    a = _run(rows, cols, o, its, "launch", start)
    b = _run(rows, cols, o, its, "flow", start)
    assert b[4] == 1 and a[0] == b[0] == k + 1
    _same(a, b)


@pytest.mark.parametrize("K", [9, 3])
def test_frame_beyond_the_table_takes_the_pair_store(K):
    rows, cols = CROPS[0]
    got = _ref(rows, cols, K, "flow", "seeded", "wide")
    assert got[4] == 0
    _vs_cpu_model(got, _cpu(rows, cols, K, "seeded", "wide"))
    _same(_ref(rows, cols, K, "launch", "seeded", "wide"), got)
