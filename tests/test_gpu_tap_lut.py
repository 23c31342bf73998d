"""Taps by LDS table in the fp64 mixture item of the dataflow launch (policy
tap_lut, k_iter_flow<double, vvo2_t, 0, 1>) on the GPU.

Integer frames whose padded values span at most a table's worth (TAPLUT_N =
1276 integers, the bound [-510, 765] of an 8-bit frame) get an offset store
beside the binary16 pair store; the dataflow launch then reads a tap as a
16-bit offset and one ds_read_b64 from a table of doubles in LDS.  Every other
reader -- one launch per iteration (the recovery path), the read-back -- keeps
the pair store, and a frame outside the range keeps the pair store's kernel.

Two crops of the RubberWhale pair (integer pixel values):

  40 x 56  3 x 4 tiles: full 16 x 16 tiles, a bottom row of 8 node rows and a
           right column of 8 node columns;
  36 x 40  a last tile row of 4 node rows: grouped items (a tile per wave).

At these sizes every wave has samples in the padding ring (sigma starts at 3,
the quadrature reaches several sigma).  Three iterations at K = 9, 2, 3 as a
dataflow launch: state and trace bit for bit against the CPU model
(oracle.emu_run), against one launch per iteration and against the pair
store's dataflow kernel (tap_lut = 0).  Then the stop rule inside a launch, an
injected launch failure finished on the pair store, frames at both ends of
the table and beyond it, gqmap_set_images between the two at one size, the
read-back, and the occupancy of the item.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import _golden as G
from tests.test_gpu_parity import _assert_bit_exact, _emulate, _policy

pytestmark = pytest.mark.gpu

R0, C0 = 150, 200
CROPS = [(40, 56), (36, 40)]
KS = [9, 2, 3]
ITS = 3
TAPLUT_N = 1276


def _lib():
    from gqmap_opticalflow_amd import _lib as L
    lib = L.load()
    D = C.POINTER(C.c_double)
    for name, args in (("gqmap_debug_tap_lut", [C.c_void_p]),
                       ("gqmap_debug_flow_per_cu", [C.c_void_p]),
                       ("gqmap_debug_persist_fault", [C.c_void_p, C.c_int]),
                       ("gqmap_debug_persist_off", [C.c_void_p]),
                       ("gqmap_debug_read_vv", [C.c_void_p, D, C.c_size_t, C.POINTER(C.c_int)]),
                       ("gqmap_debug_read_vo", [C.c_void_p, D, D, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)])):
        f = getattr(lib, name)
        f.restype, f.argtypes = C.c_int, args
    return lib


@functools.lru_cache(maxsize=None)
def _crop(rows, cols, kind="plain"):
    """plain: the crop; ends: two inner pixels of the second frame at -510
    and 765, the table's first and last value; wide: at 0 and 1400, more than
    a table holds (every value still exact in binary16: the pair store)."""
    from gqmap_opticalflow_amd import flow_to_color, flowio
    I1, I2, gt = flowio.load_pair("rubberwhale")
    _, _, (minu, maxu, minv, maxv), _ = flow_to_color(gt)
    I1 = np.asfortranarray(I1[R0:R0 + rows, C0:C0 + cols])
    I2 = np.array(I2[R0:R0 + rows, C0:C0 + cols], order="F")
    assert np.array_equal(I1, np.round(I1)) and np.array_equal(I2, np.round(I2))  # the pair store's condition
    if kind != "plain":  # (three pixels or more from the border: the padding keeps its values)
        lo, hi = (-510.0, 765.0) if kind == "ends" else (0.0, 1400.0)
        I2[5, 7], I2[rows - 6, cols - 9] = lo, hi
        I2[17, 20], I2[18, 21] = hi, lo  # (next to each other too: one cell's taps)
    I2.setflags(write=False)
    return I1, I2, dict(minu=minu, maxu=maxu, minv=minv, maxv=maxv)


def _opts(rows, cols, K, **kw):
    return dict(_crop(rows, cols)[2], K=K, L=1, temperature=0.0, drate=0.5, epsn=1e-6, lambdad=1.0, lambdas=5.0,
                split=1, **kw)


def _run(rows, cols, o, its, mode, kind="plain", start=None, fault=None):
    """mode: 'launch' one launch per iteration, 'pair' the dataflow launch on
    the pair store, 'table' the dataflow launch by default (the offset store
    where the frame allows it).  Returns (done, trace, state, offset store in
    use, fell back to one launch per iteration)."""
    from gqmap_opticalflow_amd import Engine, initial_state
    I1, I2, _ = _crop(rows, cols, kind)
    pol = dict(flow=0, graph=0) if mode == "launch" else dict(flow=1, tap_lut=0) if mode == "pair" else dict(flow=1)
    with _policy(**pol):
        eng = Engine(o, I1, I2, "mixture", "fp64")
    with eng:
        assert eng.info().split == 1
        assert eng.dataflow() == (mode != "launch")
        tap = _lib().gqmap_debug_tap_lut(eng.ctx)
        eng.set_state(initial_state(o, rows, cols, seed=0) if start is None else start.copy())
        if fault is not None:
            assert _lib().gqmap_debug_persist_fault(eng.ctx, fault) == 0
        done, tr = eng.run(its)
        return done, tr, eng.get_state(), tap, _lib().gqmap_debug_persist_off(eng.ctx)


@functools.lru_cache(maxsize=None)
def _ref(rows, cols, K, mode, kind="plain"):
    """(shared, left unchanged)"""
    return _run(rows, cols, _opts(rows, cols, K), ITS, mode, kind)


def _same(a, b):
    assert a[0] == b[0]
    np.testing.assert_array_equal(b[1], a[1])
    for k in G.STATE_KEYS:
        np.testing.assert_array_equal(getattr(b[2], k), getattr(a[2], k), err_msg=k)
    assert b[2].it == a[2].it and b[2].T == a[2].T


def _vs_cpu_model(rows, cols, K, kind, got):
    from gqmap_opticalflow_amd import initial_state
    I1, I2, _ = _crop(rows, cols, kind)
    o = _opts(rows, cols, K)
    e_done, e_tr, e_T, ost = _emulate(o, I1, I2, initial_state(o, rows, cols, seed=0), ITS, "fp64", 1)
    assert got[0] == ITS
    _assert_bit_exact(got[2], got[1], got[0], e_done, e_tr, ost)
    assert got[2].T == e_T


def test_crops_have_the_tiles_they_are_for():
    assert (-(-40 // 16), -(-56 // 16), 40 % 16, 56 % 16) == (3, 4, 8, 8)
    assert 36 - 2 * 16 == 4  # at most 4 node rows: the last tile row is grouped (k_iter_flow GRP)


def test_which_contexts_take_the_offset_store():
    from gqmap_opticalflow_amd import Engine
    rows, cols = CROPS[0]
    I1, I2, _ = _crop(rows, cols)
    o = _opts(rows, cols, 9)
    for pol, precision, want in ((dict(flow=1), "fp64", 1), (dict(flow=1, tap_lut=0), "fp64", 0),
                                 (dict(flow=1, vv_pair=0), "fp64", 0), (dict(flow=1), "fp32", 0)):
        with _policy(**pol):
            eng = Engine(o, I1, I2, "mixture", precision)
        with eng:
            assert _lib().gqmap_debug_tap_lut(eng.ctx) == want, (pol, precision)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("rows,cols", CROPS)
def test_table_taps_bit_exact_vs_cpu_model(rows, cols, K):
    got = _ref(rows, cols, K, "table")
    assert got[3] == 1 and got[4] == 0
    _vs_cpu_model(rows, cols, K, "plain", got)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("rows,cols", CROPS)
def test_table_taps_bit_exact_vs_per_launch_and_pair_store(rows, cols, K):
    a, b, c = (_ref(rows, cols, K, m) for m in ("launch", "pair", "table"))
    assert (a[3], b[3], c[3]) == (1, 0, 1)  # (per launch: the store is there, its kernels read the pair store)
    assert a[0] == ITS
    _same(a, c)
    _same(b, c)


def test_stop_rule_inside_the_launch():
    """The stop rule (sum|dmu| < tor) met at row k of one dataflow launch: tor
    just above a value of the trace that lies below every earlier one (the
    threshold form of tests/test_gpu_flow.py), so items of iteration k + 1 are
    in flight when finalize(k) stops the run."""
    rows, cols, its = 40, 56, 40
    o = _opts(rows, cols, 9)
    _, tr0, *_ = _run(rows, cols, o, its, "launch")
    warm = int(np.argmax(tr0[:its - 8, 1])) + 1  # sum|dmu| first climbs from the seeded state: start past its peak
    start = _run(rows, cols, o, warm, "launch")[2]
    its -= warm
    _, tr, *_ = _run(rows, cols, o, its, "launch", start=start)
    run_min = np.minimum.accumulate(tr[:, 1])
    ks = [k for k in range(2, its) if tr[k, 1] < run_min[k - 1]]
    assert ks, f"no new minimum of sum|dmu| in rows [2, {its}): {tr[:, 1]}"
    k = ks[len(ks) // 2]
    tor = float(tr[k, 1]) * (1 + 1e-12)
    assert int(np.argmax(tr[:, 1] < tor)) == k and k + 1 < its
    o = _opts(rows, cols, 9, tor=tor)
    a = _run(rows, cols, o, its, "launch", start=start)
    b = _run(rows, cols, o, its, "table", start=start)
    assert b[3] == 1 and a[0] == b[0] == k + 1
    _same(a, b)


@pytest.mark.parametrize("rows,cols", CROPS)
def test_failed_launch_finishes_on_the_pair_store(rows, cols):
    """The failure word raised at the first item of iteration 2 of the launch:
    the host restores the state the launch started from and finishes with one
    launch per iteration, whose kernels read the pair store."""
    o = _opts(rows, cols, 9)
    a = _run(rows, cols, o, 6, "launch")
    b = _run(rows, cols, o, 6, "table", fault=2)
    assert b[3] == 1 and b[4] == 1 and a[4] == 0
    assert b[0] == 6
    _same(a, b)


@pytest.mark.parametrize("K", [9, 3])
def test_frame_at_both_ends_of_the_table(K):
    rows, cols = CROPS[0]
    got = _ref(rows, cols, K, "table", "ends")
    assert got[3] == 1
    _vs_cpu_model(rows, cols, K, "ends", got)
    _same(_ref(rows, cols, K, "launch", "ends"), got)


@pytest.mark.parametrize("K", [9, 3])
def test_frame_beyond_the_table_takes_the_pair_store(K):
    rows, cols = CROPS[0]
    got = _ref(rows, cols, K, "table", "wide")
    assert got[3] == 0
    _vs_cpu_model(rows, cols, K, "wide", got)
    _same(_ref(rows, cols, K, "launch", "wide"), got)
    _same(_ref(rows, cols, K, "pair", "wide"), got)


def _read_vv(ctx, Mo, No):
    from gqmap_opticalflow_amd import _lib as L
    out = np.zeros((Mo + 2) * (No + 2))
    f32 = C.c_int(-1)
    L.check(_lib().gqmap_debug_read_vv(ctx, L.dptr(out), out.size, C.byref(f32)), "gqmap_debug_read_vv")
    return out.reshape((Mo + 2, No + 2), order="F")


def _read_vo(ctx, Mo, No):
    from gqmap_opticalflow_amd import _lib as L
    lo, hi = np.zeros((Mo + 2) * (No + 2)), np.zeros((Mo + 2) * (No + 2))
    tail, rng = C.c_int(-1), (C.c_int * 2)()
    L.check(_lib().gqmap_debug_read_vo(ctx, L.dptr(lo), L.dptr(hi), lo.size, C.byref(tail), rng), "gqmap_debug_read_vo")
    return lo.reshape((Mo + 2, No + 2), order="F"), hi.reshape((Mo + 2, No + 2), order="F"), tail.value, tuple(rng)


def test_set_images_between_the_stores_at_one_size():
    """In range -> beyond the table -> back, one context, one frame size: the
    dataflow launch follows the frame (offset store, pair store, offset
    store), each run the bits of one launch per iteration on that frame, and
    the read-back returns each frame's padded values."""
    from gqmap_opticalflow_amd import Engine, initial_state
    from gqmap_opticalflow_amd import _lib as L
    from oracle import oracle
    rows, cols = CROPS[0]
    o = _opts(rows, cols, 9)
    start = initial_state(o, rows, cols, seed=0)
    with _policy(flow=1):
        eng = Engine(o, *_crop(rows, cols)[:2], "mixture", "fp64")
    with eng:
        for kind, want in (("plain", 1), ("wide", 0), ("plain", 1), ("ends", 1)):
            I1, I2, _ = _crop(rows, cols, kind)
            L.check(eng.lib.gqmap_set_images(eng.ctx, L.dptr(L.f64(I1)), L.dptr(L.f64(I2)), rows, cols), "gqmap_set_images")
            assert _lib().gqmap_debug_tap_lut(eng.ctx) == want, kind
            assert eng.dataflow()
            np.testing.assert_array_equal(_read_vv(eng.ctx, rows, cols), oracle.get_vv(np.asarray(I2)), err_msg=kind)
            eng.set_state(start.copy())
            done, tr = eng.run(ITS)
            _same(_ref(rows, cols, 9, "launch", kind), (done, tr, eng.get_state()))


@pytest.mark.parametrize("kind", ["plain", "ends"])
def test_offset_store_round_trips_against_the_pair_store(kind):
    """The offset store decoded through its table holds the pair store's
    values: the low half of element (r, c) column c, the high half column
    c + 1 (0 past the frame), the zero column and the tail 0; the read-back of
    the pair store is the padded frame, as before."""
    from gqmap_opticalflow_amd import Engine
    from oracle import oracle
    rows, cols = CROPS[1]
    I1, I2, _ = _crop(rows, cols, kind)
    with _policy(flow=1):
        eng = Engine(_opts(rows, cols, 9), I1, I2, "mixture", "fp64")
    with eng:
        vv = _read_vv(eng.ctx, rows, cols)
        np.testing.assert_array_equal(vv, oracle.get_vv(np.asarray(I2)))
        lo, hi, tail, (vmin, vn) = _read_vo(eng.ctx, rows, cols)
        np.testing.assert_array_equal(lo, vv)
        np.testing.assert_array_equal(hi[:, :-1], vv[:, 1:])
        assert not hi[:, -1].any() and tail == 0
        assert vmin == min(0, int(vv.min())) and vn == max(0, int(vv.max())) - vmin + 1 <= TAPLUT_N
        if kind == "ends":
            assert (vmin, vn) == (-510, TAPLUT_N)


def test_two_workgroups_per_cu():
    """The occupancy query the launches size their grid by: the item with the
    table in LDS (31 KB, 249 VGPRs) stays at two workgroups per CU, as the
    pair store's."""
    from gqmap_opticalflow_amd import Engine
    rows, cols = CROPS[0]
    I1, I2, _ = _crop(rows, cols)
    for pol, want in ((dict(flow=1), 1), (dict(flow=1, tap_lut=0), 0)):
        with _policy(**pol):
            eng = Engine(_opts(rows, cols, 9), I1, I2, "mixture", "fp64")
        with eng:
            assert _lib().gqmap_debug_tap_lut(eng.ctx) == want
            assert _lib().gqmap_debug_flow_per_cu(eng.ctx) == 2
