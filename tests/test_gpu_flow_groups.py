"""Groups of partial tiles and long chunks of the dataflow launch (k_iter_flow).

When the last tile row of a frame holds at most 4 node rows, up to four of its
tiles that follow each other in a band's row walk run as one queue item, a
tile per wave; and a dataflow context replays chunks of FLOW_CHUNK iterations
(one launch each) instead of 50.  Both are execution forms only: every case
runs the same options once per launch (policy flow = 0) and once as dataflow
launches (flow = 1, one lane per node) and compares the trace and all nine
state planes bit for bit.

The frames are crops of the RubberWhale pair: small, so that groups and band
edges are met within a few items.  Tiles are 16 x 16 nodes, numbered down the
tile columns; XCD queue x owns the band of (ntiles - x + 7) >> 3 consecutive
tiles after those of the queues before it."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import _golden as G
from tests.test_gpu_parity import _policy

pytestmark = pytest.mark.gpu

TILE = 16
ITS = 30


def flow_chunk():
    from gqmap_opticalflow_amd import _lib
    f = _lib.load().gqmap_debug_flow_chunk
    f.restype = C.c_int
    f.argtypes = []
    return f()


@functools.lru_cache(maxsize=None)
def _pair():
    from gqmap_opticalflow_amd import flow_to_color, flowio
    I1, I2, gt = flowio.load_pair("rubberwhale")
    _, _, (minu, maxu, minv, maxv), _ = flow_to_color(gt)
    o = dict(K=9, L=1, temperature=0.0, drate=0.5, epsn=1e-6, lambdad=1.0, lambdas=5.0,
             minu=minu, maxu=maxu, minv=minv, maxv=maxv, split=1)
    return I1, I2, o


def _crop(rows, cols):
    I1, I2, o = _pair()
    return np.asfortranarray(I1[:rows, :cols]), np.asfortranarray(I2[:rows, :cols]), dict(o)


def bands(ntiles):
    """[s, e) of the 8 XCD queues' bands (k_iter_flow)."""
    out, s = [], 0
    for x in range(8):
        nb = (ntiles - x + 7) >> 3
        out.append((s, s + nb))
        s += nb
    assert s == ntiles
    return out


def last_row_bands(rows, cols):
    """The band of every tile of the last tile row, left to right."""
    tm, tn = -(-rows // TILE), -(-cols // TILE)
    bs = bands(tm * tn)
    tiles = [c * tm + tm - 1 for c in range(tn)]
    return [next(x for x, (s, e) in enumerate(bs) if s <= t < e) for t in tiles]


def _run(o, I1, I2, its, flow, engine="mixture", precision="fp64", seed=0, fault=None, start=None):
    from gqmap_opticalflow_amd import Engine, _lib
    with _policy(flow=1 if flow else 0):
        e = Engine(o, I1, I2, engine, precision)
    try:
        assert e.info().split == 1
        assert e.dataflow() == bool(flow)
        if start is None:
            e.init_state(seed)
        else:
            e.set_state(start.copy())
        if fault is not None:
            f = _lib.load().gqmap_debug_persist_fault
            f.restype = C.c_int
            f.argtypes = [C.c_void_p, C.c_int]
            assert f(e.ctx, fault) == 0
        done, tr = e.run(its)
        # (a launch that gave up would be recovered per launch, bit-exactly:
        # only an injected failure may have taken that path)
        off = _lib.load().gqmap_debug_persist_off
        off.restype = C.c_int
        off.argtypes = [C.c_void_p]
        assert bool(off(e.ctx)) == (fault is not None)
        return done, tr, e.get_state()
    finally:
        e.close()


def _same(a, b):
    (d0, t0, s0), (d1, t1, s1) = a, b
    assert d0 == d1
    np.testing.assert_array_equal(t1, t0)
    for k in G.STATE_KEYS:  # muu, muv, sigu, sigv, pn and the four rou planes
        np.testing.assert_array_equal(getattr(s1, k), getattr(s0, k), err_msg=k)
    assert s1.it == s0.it and s1.T == s0.T


@functools.lru_cache(maxsize=None)
def _ref_100x136(its):
    """The per-launch run of the 100 x 136 crop (shared, left unchanged)."""
    I1, I2, o = _crop(100, 136)
    return _run(o, I1, I2, its, False)


# rows, cols, valid node rows of the last tile row, grouped
CROPS = [
    (100, 136, 4, True),    # vr = 4 and a partial tile column
    (98, 40, 2, True),      # vr = 2; three tile columns: most groups are short
    (97, 272, 1, True),     # vr = 1; 17 bottom tiles
    (96, 136, 16, False),   # no partial row: grouping switches off
    (104, 136, 8, False),   # vr = 8: no grouping
    (20, 136, 4, True),     # a full tile row above a vr = 4 row
]


@pytest.mark.parametrize("rows,cols,vr,grouped", CROPS)
def test_groups_bit_exact_vs_per_launch(rows, cols, vr, grouped):
    assert rows - (-(-rows // TILE) - 1) * TILE == vr and (vr <= 4) == grouped
    # a band boundary falls inside the last tile row: its tiles lie in more
    # than one band, so groups end at band edges
    lb = last_row_bands(rows, cols)
    assert len(set(lb)) >= 2, lb
    I1, I2, o = _crop(rows, cols)
    ref = _ref_100x136(ITS) if (rows, cols) == (100, 136) else _run(o, I1, I2, ITS, False)
    got = _run(o, I1, I2, ITS, True)
    assert ref[0] == got[0] == ITS
    _same(ref, got)


def test_groups_of_several_tiles_exist():
    """The crops above do form groups of more than one tile (a band holding
    two or more tiles of the last row) as well as single-tile groups."""
    sizes = set()
    for rows, cols, vr, grouped in CROPS:
        if grouped:
            lb = last_row_bands(rows, cols)
            sizes |= {min(4, lb.count(x) - 4 * g) for x in set(lb) for g in range((lb.count(x) + 3) // 4)}
    assert {1, 2} <= sizes, sizes


STOP_STEP0 = 0.002  # a step this small lets sum|dmu| fall steadily once the first transient is over


@functools.lru_cache(maxsize=None)
def _stop_ref(warm, its):
    """The 100 x 136 crop with the small step, per launch: the state after
    `warm` iterations (None: the seeded initial state) and the trace of the
    `its` iterations that follow it (shared, left unchanged)."""
    I1, I2, o = _crop(100, 136)
    o = dict(o, step0=STOP_STEP0)
    start = _run(o, I1, I2, warm, False)[2] if warm else None
    return start, _run(o, I1, I2, its, False, start=start)[1]


def _stop_case(lo, hi, its, warm):
    """The stop rule (sum|dmu| < tor) met at row k in [lo, hi) of a run of
    `its` iterations: tor just above a value of the trace that lies below
    every earlier one."""
    I1, I2, o = _crop(100, 136)
    start, tr = _stop_ref(warm, its)
    assert len(tr) == its
    run_min = np.minimum.accumulate(tr[:, 1])
    ks = [k for k in range(max(lo, 1), hi) if tr[k, 1] < run_min[k - 1]]
    assert ks, f"no new minimum of sum|dmu| in rows [{lo}, {hi})"
    k = ks[len(ks) // 2]
    o = dict(o, step0=STOP_STEP0, tor=float(tr[k, 1]) * (1 + 1e-12))
    a = _run(o, I1, I2, its, False, start=start)
    b = _run(o, I1, I2, its, True, start=start)
    assert a[0] == b[0] == k + 1
    _same(a, b)


def test_stop_rule_inside_first_50():
    """Launch-local row 5..49 of the first chunk's launch (from a state 150
    iterations into the solve, where the trace falls from the first row on)."""
    _stop_case(5, 50, flow_chunk() + 20, 150)


def test_stop_rule_between_50_and_flow_chunk():
    fc = flow_chunk()
    assert fc > 52, fc
    _stop_case(50, fc, fc + 20, 0)


def test_stop_rule_in_leftover_launch():
    fc = flow_chunk()
    _stop_case(fc, fc + 20, fc + 20, 0)


@pytest.mark.parametrize("j", [0, 60])
def test_failed_launch_recovers_bit_exact(j):
    """The failure word raised at the first item of launch-local iteration j
    of the chunk's launch: restored from the snapshot, finished per launch."""
    fc = flow_chunk()
    assert j < fc
    I1, I2, o = _crop(100, 136)
    its = fc + 20
    b = _run(o, I1, I2, its, True, fault=j)
    assert b[0] == its
    _same(_ref_100x136(its), b)


def test_groups_fp32():
    I1, I2, o = _crop(100, 136)
    _same(_run(o, I1, I2, ITS, False, precision="fp32"), _run(o, I1, I2, ITS, True, precision="fp32"))


def test_groups_ctf_level():
    """One coarse-to-fine level engine (gqmap_ctf arithmetic) at one lane per node."""
    from gqmap_opticalflow_amd import ctf_options
    I1, I2, o = _crop(100, 136)
    oc = ctf_options(its=ITS, minu=o["minu"], maxu=o["maxu"], minv=o["minv"], maxv=o["maxv"])
    oc["split"] = 1
    a = _run(oc, I1, I2, ITS, False, engine="ctf", seed=3)
    b = _run(oc, I1, I2, ITS, True, engine="ctf", seed=3)
    assert a[0] == b[0] == ITS
    _same(a, b)


def test_c2_two_chunks_and_leftover():
    """The full C2 frame (388 x 584: 37 tiles of 4 rows at the bottom), two
    chunk graphs and a leftover of 7 iterations, fp64."""
    I1, I2, o = _pair()
    its = 2 * flow_chunk() + 7
    a = _run(o, I1, I2, its, False)
    b = _run(o, I1, I2, its, True)
    assert a[0] == b[0] == its
    _same(a, b)
