"""Device parity at degenerate grids: frames smaller than one tile, thin
strips, dataflow launches with fewer tiles than XCD queues, the persistent
launch and the pyramid on 4 x 4 levels.

Every comparison is bit for bit (assert_array_equal): against the CPU model of
the kernel (oracle/gqmap_emul.cpp, pinned at these shapes by
tests/test_small_grids.py), against the per-launch path, against the whole
grid, or against the oracle's plumbing.  Every case asserts the kernel form it
was written for -- lanes per node and kernel shape, Engine.dataflow(),
Engine.persistent(), and that no launch was recovered through the fallback
(gqmap_debug_persist_off == 0): a case that ran on another path is not covered.

Shapes are rows x cols.  Tiles are 16 x 16 nodes at Q = 1 lanes per node,
16 x 8 at 2 (and the role split), 8 x 8 at 4, 8 x 4 at 8, 4 x 4 at 16 and
5 x 1 at 64 (one wave per node)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests import _golden as G
from tests.test_gpu_flow_groups import STOP_STEP0, bands, flow_chunk
from tests.test_gpu_parity import _assert_bit_exact, _emulate, _gh, _oracle_state, _policy
from tests.test_gpu_pyramid import _check_levels, _oracle_pipeline, _pipeline_pair
from tests.test_gpu_rolesplit import ROLE, _shape
from tests.test_gpu_tiles import _assemble, _whole
from tests.test_small_grids import ENGINES, ITS, S, SPLITS, SSUP, SUPER_SPLITS, ids, small_case

pytestmark = pytest.mark.gpu


def _persist_off(eng):
    f = eng.lib.gqmap_debug_persist_off
    f.restype = C.c_int
    f.argtypes = [C.c_void_p]
    return f(eng.ctx)


@functools.lru_cache(maxsize=None)
def _model(engine, L, K, shape, split, precision, its=ITS, temperature=None):
    """The CPU model's run of one small case (shared, left unchanged).
    split 0: the model's own automatic lanes per node (oracle.split_for)."""
    extra = dict(split=split) if split else {}
    I1, I2, o, st = small_case(engine, L, K, *shape, temperature=temperature, **extra)
    return _emulate(o, I1, I2, st, its, precision, None)


class _Shapes:
    """Runs a body per shape and reports every shape that failed, not the first."""

    def __init__(self):
        self.bad = []

    def check(self, shape, fn, *a):
        try:
            fn(*a)
        except AssertionError as e:
            self.bad.append(f"{ids(shape)}: {str(e).strip().splitlines()[0] if str(e).strip() else 'assert'}")

    def done(self):
        assert not self.bad, "\n".join(self.bad)


# ---- A. per-launch kernels, every form, against the CPU model ------------------

def _per_launch_case(engine, L, K, shape, split, precision):
    from gqmap_opticalflow_amd import Engine
    q = 1 if split == ROLE else split
    I1, I2, o, st = small_case(engine, L, K, *shape, split=split)
    e_done, e_tr, e_T, ost = _model(engine, L, K, shape, q, precision)
    assert e_done == ITS
    with Engine(o, I1, I2, engine, precision) as eng:
        assert eng.info().split == q
        assert _shape(eng) == (0 if split == ROLE else split)
        assert not eng.dataflow() and not eng.persistent()
        eng.set_state(st)
        done, tr = eng.run(ITS)
        g = eng.get_state()
        assert _persist_off(eng) == 0
    _assert_bit_exact(g, tr, done, e_done, e_tr, ost)
    assert g.T == e_T and g.it == 1 + ITS


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("engine,L,K", ENGINES)
def test_per_launch_kernels_bit_exact_vs_model(engine, L, K, split, precision):
    # k_iter at Q = 1..16, k_iter_wn (Q = 64) and the role split, one launch
    # per iteration, on every shape of S
    sh = _Shapes()
    with _policy(flow=0, persist=0):
        for shape in S:
            sh.check(shape, _per_launch_case, engine, L, K, shape, split, precision)
    sh.done()


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("split", SUPER_SPLITS)
@pytest.mark.parametrize("L", [3, 1])
def test_per_launch_super_bit_exact_vs_model(L, split, precision):
    # node grids 3 x 3, 3 x 4, 4 x 3, 3 x 17, 17 x 3: one interior row or column
    sh = _Shapes()
    with _policy(flow=0, persist=0):
        for shape in SSUP:
            sh.check(shape, _per_launch_case, "super", L, 11, shape, split, precision)
    sh.done()


def _literal_case(shape):
    from gqmap_opticalflow_amd import Engine
    from oracle import oracle
    I1, I2, o, st = small_case("mixture", 1, 9, *shape)
    o = dict(o, arith="literal")
    ost = _oracle_state(st)
    X, W = _gh(9)
    e_done, e_tr, e_T = oracle.emu_run_lit(o, I1, I2, ost, st.it, ITS, X, W, T=st.T,
                                           nthreads=min(16, os.cpu_count() or 1))
    assert e_done == ITS
    with Engine(o, I1, I2) as eng:
        assert eng.info().split == 1 and _shape(eng) == 1
        assert not eng.dataflow() and not eng.persistent()
        eng.set_state(st)
        done, tr = eng.run(ITS)
        g = eng.get_state()
    _assert_bit_exact(g, tr, done, e_done, e_tr, ost)


def test_per_launch_literal_engine_bit_exact_vs_model():
    # k_iter_lit (options arith = "literal", fp64 mixture) against the CPU
    # model of the literal order: both sum the pixels exactly, so the trace is
    # compared bit for bit as well
    sh = _Shapes()
    with _policy(flow=0, persist=0):
        for shape in S:
            sh.check(shape, _literal_case, shape)
    sh.done()


# ---- B. dataflow launch with few tiles ------------------------------------------

# rows x cols and, for 16 x 16 tiles (Q = 1), the tile grid and what it is
# there for.  XCD queue x owns (ntiles - x + 7) >> 3 tiles: with fewer than 8
# tiles the last queues' bands are empty (test_flow_bands_of_the_shapes).
FLOW_SHAPES = [
    (4, 4),     # 1 x 1: one tile, its own neighbourhood, a grouped last row (vr = 4); bands 1-7 empty
    (16, 16),   # 1 x 1: one full tile, no group; bands 1-7 empty
    (17, 16),   # 2 x 1: two tiles in one column, vr = 1 (the second is a group of one); bands 2-7 empty
    (16, 17),   # 1 x 2: two tile columns, no group; bands 2-7 empty
    (20, 16),   # 2 x 1: tiles_n == 1, vr = 4; bands 2-7 empty
    (4, 136),   # 1 x 9: tiles_m == 1, nine tiles all last-row, groups end at band edges; no band empty
    (33, 40),   # 3 x 3: vr = 1; no band empty (band 0 holds two tiles)
    (36, 100),  # 3 x 7: 21 tiles, vr = 4; no band empty
]
EMPTY_BANDS = {(4, 4): 7, (16, 16): 7, (17, 16): 6, (16, 17): 6, (20, 16): 6, (4, 136): 0, (33, 40): 0, (36, 100): 0}
CHUNK_SHAPES = [(4, 4), (17, 16), (4, 136)]

# engine, L, K, split, precision, extra options
FLOW_ENGINES = [
    ("mixture", 1, 9, 1, "fp64", {}),
    ("mixture", 1, 9, 1, "fp32", {}),
    ("mixture", 1, 9, 1, "fp64", {"arith": "literal"}),
    ("ctf", 1, 11, 1, "fp64", {}),
    ("ctf", 1, 11, 2, "fp64", {}),  # 16 x 8 tiles: twice the tile columns
    ("ctf", 1, 11, 4, "fp64", {}),  # 8 x 8 tiles; runs as items only when forced (policy flow = 1)
]
flow_ids = lambda v: "-".join(map(str, v)) if isinstance(v, dict) else None


def test_flow_bands_of_the_shapes():
    for (rows, cols), empty in EMPTY_BANDS.items():
        nt = -(-rows // 16) * -(-cols // 16)
        assert sum(s == e for s, e in bands(nt)) == empty, (rows, cols)
        assert [s == e for s, e in bands(nt)] == [False] * (8 - empty) + [True] * empty
    assert set(EMPTY_BANDS) == set(FLOW_SHAPES)


def _flow_run(case, engine, precision, its, flow, q):
    """One run under policy flow = 1 / 0: (done, trace, state, stopped)."""
    from gqmap_opticalflow_amd import Engine
    I1, I2, o, st = case
    with _policy(flow=1 if flow else 0):
        e = Engine(o, I1, I2, engine, precision)
    try:
        assert e.info().split == q and _shape(e) == q
        assert e.dataflow() == bool(flow)
        assert not e.persistent()
        e.set_state(st.copy())
        done, tr = e.run(its)
        # a launch that timed out and was recovered per launch must not pass
        assert _persist_off(e) == 0
        return done, tr, e.get_state(), e.info().stopped
    finally:
        e.close()


def _same(a, b):
    assert a[0] == b[0]
    np.testing.assert_array_equal(b[1], a[1])
    for k in G.STATE_KEYS:
        np.testing.assert_array_equal(getattr(b[2], k), getattr(a[2], k), err_msg=k)
    assert b[2].it == a[2].it and b[2].T == a[2].T
    assert a[3] == b[3]


def _flow_case(engine, L, K, shape, split, precision, extra, its, temperature=None):
    case = small_case(engine, L, K, *shape, temperature=temperature, split=split, **extra)
    a =_flow_run(case, engine, precision, its, False, split)
    b = _flow_run(case, engine, precision, its, True, split)
    assert a[0] == b[0] == its
    _same(a, b)


@pytest.mark.parametrize("engine,L,K,split,precision,extra", FLOW_ENGINES, ids=flow_ids)
def test_flow_few_tiles_bit_exact_vs_per_launch(engine, L, K, split, precision, extra):
    sh = _Shapes()
    for shape in FLOW_SHAPES:
        sh.check(shape, _flow_case, engine, L, K, shape, split, precision, extra, 30)
    sh.done()


@pytest.mark.parametrize("engine,L,K,split,precision,extra", FLOW_ENGINES, ids=flow_ids)
def test_flow_few_tiles_chunk_and_leftover(engine, L, K, split, precision, extra):
    # a whole chunk's launch and a leftover launch of 7 (tor = 0: no early stop)
    sh = _Shapes()
    for shape in CHUNK_SHAPES:
        sh.check(shape, _flow_case, engine, L, K, shape, split, precision, dict(extra, tor=0.0), flow_chunk() + 7)
    sh.done()


@pytest.mark.parametrize("shape", SSUP, ids=ids)
def test_flow_super_few_tiles_bit_exact_vs_per_launch(shape):
    # the super engine as items (a mixture component per item; only when
    # forced): 8 x 8 tiles at Q = 4, node grids of one to three tiles
    _flow_case("super", 3, 11, shape, 4, "fp64", {}, 30)


def test_flow_few_tiles_temperature_decay():
    # 17 x 16 with a non-zero temperature that decays every 7 iterations: the
    # items' own copy of the decay
    for engine, K in (("mixture", 9), ("ctf", 11)):
        _flow_case(engine, 1, K, (17, 16), 1, "fp64", {"t_decay_every": 7}, 30, temperature=0.3)


@pytest.mark.parametrize("where", ["row0", "inside"])
@pytest.mark.parametrize("shape", [(4, 4), (33, 40)], ids=ids)
@pytest.mark.parametrize("engine,K", [("mixture", 9), ("ctf", 11)])
def test_flow_few_tiles_stop_rule(engine, K, shape, where):
    its = 120  # inside one chunk's launch; the ctf 33 x 40 trace only falls from row 54 on
    assert its < flow_chunk()
    case = small_case(engine, 1, K, *shape, split=1, step0=STOP_STEP0, tor=0.0)
    if where == "row0":
        k, tor = 0, 1e9
    else:
        # tor just above a value of the trace that lies below every earlier
        # one (test_gpu_flow_groups._stop_case): the rule is first met there
        tr = _flow_run(case, engine, "fp64", its, False, 1)[1]
        assert len(tr) == its
        run_min = np.minimum.accumulate(tr[:, 1])
        ks = [k for k in range(1, its) if tr[k, 1] < run_min[k - 1]]
        assert ks, "no new minimum of sum|dmu| after row 0"
        k = ks[len(ks) // 2]
        tor = float(tr[k, 1]) * (1 + 1e-12)
    case[2]["tor"] = tor
    a = _flow_run(case, engine, "fp64", its, False, 1)
    b = _flow_run(case, engine, "fp64", its, True, 1)
    assert a[0] == b[0] == k + 1
    assert a[3] == b[3] == 1
    assert b[2].it == case[3].it + k + 1
    _same(a, b)


# ---- C. persistent launch on the smallest levels -------------------------------

PERSIST_ITS = 130  # two replayed 50-iteration chunks and a leftover launch of 30


def _persist_case(shape, split, precision):
    from gqmap_opticalflow_amd import Engine
    extra = dict(split=split) if split else {}
    I1, I2, o, st = small_case("ctf", 1, 11, *shape, temperature=0.3, **extra)
    e_done, e_tr, e_T, ost = _model("ctf", 1, 11, shape, split, precision, PERSIST_ITS, 0.3)
    assert e_done == PERSIST_ITS
    with Engine(o, I1, I2, "ctf", precision) as eng:
        assert eng.info().split == (split or 64) and _shape(eng) == (split or 64)
        assert eng.persistent()
        eng.set_state(st)
        done, tr = eng.run(PERSIST_ITS)
        g = eng.get_state()
        assert _persist_off(eng) == 0 and eng.persistent()
    _assert_bit_exact(g, tr, done, e_done, e_tr, ost)
    assert g.T == e_T and g.it == st.it + PERSIST_ITS


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("split", [8, 16, 64, 0])
def test_persistent_small_levels_bit_exact_vs_model(split, precision):
    # split 0: the automatic choice (one wave per node below 2^11 nodes)
    sh = _Shapes()
    for shape in S:
        sh.check(shape, _persist_case, shape, split, precision)
    sh.done()


@pytest.mark.parametrize("where", ["row0", "inside"])
@pytest.mark.parametrize("split", [8, 64])
@pytest.mark.parametrize("shape", [(4, 4), (5, 17)], ids=ids)
def test_persistent_small_levels_stop_rule(shape, split, where):
    # the speculative iteration after the stopping one leaves no trace in the
    # state, the trace, Ctl::it or done: all equal the CPU model's stopped run
    from gqmap_opticalflow_amd import Engine
    its = 60
    # (the small step of tests/test_gpu_flow_groups.py: sum|dmu| falls from the first rows on)
    I1, I2, o, st = small_case("ctf", 1, 11, *shape, split=split, tor=0.0, step0=STOP_STEP0)
    if where == "row0":
        k, tor = 0, 1e9
    else:
        # a row of the first 50-iteration chunk whose sum|dmu| lies below every earlier one
        ptd = _emulate(o, I1, I2, st, 45, "fp64", None)[1][:, 1]
        run_min = np.minimum.accumulate(ptd)
        ks = [k for k in range(1, 45) if ptd[k] < run_min[k - 1]]
        assert ks, "no new minimum of sum|dmu| after row 0"
        k = ks[len(ks) // 2]
        tor = float(ptd[k]) * (1 + 1e-12)
    o = dict(o, tor=tor)
    e_done, e_tr, e_T, ost = _emulate(o, I1, I2, st, its, "fp64", None)
    assert e_done == k + 1
    with Engine(o, I1, I2, "ctf", "fp64") as eng:
        assert eng.info().split == split and eng.persistent()
        eng.set_state(st)
        done, tr = eng.run(its)
        g = eng.get_state()
        assert eng.info().stopped == 1
        assert eng.run(30)[0] == 0
        g2 = eng.get_state()
        assert _persist_off(eng) == 0
    _assert_bit_exact(g, tr, done, e_done, e_tr, ost)
    assert g.it == g2.it == st.it + e_done and g.T == e_T
    for key in G.STATE_KEYS:
        np.testing.assert_array_equal(getattr(g2, key), getattr(g, key), err_msg=key)


# ---- D. thin column strips --------------------------------------------------------

# rows x cols, strips: 20 x 9 / 9 and 5 x 4 / 4 give every strip one owned
# column (between two ghost columns inside the grid); at Q = 64 (5 x 1 tiles)
# the left ghost column is a tile column of its own that is never launched
STRIPS = [((20, 9), 4), ((20, 9), 9), ((20, 6), 3), ((5, 4), 4), ((20, 12), 5)]


def _strip_problem(engine, L, shape, split):
    extra = dict(split=split) if split else {}
    I1, I2, o, _ = small_case(engine, L, 11 if engine == "super" else 9, *shape, t_decay_every=15, **extra)
    if engine != "super":
        o = dict(o, temperature=0.05, drate=0.75)  # (tests/test_gpu_tiles.py _problem)
    return I1, I2, o


def _strip_case(engine, L, precision, shape, n, split, q, its=40, init=None):
    from gqmap_opticalflow_amd import Engine, tile_group_run
    I1, I2, o = _strip_problem(engine, L, shape, split)
    start = init or (lambda e: e.init_state(3))
    with Engine(o, I1, I2, engine, precision) as e:
        assert e.info().split == q
        start(e)
        first = e.get_state()
        done, tr = e.run(its)
        ref = e.get_state()
    assert done == its
    tiles = [Engine(o, I1, I2, engine, precision, n_tiles=n, tile=t) for t in range(n)]
    try:
        assert all(t.info().split == q and _shape(t) == q for t in tiles)
        assert [t.col0 for t in tiles] + [tiles[-1].col1] == [ref.muu.shape[1] * t // n for t in range(n + 1)]
        for t in tiles:
            start(t)
        got0 = _assemble(tiles, lambda t: t.get_state())
        for k in G.STATE_KEYS[:6]:
            np.testing.assert_array_equal(getattr(got0, k), getattr(first, k), err_msg="init " + k)
        tdone, ttr = tile_group_run(tiles, its)
        assert tdone == its
        np.testing.assert_array_equal(ttr, tr)
        got = _assemble(tiles, lambda t: t.get_state())
        for k in G.STATE_KEYS:
            np.testing.assert_array_equal(getattr(got, k), getattr(ref, k), err_msg=k)
    finally:
        for t in tiles:
            t.close()


@pytest.mark.parametrize("split", [0, 1, 4])
@pytest.mark.parametrize("L,precision", [(1, "fp64"), (3, "fp32")])
def test_thin_strips_bit_exact_vs_whole_grid(L, precision, split):
    # split 0: the automatic choice, one wave per node on grids this small
    sh = _Shapes()
    for shape, n in STRIPS:
        sh.check(shape + (n,), _strip_case, "mixture", L, precision, shape, n, split, split or 64)
    sh.done()


@pytest.mark.parametrize("split", [0, 1])
def test_one_column_strips_take_the_seeds(split):
    # gqmap_init_state_seeded on 20 x 9 in nine strips: the ghost columns of
    # the one-column strips take the neighbours' flows and widths
    from tests._blockmatch_gpu import flows
    from tests.test_gpu_block_match_refine import widths
    M, N = 20, 9
    o = _strip_problem("mixture", 3, (M, N), split)[2]
    f, s = flows(M, N, 3, seed=11), widths(M, N, 3, 13, o)
    _strip_case("mixture", 3, "fp64", (M, N), 9, split, split or 64, its=10,
                init=lambda e: e.init_state_from_flow(f, seed=4, sigma=s))


def test_thin_strips_super():
    # a 16 x 36 image: 4 x 9 nodes in 3 strips of 3 node columns
    _strip_case("super", 3, "fp64", (16, 36), 3, 0, 16)


# ---- E. pyramid and its plumbing at the smallest levels ---------------------

PYRAMIDS = [((32, 48), (1 / 8, 1 / 4, 1 / 2, 1.0)), ((64, 64), (1 / 16, 1 / 8, 1 / 4, 1 / 2, 1.0)),
            ((8, 8), (1 / 2, 1.0)), ((4, 4), (1.0,))]


@functools.lru_cache(maxsize=None)
def _pyramid_case(shape):
    I1, I2, _, _, rng = _pipeline_pair("Grove3", (150, 200) + shape)
    return I1, I2, rng


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("shape,scales", PYRAMIDS, ids=ids)
def test_small_pyramids_bit_exact_vs_oracle_pipeline(shape, scales, precision):
    from gqmap_opticalflow_amd import Pyramid, ctf_options
    I1, I2, rng = _pyramid_case(shape)
    opts = ctf_options(its=12, **rng)
    warp, levels = _oracle_pipeline(opts, I1, I2, scales, 7, precision)
    assert np.isfinite(warp).all()
    with Pyramid(opts, scales, precision) as p:
        p.set_images(I1, I2)
        flow, its, ms = p.run(seed=7)
        assert its == [lv["its"] for lv in levels]
        assert [p.level(l)["I1w"].shape for l in range(len(scales))] == \
            [(int(np.ceil(shape[0] * s)), int(np.ceil(shape[1] * s))) for s in scales]
        assert p.level(0)["I1w"].shape[0] == 4  # the smallest level the library takes
        _check_levels(p, levels, warp, flow)
        flow2, its2, _ = p.run(seed=7)  # a second run from the same seed repeats bit for bit
        assert its2 == its
        np.testing.assert_array_equal(flow2, flow)
        _check_levels(p, levels, warp, flow2)


def test_small_pyramids_fill_missing_samples():
    """At least one level of the pyramids above warps samples out of its frame,
    so the fill kernel has missing entries to fill (checked with the oracle on
    the CPU: the unfilled warped frame of the level holds NaN)."""
    from gqmap_opticalflow_amd import ctf_options
    from oracle import oracle
    holes = 0
    for shape, scales in PYRAMIDS:
        I1, I2, rng = _pyramid_case(shape)
        _, levels = _oracle_pipeline(ctf_options(its=12, **rng), I1, I2, scales, 7, "fp64")
        for l in range(1, len(scales)):
            win = np.asfortranarray(oracle.imresize(levels[l - 1]["warp"], 2.0) * 2)
            raw = oracle.warp_image(oracle.imresize(I1, scales[l]), win, fill=False)
            np.testing.assert_array_equal(oracle.warp_image(oracle.imresize(I1, scales[l]), win), levels[l]["I1w"])
            holes += int(np.isnan(raw).any())
    assert holes > 0


@pytest.mark.parametrize("antialias", [True, False])
@pytest.mark.parametrize("scale", [2.0, 0.5, 1.7])
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (2, 3), (3, 2, 2)], ids=ids)
def test_imresize_tiny_inputs_bit_exact(shape, scale, antialias):
    # tap tables of a 1- or 2-long axis: every tap mirrors back into the input
    from gqmap_opticalflow_amd import imresize
    from oracle import oracle
    A = np.asfortranarray(np.random.default_rng(5).random(shape) * 255)
    a, b = imresize(A, scale, antialias), oracle.imresize(A, scale, antialias)
    assert a.shape == b.shape == tuple(int(np.ceil(n * scale)) for n in shape[:2]) + shape[2:]
    np.testing.assert_array_equal(a, b)


def _warps(M, N):
    """name -> warp (M x N x 2; plane 0 moves along the columns, 1 along the rows)."""
    z = lambda: np.zeros((M, N, 2), order="F")
    rng = np.random.default_rng(9)
    out = {"zero": z()}
    w = z()  # every sample exactly on column N: the min(floor, N - 1) clamp at fraction 1
    w[:, :, 0] = np.arange(1, N + 1)[None, :] - N
    out["on_last_column"] = w
    w = z()  # ... and exactly on row M
    w[:, :, 1] = np.arange(1, M + 1)[:, None] - M
    out["on_last_row"] = w
    w = z()  # both, in the corner sample
    w[:, :, 0] = np.arange(1, N + 1)[None, :] - N
    w[:, :, 1] = np.arange(1, M + 1)[:, None] - M
    out["on_last_corner"] = w
    w = z()  # one column further: the last column falls out of the frame
    w[:, :, 0] = -1.0
    out["one_column_out"] = w
    for name, plane, v in (("frame_left", 0, float(N)), ("frame_right", 0, -float(N)), ("frame_up", 1, float(M)),
                           ("frame_down", 1, -float(M))):
        w = z()  # a whole frame: everything is missing, filling leaves NaN
        w[:, :, plane] = v
        out[name] = w
    w = np.asfortranarray(rng.normal(scale=0.7, size=(M, N, 2)))
    w[0, 0, 0], w[M - 1, N - 1, 1], w[0, N - 1, 0], w[M - 1, 0, 1] = np.nan, np.nan, np.inf, -np.inf
    out["nan_inf_entries"] = w
    return out


def _frames(M, N):
    """name -> frame: a full one, and frames with NaN so that a filled line has
    a two-sided gap with a tie (odd gap: the middle goes to the later sample),
    runs that reach both ends, and an all-missing column beside a partly
    filled one."""
    V = np.asfortranarray(np.random.default_rng(4).random((M, N)) * 255)
    out = {"full": V}
    a = V.copy(order="F")
    a[0, 0] = np.nan
    out["corner_missing"] = a
    b = V.copy(order="F")
    b[:, 0] = np.nan            # an all-missing column: filled along the rows from column 1
    b[: max(1, M // 3), 1] = np.nan  # next to a partly filled one (a run from the top end)
    if M >= 7:
        b[1:4, N - 1] = np.nan  # a gap of three between rows 0 and 4: the tie at its middle
        b[M - 2:, N - 1] = np.nan   # and a run to the bottom end
    if N >= 7:
        b[M - 1, 2:7] = np.nan  # along a row: a gap of five (where the column fill cannot reach: M = 2)
    out["gaps"] = b
    c = V.copy(order="F")
    c[:, N - 1] = np.nan
    c[M - 1, :] = np.nan
    out["last_row_and_column_missing"] = c
    return out


@pytest.mark.parametrize("fill", [True, False])
@pytest.mark.parametrize("shape", [(2, 2), (2, 9), (9, 2), (7, 5)], ids=ids)
def test_warp_image_tiny_frames_bit_exact(shape, fill):
    from gqmap_opticalflow_amd import warp_image
    from oracle import oracle
    M, N = shape
    warps, frames = _warps(M, N), _frames(M, N)
    bad, all_nan, filled = [], 0, 0
    for wn, w in warps.items():
        for fn, V in frames.items():
            if fn != "full" and wn not in ("zero", "on_last_corner", "nan_inf_entries"):
                continue
            a, b = warp_image(V, w, fill), oracle.warp_image(V, w, fill)
            try:
                np.testing.assert_array_equal(a, b)  # NaN positions included
            except AssertionError:
                bad.append((wn, fn))
            all_nan += int(np.isnan(b).all())
            filled += int(fill and not np.isnan(b).any() and np.isnan(oracle.warp_image(V, w, False)).any())
    assert not bad, bad
    assert all_nan >= 4  # the whole-frame shifts leave nothing to fill from
    assert not fill or filled > 0
