"""The CPU references at degenerate grids: frames smaller than one tile, thin
strips, two interior rows or columns.

tests/test_gpu_small_grids.py holds the device to the CPU model of the kernel
(oracle/gqmap_emul.cpp) bit for bit at these shapes, so the model itself is
pinned here first: one step against the literal restatement
(oracle/gqmap_oracle.c) at the project's one-step gate (1e-10), 40 iterations
at every lanes-per-node count Q and both precisions that complete with a
finite trace and state, and exact sums that do not depend on the thread count.

Shapes are rows x cols of the image (the node grid of the single-pixel
engines; the super engine's nodes are a quarter of each side).  A 4 x 4 grid
has two interior rows and columns; every shape up to 15 x 15 is smaller than a
16 x 16 tile (Q = 1), 4 x 40 and 40 x 4 are one tile row / column at every Q
but 64, 17 x 17 and 33 x 16 leave a one-row (one-column) ragged edge."""
import dataclasses
import functools

import numpy as np
import pytest

from tests import _golden as G
from tests.test_gpu_parity import _gh, _oracle_state, _reference_init_case

S = [(4, 4), (4, 5), (5, 4), (8, 8), (4, 40), (40, 4), (5, 17), (17, 5), (15, 15), (16, 16), (17, 17), (33, 16)]
SSUP = [(12, 12), (12, 16), (16, 12), (12, 68), (68, 12)]
SPLITS = [1, 2, 4, 8, 16, 64, -1]  # -1: GQMAP_SPLIT_ROLE, a kernel shape with the Q = 1 arithmetic
SUPER_SPLITS = [1, 4, 16]
ENGINES = [("mixture", 1, 9), ("mixture", 3, 9), ("ctf", 1, 11)]
ITS = 40

ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None


@functools.lru_cache(maxsize=None)
def _small_case(engine, L, K, M, N, temperature, extra):
    name, r0, c0 = ("Urban3", 100, 120) if engine == "super" else ("rubberwhale", 150, 200)
    extra = dict(dict(alpha_start=10, t_decay_every=20), **dict(extra))
    I1, I2, _, _, o, st = _reference_init_case(name, M, N, r0, c0, L=L, K=K, engine=engine, **extra)
    if temperature is not None:
        o = dict(o, temperature=temperature)
        st = dataclasses.replace(st, T=temperature)
    return I1, I2, o, st


def small_case(engine, L, K, M, N, temperature=None, **extra):
    """The frames, options and seeded initial state of one small-grid case:
    RubberWhale cropped at (150, 200); the super engine takes Urban3 at
    (100, 120), the crop of tests/test_gpu_tiles.py.  alpha update from
    iteration 10, temperature decay every 20 (of the engine's own starting
    temperature, or the one given).  The frames are shared: read only."""
    I1, I2, o, st = _small_case(engine, L, K, M, N, temperature, tuple(sorted(extra.items())))
    return I1, I2, dict(o), st.copy()


def _finite(tr, ost):
    assert np.isfinite(tr).all()
    for k, a in zip(G.STATE_KEYS, ost.arrays()):
        assert np.isfinite(a).all(), k


@pytest.mark.parametrize("shape", S, ids=ids)
@pytest.mark.parametrize("engine,L,K", ENGINES)
def test_model_one_step_matches_literal_restatement(oracle_lib, engine, L, K, shape):
    I1, I2, o, st = small_case(engine, L, K, *shape)
    X, W = _gh(K)
    a, b = _oracle_state(st), _oracle_state(st)
    da, ta, _ = oracle_lib.emu_run(o, I1, I2, a, 1, 1, X, W, T=st.T, split=1)
    db, tb, _ = oracle_lib.run(o, I1, I2, b, 1, 1, T=st.T)
    assert da == db == 1
    np.testing.assert_allclose(ta, tb, rtol=1e-10, atol=1e-10)
    for k, x, y in zip(G.STATE_KEYS, a.arrays(), b.arrays()):
        np.testing.assert_allclose(x, y, rtol=1e-10, atol=1e-10, err_msg=k)


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("shape", S, ids=ids)
@pytest.mark.parametrize("engine,L,K", ENGINES)
def test_model_runs_every_split(oracle_lib, engine, L, K, shape, precision):
    X, W = _gh(K)
    role = None
    for split in SPLITS:
        I1, I2, o, st = small_case(engine, L, K, *shape, split=split)
        ost = _oracle_state(st)
        done, tr, _ = oracle_lib.emu_run(o, I1, I2, ost, 1, ITS, X, W, T=st.T, fp32=precision == "fp32")
        assert done == ITS, (split, done)
        _finite(tr, ost)
        if split == 1:
            role = (tr, ost)
    # the role split is the Q = 1 arithmetic (the last entry of SPLITS)
    np.testing.assert_array_equal(tr, role[0])
    for a, b in zip(ost.arrays(), role[1].arrays()):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("shape", SSUP, ids=ids)
@pytest.mark.parametrize("L", [3, 1])
def test_super_model_runs_every_split(oracle_lib, L, shape, precision):
    X, W = _gh(11)
    for split in SUPER_SPLITS:
        I1, I2, o, st = small_case("super", L, 11, *shape, split=split)
        assert st.muu.shape == (shape[0] // 4, shape[1] // 4, L)
        ost = _oracle_state(st)
        done, tr, _ = oracle_lib.emu_run(o, I1, I2, ost, 1, ITS, X, W, T=st.T, fp32=precision == "fp32")
        assert done == ITS, (split, done)
        _finite(tr, ost)


@pytest.mark.parametrize("shape", [(4, 4), (5, 17)], ids=ids)
@pytest.mark.parametrize("engine,L,K", ENGINES)
def test_model_sums_do_not_depend_on_thread_count(oracle_lib, engine, L, K, shape):
    I1, I2, o, st = small_case(engine, L, K, *shape, split=1)
    X, W = _gh(K)
    res = []
    for nt in (1, 3, 8):
        ost = _oracle_state(st)
        done, tr, _ = oracle_lib.emu_run(o, I1, I2, ost, 1, ITS, X, W, T=st.T, nthreads=nt)
        assert done == ITS
        res.append((tr, ost.arrays()))
    for tr, arrs in res[1:]:
        np.testing.assert_array_equal(tr, res[0][0])
        for a, b in zip(arrs, res[0][1]):
            np.testing.assert_array_equal(a, b)
