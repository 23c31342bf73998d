"""The CPU references over the accepted option range: L = 1..8, K = 2..16, every
lanes-per-node count Q (tests/_wide_options.py holds the table).

tests/test_gpu_wide_options.py holds the device to the CPU model of the kernel
(oracle/gqmap_emul.cpp) bit for bit over this table, so the model is pinned
here first: one step against the literal restatement (oracle/gqmap_oracle.c)
at the project's one-step gate (1e-10, tests/test_small_grids.py), and 40
iterations at every (case, Q, precision) that complete with a finite trace
and state.  Then the states the `if a ~= 0` guard is there for: mixture
weights that are exactly 0."""
import numpy as np
import pytest

from tests import _golden as G
from tests import _wide_options as WO
from tests.test_gpu_parity import _gh, _oracle_state


def _finite(tr, ost):
    assert np.isfinite(tr).all()
    for k, a in zip(G.STATE_KEYS, ost.arrays()):
        assert np.isfinite(a).all(), k


def _one_step_model_vs_literal(oracle_lib, I1, I2, o, st, it_first=1):
    X, W = _gh(o["K"])
    a, b = _oracle_state(st), _oracle_state(st)
    da, ta, _ = oracle_lib.emu_run(o, I1, I2, a, it_first, 1, X, W, T=st.T, split=1)
    db, tb, _ = oracle_lib.run(o, I1, I2, b, it_first, 1, T=st.T)
    assert da == db == 1
    np.testing.assert_allclose(ta, tb, rtol=1e-10, atol=1e-10)
    for k, x, y in zip(G.STATE_KEYS, a.arrays(), b.arrays()):
        np.testing.assert_allclose(x, y, rtol=1e-10, atol=1e-10, err_msg=k)
    return a, b


def test_frames_have_the_tiles_they_are_for():
    up = lambda a, b: -(-a // b)
    M, N = WO.nodes("mixture")
    assert (up(M, 16), up(N, 16), M - 2 * 16, N - 2 * 16) == (3, 3, 4, 10)  # the last tile row is grouped (<= 4 rows)
    for q in WO.ALL_SPLITS:
        tm, tn = WO.TILE[q]
        assert M % tm or N % tn, q               # a ragged edge
        assert up(M, tm) * up(N, tn) > 1, q      # more than one block
    Ms, Ns = WO.nodes("super")
    assert (Ms, Ns) == (12, 18)
    assert [(up(Ms, WO.TILE[q][0]), up(Ns, WO.TILE[q][1])) for q in WO.SUPER_SPLITS] == [(1, 2), (2, 3), (3, 5)]
    for q in WO.SUPER_SPLITS:
        assert Ms % WO.TILE[q][0] or Ns % WO.TILE[q][1], q


def test_table_covers_the_accepted_range():
    Ls = {L for _, L, _ in WO.CASES}
    Ks = {K for _, _, K in WO.CASES}
    assert {1, 2, 4, 5, 8} <= Ls and {2, 3, 4, 16} <= Ks and max(Ls) == 8 and max(Ks) == 16 and min(Ks) == 2
    for e in ("mixture", "ctf"):
        assert {q for x, L, K, q in WO.TABLE if (x, K) == (e, 16)} == set(WO.ALL_SPLITS)
        # lanes of a node without a sample: K^2 < Q
        assert {(K, q) for x, L, K, q in WO.TABLE if x == e and L == 1 and K * K < q} == \
            {(2, 8), (2, 16), (2, 64), (3, 16), (3, 64), (4, 64)}
        # every K = 2 and K = 3 case, whatever its L, runs at Q = 8, 16, 64
        for x, L, K in WO.CASES:
            if x == e and K <= 3:
                assert [q for y, l, k, q in WO.TABLE if (y, l, k) == (x, L, K)] == [8, 16, 64], (x, L, K)
    # ... with eight components: lanes without a sample beside the NFIX + 8 sums
    assert ("mixture", 8, 3, 16) in WO.TABLE and ("mixture", 8, 3, 64) in WO.TABLE and ("mixture", 8, 3, 8) in WO.TABLE
    assert {q for x, L, K, q in WO.TABLE if (x, L, K) == ("super", 8, 16)} == set(WO.SUPER_SPLITS)


@pytest.mark.parametrize("engine,L,K", WO.CASES)
def test_model_one_step_matches_literal_restatement(oracle_lib, engine, L, K):
    _one_step_model_vs_literal(oracle_lib, *WO.case(engine, L, K))


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("engine,L,K,split", WO.TABLE)
def test_model_runs_the_table(oracle_lib, engine, L, K, split, precision):
    I1, I2, o, st = WO.case(engine, L, K, split)
    X, W = _gh(K)
    ost = _oracle_state(st)
    done, tr, _ = oracle_lib.emu_run(o, I1, I2, ost, 1, WO.ITS, X, W, T=st.T, fp32=precision == "fp32")
    assert done == WO.ITS
    _finite(tr, ost)


@pytest.mark.parametrize("engine,L,guard_a", WO.ZERO_CASES)
def test_zero_weights_one_step_matches_literal_restatement(oracle_lib, engine, L, guard_a):
    # iteration 1 (gradients only) and iteration 11 (the first projsplx update: alpha_start = 10)
    I1, I2, o, st = WO.zero_weight_case(engine, L, guard_a, split=1)
    for it_first in (1, 11):
        a, b = _one_step_model_vs_literal(oracle_lib, I1, I2, o, st, it_first)
        _finite(np.zeros(1), a)
        _finite(np.zeros(1), b)


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("engine,L,guard_a", WO.ZERO_CASES)
def test_zero_weights_stay_zero(oracle_lib, engine, L, guard_a, precision):
    I1, I2, o, st = WO.zero_weight_case(engine, L, guard_a)
    zero = st.alpha == 0
    assert zero.sum() == L - 2
    X, W = _gh(WO.ZERO_K)
    ost = _oracle_state(st)
    done, tr, _ = oracle_lib.emu_run(o, I1, I2, ost, 1, WO.ITS, X, W, T=st.T, fp32=precision == "fp32")
    assert done == WO.ITS
    _finite(tr, ost)
    assert (ost.alpha[zero] == 0).all() and (ost.alpha[~zero] > 0).all()
    assert not np.array_equal(ost.alpha, st.alpha)  # the update ran


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_projsplx_drives_weights_to_zero_by_itself(oracle_lib, precision):
    # tests/test_gpu_wide_options.py compares the device with this run: without
    # a weight at exactly 0 it would never reach the guard's branch
    I1, I2, o, st = WO.zeroing_case()
    assert (st.alpha > 0).all()
    X, W = _gh(WO.ZEROING[2])
    ost = _oracle_state(st)
    done, tr, _ = oracle_lib.emu_run(o, I1, I2, ost, 1, WO.ITS, X, W, T=st.T, fp32=precision == "fp32")
    assert done == WO.ITS
    _finite(tr, ost)
    assert (ost.alpha == 0).sum() >= 1 and ost.alpha.sum() == pytest.approx(1.0, abs=1e-12)


@pytest.mark.parametrize("engine,L", [("mixture", 1), ("ctf", 1), ("super", 2)])
def test_two_point_rule_has_no_sigma_gradient(oracle_lib, engine, L):
    """Why the table carries K = 3 beside K = 2: with two Gauss-Hermite nodes
    (x = +-1/sqrt 2, equal weights) the quadrature's sigma gradient carries
    the factor x^2 - 1/2 = 0 at both nodes, so at temperature 0 sum|dsigma| of
    the literal restatement is rounding noise at every iteration and a K = 2
    case never moves sigma through the potentials.  What is left at K = 2 is
    the entropy term T / sigma alone (the single-scale engines reach
    T = t_min = 0.001 at the first decay, the super engine starts at 0.2),
    which does not depend on the frames.  So this test alone leaves the
    table's options: temperature 0 and no decay (with them sum|dsigma| is
    1e-3 for the mixture engine from iteration 20 on and 2e-2 for the super
    engine throughout; the ctf engine, t_min = 0, stays at 1e-15 either way).
    K = 3 is the smallest rule whose quadrature has a sigma gradient."""
    no_T = dict(temperature=0.0, t_decay_every=0)
    I1, I2, o, st = WO.case(engine, L, 2, **no_T)
    ost = _oracle_state(st)
    done, tr, _ = oracle_lib.run(o, I1, I2, ost, 1, WO.ITS, T=st.T)
    assert done == WO.ITS
    assert np.abs(tr[:, 2]).max() < 1e-12
    I1, I2, o, st = WO.case(engine, L, 3, **no_T)
    done, tr, _ = oracle_lib.run(o, I1, I2, _oracle_state(st), 1, 5, T=st.T)
    assert tr[:, 2].min() > 1e-6
