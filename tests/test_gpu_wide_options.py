"""Device parity over the accepted option range: L = 1..8, K = 2..16, H = 1..4,
every lanes-per-node count Q (the table of tests/_wide_options.py, whose CPU
side tests/test_wide_options.py pins first).

Every comparison with the CPU model of the kernel (oracle/gqmap_emul.cpp) is
bit for bit (assert_array_equal) on the trace, every state plane, w, alpha, it
and T.  What depends on L and K beyond the arithmetic: the finalize reductions
over NFIX + L sums, the super engine's L blocks (or dataflow items) per tile,
the softmax and projsplx updates over L weights, the `if a ~= 0` guard at
weights that are exactly 0, the K^2-point table copy in LDS (K = 16 fills it)
and lanes without a sample where K^2 < Q.

A. one launch per iteration against the model, the whole table;
B. the execution forms whose bookkeeping depends on L or K (dataflow items,
   persistent launch, replayed graphs) against one launch per iteration;
C. projsplx, weights at exactly 0;
D. state set-up at L = 8 and H = 4, map and log P."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import _wide_options as WO
from tests._blockmatch_gpu import as_fp32, assert_state_equal, flows
from tests.test_gpu_block_match_refine import widths
from tests.test_gpu_parity import _assert_bit_exact, _emulate, _policy
from tests.test_gpu_rolesplit import _shape
from tests.test_gpu_small_grids import _persist_off
from tests.test_small_grids import small_case

pytestmark = pytest.mark.gpu

PER_LAUNCH = dict(flow=0, persist=0, graph=0)
PRECISIONS = ["fp64", "fp32"]


@functools.lru_cache(maxsize=None)
def _model(engine, L, K, split, precision, its=WO.ITS, extra=()):
    """The CPU model's run of one table case (shared, left unchanged):
    (done, trace, T, state)."""
    I1, I2, o, st = WO.case(engine, L, K, split, **dict(extra))
    return _emulate(o, I1, I2, st, its, precision, None)


def _run(case, engine, precision, its, policy, flow=False, persist=False):
    """One run of a case (frames, options, state) by an engine created under
    `policy`: (done, trace, state).  Asserts the lanes per node and kernel
    shape asked for, the execution form, and that no launch was recovered
    through the per-launch fallback."""
    from gqmap_opticalflow_amd import Engine
    I1, I2, o, st = case
    split = o["split"]
    with _policy(**policy):
        eng = Engine(o, I1, I2, engine, precision)
    with eng:
        assert eng.info().split == (1 if split == WO.ROLE else split)
        assert _shape(eng) == (0 if split == WO.ROLE else split)
        assert eng.dataflow() == flow and eng.persistent() == persist
        eng.set_state(st.copy())
        done, tr = eng.run(its)
        g = eng.get_state()
        assert _persist_off(eng) == 0
    assert done == its and g.it == st.it + its
    return done, tr, g


def _equals_model(run, model):
    done, tr, g = run
    e_done, e_tr, e_T, ost = model
    _assert_bit_exact(g, tr, done, e_done, e_tr, ost)
    assert g.T == e_T


def _same(a, b):
    assert a[0] == b[0]
    np.testing.assert_array_equal(b[1], a[1])
    assert_state_equal(b[2], a[2])


# ---- A. per-launch kernels against the CPU model, the whole table -------------

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("engine,L,K,split", WO.TABLE)
def test_per_launch_bit_exact_vs_model(engine, L, K, split, precision):
    model = _model(engine, L, K, split, precision)
    assert model[0] == WO.ITS
    _equals_model(_run(WO.case(engine, L, K, split), engine, precision, WO.ITS, PER_LAUNCH), model)


# ---- B. execution forms against one launch per iteration ----------------------

def _form_case(engine, L, K, split, precision, its, policy, extra=None, model=True, **form):
    extra = extra or {}
    case = WO.case(engine, L, K, split, **extra)
    a = _run(case, engine, precision, its, PER_LAUNCH)
    b = _run(case, engine, precision, its, policy, **form)
    _same(a, b)
    if model:
        _equals_model(b, _model(engine, L, K, split, precision, its, tuple(sorted(extra.items()))))
    return b


@pytest.mark.parametrize("K", [4, 16])
def test_dataflow_mixture_pair_store(K):
    # integer-valued frames: the fp64 mixture engine at Q = 1 takes the binary16
    # pair store of the padded frame (tests/test_gpu_halo_chain.py); 3 x 3
    # tiles, the last tile row grouped; 40 iterations are launches of 32 and 8
    I1, I2, _, _ = WO.case("mixture", 1, K, 1)
    assert np.array_equal(I1, np.round(I1)) and np.array_equal(I2, np.round(I2))
    _form_case("mixture", 1, K, 1, "fp64", WO.ITS, dict(flow=1), flow=True)


def test_dataflow_ctf_full_table():
    _form_case("ctf", 1, 16, 1, "fp64", WO.ITS, dict(flow=1), flow=True)


@pytest.mark.parametrize("alpha_start", [10, 500])
@pytest.mark.parametrize("L,K", [(2, 5), (8, 16)])
def test_dataflow_super_items_per_component(L, K, alpha_start):
    # an item per (tile, component): nitems = ntiles * L, 2 x 3 tiles of 8 x 8
    # at Q = 4.  alpha_start = 10: alpha moves from iteration 11 on, an item
    # waits for the finalize of the iteration before; 500: it never moves in
    # this run, the other lag of flow_wait
    _form_case("super", L, K, 4, "fp64", WO.ITS, dict(flow=1), dict(alpha_start=alpha_start), flow=True)


@pytest.mark.parametrize("alpha_start", [10, 500])
@pytest.mark.parametrize("L,K", [(2, 5), (8, 16)])
def test_super_at_one_lane_per_node_is_not_a_dataflow_launch(L, K, alpha_start):
    # the super item exists at Q = 4 only (launch_flow_t): at Q = 1 a forced
    # flow policy leaves the replayed graphs of L blocks per tile, which must
    # equal one launch per iteration and the model
    _form_case("super", L, K, 1, "fp64", 61, dict(flow=1), dict(alpha_start=alpha_start), flow=False)


PERSIST_FRAME = (18, 13)  # Q = 16: 5 x 4 tiles of 4 x 4; Q = 64: 4 x 13 tiles of 5 x 1; ragged at both


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("split", [16, 64])
@pytest.mark.parametrize("K", [16, 3])
def test_persistent_launch_bit_exact_vs_model(K, split, precision):
    # 61 iterations: a replayed chunk of 50 and a leftover launch of 11, with
    # a temperature that decays inside both
    M, N = PERSIST_FRAME
    tm, tn = WO.TILE[split]
    assert M % tm and (N % tn or tn == 1) and -(-M // tm) * -(-N // tn) + 1 <= 64
    case = small_case("ctf", 1, K, M, N, temperature=0.3, split=split)
    a = _run(case, "ctf", precision, 61, PER_LAUNCH)
    b = _run(case, "ctf", precision, 61, {}, persist=True)
    _same(a, b)
    _equals_model(b, _emulate(case[2], case[0], case[1], case[3], 61, precision, None))


def test_graph_replay_eight_components():
    # 133 iterations: two replayed 50-iteration graphs and a leftover of 33.
    # The library has no accessor for the graph state; gqmap_run replays graphs
    # whenever the context's policy graph is on (the default) and returns a
    # failed capture as an error, never as one launch per iteration
    b = _form_case("mixture", 8, 16, 1, "fp64", 133, {}, model=False)
    np.testing.assert_array_equal(b[1][:WO.ITS], _model("mixture", 8, 16, 1, "fp64")[1])


# ---- C. alpha updates -----------------------------------------------------------

FORMS = [("per_launch", PER_LAUNCH), ("default", {})]


@pytest.mark.parametrize("form,policy", FORMS)
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("engine,L,K,split", [("mixture", 8, 16, 1), ("super", 8, 3, 16)])
def test_projsplx_eight_components_bit_exact_vs_model(engine, L, K, split, precision, form, policy):
    extra = dict(alpha_mode=1)
    model = _model(engine, L, K, split, precision, WO.ITS, tuple(extra.items()))
    got = _run(WO.case(engine, L, K, split, **extra), engine, precision, WO.ITS, policy)
    _equals_model(got, model)
    assert not np.array_equal(got[2].alpha, WO.case(engine, L, K, split)[3].alpha)


@functools.lru_cache(maxsize=None)
def _zero_model(engine, L, guard_a, precision):
    I1, I2, o, st = WO.zero_weight_case(engine, L, guard_a)
    return _emulate(o, I1, I2, st, WO.ITS, precision, None)


@pytest.mark.parametrize("form,policy", FORMS)
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("engine,L,guard_a", WO.ZERO_CASES)
def test_zero_weights_bit_exact_vs_model(engine, L, guard_a, precision, form, policy):
    case = WO.zero_weight_case(engine, L, guard_a)
    zero = case[3].alpha == 0
    assert zero.sum() == L - 2
    got = _run(case, engine, precision, WO.ITS, policy)
    assert np.isfinite(got[1]).all()
    assert (got[2].alpha[zero] == 0).all() and (got[2].alpha[~zero] > 0).all()
    _equals_model(got, _zero_model(engine, L, guard_a, precision))


@functools.lru_cache(maxsize=None)
def _zeroing_model(precision):
    I1, I2, o, st = WO.zeroing_case()
    return _emulate(o, I1, I2, st, WO.ITS, precision, None)


@pytest.mark.parametrize("form,policy", FORMS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_weights_driven_to_zero_bit_exact_vs_model(precision, form, policy):
    # (that the model reaches a weight of exactly 0: tests/test_wide_options.py)
    model = _zeroing_model(precision)
    assert (model[3].alpha == 0).any()
    got = _run(WO.zeroing_case(), WO.ZEROING[0], precision, WO.ITS, policy)
    _equals_model(got, model)
    np.testing.assert_array_equal(got[2].alpha == 0, model[3].alpha == 0)


# ---- D. state set-up at wide L ------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("engine", ["mixture", "super"])
def test_device_init_equals_host_init_eight_components(engine, precision):
    from gqmap_opticalflow_amd import Engine, initial_state
    I1, I2, o, _ = WO.case(engine, 8, 4)
    M, N = WO.nodes(engine)
    with Engine(o, I1, I2, engine, precision) as eng:
        assert (eng.M, eng.N, eng.L) == (M, N, 8)
        eng.init_state(seed=11)
        got = eng.get_state()
    want = initial_state(o, M, N, seed=11, engine=engine)
    assert_state_equal(got, as_fp32(want) if precision == "fp32" else want, "init")
    assert got.alpha.shape == (8,) and got.alpha.sum() == pytest.approx(1.0, abs=1e-15)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("L", [4, 8])
@pytest.mark.parametrize("engine", ["mixture", "super"])
def test_four_hypotheses_equal_the_host_formula(engine, L, precision):
    # H = GQ_BM_HMAX = 4 needs L >= 4: gqmap_init_state_flows and, with widths,
    # gqmap_init_state_seeded; components l >= 4 keep the plain draw
    from gqmap_opticalflow_amd import Engine, initial_state
    I1, I2, o, _ = WO.case(engine, L, 4)
    M, N = WO.nodes(engine)
    f, s = flows(M, N, 4, seed=11), widths(M, N, 4, 13, o)
    with Engine(o, I1, I2, engine, precision) as e:
        e.init_state_from_flow(f, seed=7, sigma=s)
        seeded = e.get_state()
        e.init_state_from_flow(f, seed=7)
        flowed = e.get_state()
        e.init_state(7)
        plain = e.get_state()
    fp = (lambda st: as_fp32(st)) if precision == "fp32" else (lambda st: st)
    assert_state_equal(seeded, fp(initial_state(o, M, N, seed=7, engine=engine, flow=f, sigma=s)), "seeded init")
    assert_state_equal(flowed, fp(initial_state(o, M, N, seed=7, engine=engine, flow=f)), "flows init")
    assert_state_equal(plain, fp(initial_state(o, M, N, seed=7, engine=engine)), "plain init")
    for l in range(L):
        for k in ("muu", "muv", "sigu", "sigv"):
            same = np.array_equal(getattr(seeded, k)[:, :, l], getattr(plain, k)[:, :, l])
            assert same == (l >= 4), f"{k} component {l}"
        assert np.array_equal(flowed.sigu[:, :, l], plain.sigu[:, :, l])
        assert np.array_equal(flowed.muu[:, :, l], plain.muu[:, :, l]) == (l >= 4)


def test_five_hypotheses_are_refused():
    from gqmap_opticalflow_amd import Engine
    I1, I2, o, _ = WO.case("mixture", 8, 4)
    M, N = WO.nodes("mixture")
    D = C.POINTER(C.c_double)
    with Engine(o, I1, I2) as e:
        e.init_state(2)
        before = e.get_state()
        f = np.zeros((M, N, 2, 5), order="F")
        s = np.ones((M, N, 2, 5), order="F")
        assert e.lib.gqmap_init_state_flows(e.ctx, f.ctypes.data_as(D), 5, C.c_uint64(3)) == 1  # GQMAP_ERR_INVALID_ARG
        assert b"gqmap_init_state_flows" in e.lib.gqmap_last_error()
        assert e.lib.gqmap_init_state_seeded(e.ctx, f.ctypes.data_as(D), s.ctypes.data_as(D), 5, C.c_uint64(3)) == 1
        assert b"gqmap_init_state_seeded" in e.lib.gqmap_last_error()
        assert_state_equal(e.get_state(), before, "nothing written")


@pytest.mark.parametrize("engine", ["mixture", "super"])
def test_map_and_logp_eight_components(engine):
    # (the references of test_engine_map_and_logp and tests/test_gpu_logp.py)
    from gqmap_opticalflow_amd import Engine
    from oracle import oracle
    I1, I2, o, st = WO.case(engine, 8, 4)
    with Engine(o, I1, I2, engine) as eng:
        eng.set_state(st.copy())
        assert eng.run(WO.ITS)[0] == WO.ITS
        mp = eng.map()
        g = eng.get_state()
        lp = eng.log_p(mp)
    assert np.isfinite(mp).all()
    np.testing.assert_array_equal(mp, oracle.get_map(g.alpha, g.muu, g.sigu, g.muv, g.sigv, det_exp=True))
    ref = oracle.log_p(o, I1, I2, mp)
    assert np.isfinite(lp) and lp == pytest.approx(ref, rel=1e-10), (lp, ref)
