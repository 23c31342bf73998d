"""The ops that turn a converged state into the answer, at their edges:
k_mixture_map (gqmap_mixture_map, Engine.map), k_logp (Engine.log_p),
k_projsplx and k_flow_range / k_flow_color.

Each is held bit for bit to its C restatement (oracle/gqmap_oracle.c) on the
seeded inputs of tests/_result_ops_np.py, and -- because the restatement is a
twin of the kernel -- to a reference that shares no code with either: the MAP
properties P1..P3, the longdouble projection.  tests/test_result_ops.py holds
the restatement to the same references on the CPU and shows the property
checker rejecting wrong maps.

k_logp has eight instantiations; the test that reaches each one asserts the
frame store it ran on (gqmap_debug_vv_store):
  <double, vvh2_t, false>  test_logp_every_frame_store_same_bits (vv_pair = 1)
  <double, vvs_t,  false>  test_logp_fp64_vs_restatement[mixture-*], ..._same_bits (vv_pair = 0)
  <double, double, false>  test_logp_fp64_vs_restatement[ctf-*], ..._same_bits (vv_float = 0)
  <double, vvs_t,  true>   test_logp_fp64_vs_restatement[super-*], test_logp_super_frame_stores_same_bits
  <double, double, true>   test_logp_super_frame_stores_same_bits (vv_float = 0)
  <float,  float,  false>  test_logp_fp32_within_derived_bound[mixture-*]
  <float,  vvh2_t, false>  test_logp_fp32_within_derived_bound[mixture_pair-37x29]
  <float,  float,  true>   test_logp_fp32_within_derived_bound[super-*]
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import _result_ops_np as R
from tests.test_gpu_parity import _policy, _reference_init_case
from tests.test_result_ops import assert_map_properties, restated_projsplx
from tests.test_small_grids import ids, small_case

pytestmark = pytest.mark.gpu

STORES = {0: "double", 1: "float", 2: "pair"}


def _store(eng):
    f = eng.lib.gqmap_debug_vv_store
    f.restype, f.argtypes = C.c_int, [C.c_void_p]
    return STORES[f(eng.ctx)]


# ---- mixture MAP ---------------------------------------------------------------------------

def _device_map(fam):
    from gqmap_opticalflow_amd import mixture_map
    return mixture_map(fam["alpha"], fam["muu"], fam["sigu"], fam["muv"], fam["sigv"])


def _restated_map(fam):
    from oracle import oracle
    return oracle.get_map(fam["alpha"], fam["muu"], fam["sigu"], fam["muv"], fam["sigv"], det_exp=True)


@pytest.mark.parametrize("name", R.FAMILIES)
def test_mixture_map_families(name):
    # L = 1, 2, 3, 4, 5, 8 (GQMAP_LMAX); MN = 1073, no multiple of the block
    fam = R.FAMILIES[name]()
    g = _device_map(fam)
    np.testing.assert_array_equal(g, _restated_map(fam))
    assert_map_properties(g, fam, name)
    if name in R.EXACT:
        np.testing.assert_array_equal(g, R.exact_answer(name))
    if name == "sym_pair":
        c = R.sym_pair_centre(fam)
        assert np.all(np.abs(g - c) <= 3.0 * R.tol1(c)), np.abs(g - c).max()


@pytest.mark.parametrize("shape", R.CROPS, ids=ids)
def test_mixture_map_shapes(shape):
    # one pixel, one row, one column, exactly one block, one block and two pixels
    fam = R.crop(R.random(3), *shape)
    g = _device_map(fam)
    assert g.shape == shape + (2,)
    np.testing.assert_array_equal(g, _restated_map(fam))
    assert_map_properties(g, fam, ids(shape))


def engine_map_case(engine):
    """A 48 x 64 RubberWhale crop, L = 3, and a "tight" state on its node grid
    built as tests/_fullsize.py builds one: means around the ground truth,
    widths in [0.2, 1.7], correlations in [-0.4, 0.4]."""
    from gqmap_opticalflow_amd import State
    sup = engine == "super"
    I1, I2, flo, _, o, st = _reference_init_case("rubberwhale", 48, 64, 150, 200, L=3, K=11 if sup else 9,
                                                 engine=engine)
    rng = np.random.default_rng(100)
    f = 4 if sup else 1
    sh = st.muu.shape
    gu = flo[f // 2::f, f // 2::f, 0][:sh[0], :sh[1]]
    gv = flo[f // 2::f, f // 2::f, 1][:sh[0], :sh[1]]
    tight = State(
        muu=np.asfortranarray(np.clip(gu[:, :, None] + rng.normal(0, 0.5, sh), o["minu"], o["maxu"])),
        muv=np.asfortranarray(np.clip(gv[:, :, None] + rng.normal(0, 0.5, sh), o["minv"], o["maxv"])),
        sigu=np.asfortranarray(0.2 + 1.5 * rng.random(sh)), sigv=np.asfortranarray(0.2 + 1.5 * rng.random(sh)),
        pn=np.asfortranarray(0.8 * (rng.random(sh) - 0.5)), rou=np.asfortranarray(0.8 * (rng.random(sh + (2, 2)) - 0.5)),
        w=st.w, alpha=st.alpha, it=st.it, T=st.T)
    return I1, I2, o, tight


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("engine", ["mixture", "super"])
def test_engine_map_of_its_own_state(engine, precision):
    # Engine.map() reads the engine's state planes in the engine's precision:
    # k_mixture_map<float> (fp32; nothing else runs it) and <double>, the
    # super engine on its M/4 x N/4 node grid
    from gqmap_opticalflow_amd import Engine
    I1, I2, o, tight = engine_map_case(engine)
    with Engine(o, I1, I2, engine, precision) as eng:
        eng.set_state(tight)
        done, _ = eng.run(5)
        assert done == 5
        mp = eng.map()
        st = eng.get_state()
    assert mp.shape == ((12, 16, 2) if engine == "super" else (48, 64, 2))
    if precision == "fp32":  # the state the map was taken from is float
        assert all(np.array_equal(getattr(st, k), getattr(st, k).astype(np.float32)) for k in ("muu", "muv", "sigu", "sigv"))
    fam = R.state_family(st)
    np.testing.assert_array_equal(mp, _restated_map(fam))
    assert_map_properties(mp, fam, f"{engine} {precision}")


# ---- log P -------------------------------------------------------------------------------------

LOGP_FRAMES = {
    # 4 x 4: the interior is 2 x 2; 4 x 65 stands for 3 x 86 (MN = 260: one block and four nodes), since the
    # library takes no frame under 4 rows
    "mixture": [(4, 4), (5, 17), (16, 16), (4, 65), (37, 29)],
    "ctf": [(4, 4), (5, 17), (16, 16), (4, 65), (37, 29)],
    # node grids 3 x 3, 3 x 4, 4 x 3 (the smallest the engine takes: one interior node) and 9 x 7
    "super": [(12, 12), (12, 16), (16, 12), (36, 28)],
}
LOGP_CASES = [(e, s) for e, shapes in LOGP_FRAMES.items() for s in shapes]
logp_id = lambda v: ids(v) if isinstance(v, tuple) else v


def _frames(engine, shape, **extra):
    """Frames and options of tests/test_small_grids.py: RubberWhale (the super engine: Urban3) crops,
    integer-valued; the ctf engine's are scaled by 0.7, so no float holds them."""
    I1, I2, o, st = small_case(engine, 1, 9 if engine == "mixture" else 11, *shape, **extra)
    return I1, I2, o, st.muu.shape[:2]


def _maps(grid):
    """Two maps on a node grid: uniform in +-6, which crosses the border
    clamps, and the smooth ramp of tests/test_oracle.py."""
    m, n = grid
    rng = np.random.default_rng(7 + 100 * m + n)
    ramp = np.stack(np.meshgrid(np.linspace(-1, 2, n), np.linspace(0.5, -1.5, m)), axis=2)
    return {"uniform": np.asfortranarray(rng.uniform(-6, 6, size=(m, n, 2))), "ramp": np.asfortranarray(ramp)}


@pytest.mark.parametrize("engine,shape", LOGP_CASES, ids=logp_id)
def test_logp_fp64_vs_restatement(engine, shape):
    """oracle.log_p takes the ctf engine's options (make_params knows the
    engine; profile_logP is node_pot's bicubic whatever the engine iterates
    with), so ctf is a case like the others: its frames are not integers and
    take the double store."""
    from gqmap_opticalflow_amd import Engine
    from oracle import oracle
    I1, I2, o, grid = _frames(engine, shape)
    with Engine(o, I1, I2, engine, "fp64") as eng:
        assert _store(eng) == ("double" if engine == "ctf" else "float")
        for kind, mp in _maps(grid).items():
            lp, ref = eng.log_p(mp), oracle.log_p(o, I1, I2, mp)
            print(f"{engine} {ids(shape)} {kind}: log P {lp!r}, restatement {ref!r}")
            assert np.isfinite(lp) and lp < 0
            assert lp == pytest.approx(ref, rel=1e-10), (kind, lp, ref)


def _logp_under(policies, engine, shape, **extra):
    """log P of the same map on the same frames under each policy: [(store, value)], and the restatement's."""
    from gqmap_opticalflow_amd import Engine
    from oracle import oracle
    I1, I2, o, grid = _frames(engine, shape, **extra)
    assert np.array_equal(I1, np.round(I1)) and np.array_equal(I2, np.round(I2))  # every store holds them exactly
    mp = _maps(grid)["uniform"]
    out = []
    for pol in policies:
        with _policy(**pol):
            eng = Engine(o, I1, I2, engine, "fp64")
        with eng:
            out.append((_store(eng), eng.log_p(mp)))
    return out, oracle.log_p(o, I1, I2, mp)


def test_logp_every_frame_store_same_bits():
    # binary16 column pairs (one lane per node), float, double: the stores are
    # exact and sample() converts a tap before it enters the same fma chain,
    # so the policy changes no bit
    got, ref = _logp_under([dict(vv_pair=1), dict(vv_pair=0), dict(vv_float=0)], "mixture", (37, 29), split=1)
    assert [s for s, _ in got] == ["pair", "float", "double"]
    assert got[0][1] == got[1][1] == got[2][1], got
    assert got[0][1] == pytest.approx(ref, rel=1e-10)


def test_logp_super_frame_stores_same_bits():
    got, ref = _logp_under([dict(vv_float=1), dict(vv_float=0)], "super", (36, 28))
    assert [s for s, _ in got] == ["float", "double"]
    assert got[0][1] == got[1][1], got
    assert got[0][1] == pytest.approx(ref, rel=1e-10)


ROUNDINGS = 87


def logp_fp32_bound(o, I2, mp, grid, sup):
    """|log P (fp32) - log P (fp64)| on a map that is exact in float.

    Every term is -lambda sqrt(eps + d^2), 1-Lipschitz in d, so the error of
    the sum is at most lambda times the summed errors of the d:
      data   d = I1 - Vq.  The literal expression (oracle/gqmap_oracle.c
             node_pot, orc_interp_cubic) rounds 87 times on the way to d:
             j + x1 and i + x2 (2), so and to (2), the Keys weights t0..t3
             (4 + 5 + 5 + 3 = 17) and the four forms of ss (17), sixteen
             products c * ss * t (32) and the fifteen additions of Vq (15),
             Vq / 4 (1) and the subtraction (1).  Each is off by at most 2^-24
             of a value no larger than 2 Imax (the weights of an axis sum to
             at most 2.5 in absolute value, before the / 4), Imax the largest
             absolute padded-frame value: R = 2 x 87 = 174;
      edges  four per interior node (two planes, two directions), each off by
             at most 2^-24 x 4 max|map|.
    The frames are integers, exact in float; the sums run in double."""
    from oracle import oracle
    m, n = grid
    n_int = (m - 2) * (n - 2)
    n_data = n_int * (16 if sup else 1)
    imax = float(np.abs(oracle.get_vv(I2)).max())
    return 2.0 ** -24 * (o["lambdad"] * n_data * 2 * ROUNDINGS * imax
                         + o["lambdas"] * 4 * n_int * 4 * float(np.abs(mp).max()))


@pytest.mark.parametrize("engine,shape", [("mixture", (37, 29)), ("mixture", (5, 17)), ("mixture_pair", (37, 29)),
                                          ("super", (36, 28)), ("super", (12, 12))], ids=logp_id)
def test_logp_fp32_within_derived_bound(engine, shape):
    """The bound (logp_fp32_bound) is 1e-5 .. 5e-4 of |log P|: enough to catch
    a dropped row, a wrong neighbour or a missing term; the sharp check is the
    fp64 one.  |delta| / bound measured on an MI355X (uniform map, ramp):
      mixture 37x29       1.2e-4, 6.3e-6     mixture 5x17   1.5e-4, 1.1e-5
      mixture 37x29 pair  1.2e-4, 6.3e-6     (the float store's values, bit for bit)
      super 36x28         4.7e-4, 5.6e-6     super 12x12    3.3e-3, 7.6e-7"""
    from gqmap_opticalflow_amd import Engine
    from oracle import oracle
    pair = engine == "mixture_pair"  # one lane per node: the fp32 engine keeps the pair store as well
    engine = "mixture" if pair else engine
    I1, I2, o, grid = _frames(engine, shape, **(dict(split=1) if pair else {}))
    assert np.array_equal(I1, np.round(I1)) and np.array_equal(I2, np.round(I2))
    with Engine(o, I1, I2, engine, "fp32") as eng:
        assert _store(eng) == ("pair" if pair else "float")
        for kind, mp in _maps(grid).items():
            mp = np.asfortranarray(mp.astype(np.float32).astype(np.float64))  # input rounding is common to both
            lp, ref = eng.log_p(mp), oracle.log_p(o, I1, I2, mp)
            bound = logp_fp32_bound(o, I2, mp, grid, engine == "super")
            print(f"fp32 {engine}{' pair' if pair else ''} {ids(shape)} {kind}: |delta| / bound = "
                  f"{abs(lp - ref) / bound:.4g} (log P {ref:.6e}, bound {bound:.3e} = {bound / abs(ref):.2e} |log P|)")
            assert abs(lp - ref) <= bound, (kind, lp, ref, bound)


# ---- projsplx ------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", R.PROJ_N)
def test_projsplx_every_column(n):
    # n = 64 fills the kernel's private array (PROJ_NMAX); ncols around one block
    from gqmap_opticalflow_amd import projsplx
    worst = [0.0, 0.0]
    for kind in R.PROJ_KINDS:
        Y, ref = R.proj_input(n, kind), restated_projsplx(n, kind)
        for ncols in R.PROJ_NCOLS:
            Yc = np.asfortranarray(Y[:, :ncols])
            X = projsplx(Yc)
            assert X.shape == (n, ncols)
            np.testing.assert_array_equal(X, ref[:, :ncols], err_msg=f"{kind} n={n} ncols={ncols}")
            e, s = R.check_projection(X, Yc)
            worst = [max(worst[0], e), max(worst[1], s)]
    print(f"projsplx n={n}: error / bound {worst[0]:.3g}, |sum - 1| / bound {worst[1]:.3g}")
    y = np.array(R.proj_input(n, "normal")[:, 0])  # the vector form
    np.testing.assert_array_equal(projsplx(y), restated_projsplx(n, "normal")[:, 0])


def test_projsplx_rejects_sizes_outside_the_private_array():
    from gqmap_opticalflow_amd import _lib, projsplx
    for n in (65, 0):
        with pytest.raises(_lib.GqmapError):
            projsplx(np.zeros((n, 3), order="F"))
    X = projsplx(np.zeros((5, 0), order="F"))
    assert X.shape == (5, 0) and X.size == 0


# ---- flow colour -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", R.flow_cases())
def test_flow_to_color_vs_restatement(name):
    from gqmap_opticalflow_amd import flow_to_color
    from oracle import oracle
    flow, max_flow = R.flow_cases()[name]
    img, flo, stats, unk = flow_to_color(flow, max_flow)
    rimg, rflo, rstats, runk = oracle.flow_to_color(flow, max_flow)
    np.testing.assert_array_equal(flo, rflo)  # (NaNs compare equal here)
    np.testing.assert_array_equal(unk, runk)
    np.testing.assert_array_equal(np.array(stats), rstats)
    # img goes through the device's atan2: expected equal; where it is not, one level on 1e-4 of the pixels at most
    diff = np.abs(img.astype(np.int16) - rimg.astype(np.int16))
    bad = int((diff.max(axis=2) > 0).sum())
    print(f"flow colour {name}: {bad} of {diff.shape[0] * diff.shape[1]} pixels differ from the restatement")
    assert diff.max() <= 1, np.argwhere(diff > 1)[0]
    assert bad <= 1e-4 * diff.shape[0] * diff.shape[1]
