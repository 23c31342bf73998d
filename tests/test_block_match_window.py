"""Per-pixel search windows and the coarse-to-fine matcher, host models
(gqmap_block_match_window_host, gqmap_block_match_pyramid_host) against the
numpy restatement of tests/_blockmatch_window_np.py, bit for bit; the anchor
(a constant box is the existing matcher); the quality of the pyramid against
the full search on whole frames; block_match_init(levels=).  No device."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import _blockmatch_np as R
from tests import _blockmatch_window_np as W
from tests import _codeobj

NAN_BITS = 0x7FF8000000000000
CROP_97 = "97x130"


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def assert_bit_equal(got, want, names=("flow", "cost", "curv")):
    assert len(got) == len(want)
    for g, w, what in zip(got, want, names):
        assert g.shape == w.shape, what
        diff = bits(g) != bits(w)
        assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} entries differ"


def frames(crop):
    return W.pair_97x130() if crop == CROP_97 else R.crop_pair(crop)


@functools.lru_cache(maxsize=None)
def model(crop, params, kind, subpixel):
    from gqmap_opticalflow_amd import block_match_window
    out = block_match_window(*R.crop_pair(crop), W.windows(crop, params, kind), params[2], params[3], subpixel=subpixel,
                             host=True)
    for a in out:
        a.setflags(write=False)
    return out


# ---- the window matcher ------------------------------------------------------------------------

@pytest.mark.parametrize("subpixel", [False, True], ids=["integer", "subpixel"])
@pytest.mark.parametrize("kind", W.KINDS)
@pytest.mark.parametrize("params", R.PARAMS[:3], ids=str)
@pytest.mark.parametrize("crop", R.CROPS, ids=str)
def test_host_model_equals_restatement_bit_for_bit(crop, params, kind, subpixel):
    got = model(crop, params, kind, subpixel)
    want = W.reference(crop, params, kind, subpixel)
    assert len(got) == (3 if subpixel else 2)
    assert_bit_equal(got, want[:len(got)])


@pytest.mark.parametrize("crop", R.CROPS, ids=str)
def test_the_windows_of_every_kind_are_there(crop):
    """What the generator promises, and what the matcher makes of each."""
    par = R.PARAMS[0]
    _, _, M, N = crop
    win = W.windows(crop, par, "mixed")
    flow, cost, curv = model(crop, par, "mixed", True)
    empty = (win[:, :, 0] > win[:, :, 1]) | (win[:, :, 2] > win[:, :, 3])
    assert empty[0, 0] and empty[M // 2, N // 2] and empty.sum() == 2
    assert np.all(bits(flow[empty]) == NAN_BITS) and np.all(np.isposinf(cost[empty])) and np.all(curv[empty] == 0)
    assert not np.isnan(flow[~empty]).any() and np.all(np.isfinite(cost[~empty]))
    # one displacement: the flow is its negative, nothing to refine
    assert tuple(flow[M - 1, N - 1]) == (1.0, -2.0) and tuple(curv[M - 1, N - 1]) == (0.0, 0.0)
    # wholly off the frame: B is zero, every cost ties, the first in ascending (dv, du) wins
    assert tuple(win[1, 2]) == (M + 4, M + 6, -1, 1) and tuple(flow[1, 2]) == (1.0, -(M + 4.0))
    assert tuple(flow[M - 2, 1]) == (N + 9.0, 1.0) and tuple(curv[1, 2]) == (0.0, 0.0)
    # inside its own box, within half a pixel of an integer
    f, w = flow[~empty], win[~empty]
    assert np.all(-f[:, 1] >= w[:, 0] - 0.5) and np.all(-f[:, 1] <= w[:, 1] + 0.5)
    assert np.all(-f[:, 0] >= w[:, 2] - 0.5) and np.all(-f[:, 0] <= w[:, 3] + 0.5)
    assert np.any(curv > 0)
    halves = W.windows(crop, par, "halves")
    assert np.all(halves[:, N // 2:, 2] - halves[:, :N // 2, 3].max() == 40)
    hflow = model(crop, par, "halves", False)[0]
    assert np.all(hflow[:, :N // 2, 0] >= 20) and np.all(hflow[:, N // 2:, 0] <= -20)


@pytest.mark.parametrize("params", R.PARAMS, ids=str)
@pytest.mark.parametrize("crop", R.CROPS[2:], ids=str)
def test_a_constant_box_is_the_plain_matcher(crop, params):
    """The anchor: flow and cost of block_match, and flow, cost and curv of
    block_match(subpixel=True) at one hypothesis, bit for bit."""
    from gqmap_opticalflow_amd import block_match, block_match_window
    A, B = R.crop_pair(crop)
    U, V, ft, sigma = params
    win = W.constant_window(*A.shape, U, V)
    assert_bit_equal(block_match_window(A, B, win, ft, sigma, host=True), block_match(A, B, *params, host=True))
    fine = block_match(A, B, *params, host=True, subpixel=True)
    assert_bit_equal(block_match_window(A, B, win, ft, sigma, subpixel=True, host=True), [a[..., 0] for a in fine])


def test_nan_frames_name_the_first_displacement_of_the_box():
    """bm_keep_allowed's rule for costs that are never < best, here without a
    scan order: the smallest (dv, du) of the box, cost +Inf, as block_match."""
    from gqmap_opticalflow_amd import block_match, block_match_window
    A = np.full((6, 5), np.nan, order="F")
    flow, cost = block_match_window(A, A, W.constant_window(6, 5, 2, 1), 1, 1.0, host=True)
    assert_bit_equal((flow, cost), block_match(A, A, 2, 1, 1, 1.0, host=True))
    assert np.all(flow[:, :, 0] == 1) and np.all(flow[:, :, 1] == 2) and np.all(np.isposinf(cost))


@pytest.mark.parametrize("kw", [dict(ft=5), dict(sigma=0.0), dict(M=0), dict(bound=2049), dict(bound=-2049)], ids=str)
@pytest.mark.parametrize("entry", ["gqmap_block_match_window_host", "gqmap_block_match_window"])
def test_window_argument_errors_write_nothing(entry, kw):
    from gqmap_opticalflow_amd import _lib
    lib = _lib.load()
    a = dict(ft=1, sigma=1.0, M=4, bound=1)
    a.update(kw)
    A = np.zeros((4, 4), order="F")
    win = W.constant_window(4, 4, 1, 1)
    win[2, 3, 1] = a["bound"]
    flow, cost, curv = (np.full(s, 77.0, order="F") for s in ((4, 4, 2), (4, 4), (4, 4, 2)))
    ms = C.c_double(-1.0)
    args = [_lib.dptr(A), _lib.dptr(A), win.ctypes.data_as(C.POINTER(C.c_int)), a["M"], 4, a["ft"], a["sigma"], 1,
            _lib.dptr(flow), _lib.dptr(cost), _lib.dptr(curv)]
    if entry == "gqmap_block_match_window":
        args += [C.cast(C.byref(ms), _lib._D), 0]
    assert getattr(lib, entry)(*args) == 1  # GQMAP_ERR_INVALID_ARG
    assert entry.encode() in lib.gqmap_last_error()
    assert np.all(flow == 77.0) and np.all(cost == 77.0) and np.all(curv == 77.0) and ms.value == -1.0


@pytest.mark.parametrize("kw", [dict(levels=0), dict(levels=7), dict(r=5), dict(r=-1), dict(k=3), dict(U=65), dict(V=66),
                                dict(ft=5), dict(sigma=-1.0), dict(M=0)], ids=str)
@pytest.mark.parametrize("entry", ["gqmap_block_match_pyramid_host", "gqmap_block_match_pyramid"])
def test_pyramid_argument_errors_write_nothing(entry, kw):
    """levels = 2 halves U once: 64 is allowed, 65 is not."""
    from gqmap_opticalflow_amd import _lib
    lib = _lib.load()
    a = dict(levels=2, r=1, k=1, U=64, V=2, ft=1, sigma=1.0, M=4)
    A = np.zeros((4, 4), order="F")
    flow, cost, curv = (np.full(s, 77.0, order="F") for s in ((4, 4, 2), (4, 4), (4, 4, 2)))

    def call(a):
        ms = C.c_double(-1.0)
        args = [_lib.dptr(A), _lib.dptr(A), a["M"], 4, a["U"], a["V"], a["ft"], a["sigma"], a["levels"], a["r"], a["k"],
                1, _lib.dptr(flow), _lib.dptr(cost), _lib.dptr(curv)]
        if entry == "gqmap_block_match_pyramid":
            args += [C.cast(C.byref(ms), _lib._D), 0]
        return getattr(lib, entry)(*args), ms.value

    if entry.endswith("_host"):
        assert call(a)[0] == 0 and not np.any(flow == 77.0)  # the base arguments are fine
        flow[:] = 77.0
        cost[:] = 77.0
        curv[:] = 77.0
    status, ms = call({**a, **kw})
    assert status == 1 and ms == -1.0  # GQMAP_ERR_INVALID_ARG
    assert entry.encode() in lib.gqmap_last_error()
    assert np.all(flow == 77.0) and np.all(cost == 77.0) and np.all(curv == 77.0)


def test_cost_and_curv_may_be_null():
    from gqmap_opticalflow_amd import _lib
    lib = _lib.load()
    crop, par = R.CROPS[4], R.PARAMS[2]
    A, B = R.crop_pair(crop)
    win = W.windows(crop, par, "mixed")
    flow = np.zeros((5, 7, 2), order="F")
    assert lib.gqmap_block_match_window_host(_lib.dptr(A), _lib.dptr(B), win.ctypes.data_as(C.POINTER(C.c_int)), 5, 7,
                                             par[2], par[3], 1, _lib.dptr(flow), None, None) == 0
    assert np.array_equal(bits(flow), bits(model(crop, par, "mixed", True)[0]))
    assert lib.gqmap_block_match_pyramid_host(_lib.dptr(A), _lib.dptr(B), 5, 7, 3, 3, par[2], par[3], 2, 1, 1, 1,
                                              _lib.dptr(flow), None, None) == 0
    assert np.array_equal(bits(flow), bits(pyramid_model(crop, par, 2, 1, 1, True)[0]))


# ---- the pyramid -------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pyramid_model(crop, params, levels, r, k, subpixel):
    from gqmap_opticalflow_amd import block_match_pyramid
    out = block_match_pyramid(*frames(crop), *params, levels=levels, r=r, k=k, subpixel=subpixel, host=True)
    for a in out:
        a.setflags(write=False)
    return out


def test_half_resolution_by_hand():
    P = np.arange(15, dtype=np.float64).reshape(3, 5)
    h = W.half(P)
    assert h.shape == (2, 3)
    assert h[0, 0] == ((0 + 5) + (1 + 6)) * 0.25 and h[1, 2] == ((14 + 14) + (14 + 14)) * 0.25
    assert h[0, 2] == ((4 + 9) + (4 + 9)) * 0.25 and h[1, 0] == ((10 + 10) + (11 + 11)) * 0.25


@pytest.mark.parametrize("r", [0, 1])
@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("levels", [1, 2, 3])
@pytest.mark.parametrize("crop", [CROP_97, R.CROPS[4]], ids=str)
def test_pyramid_host_model_equals_restatement_bit_for_bit(crop, levels, k, r):
    """97 x 130 (49 x 65 and 25 x 33 above it) and 5 x 7 (3 x 4, 2 x 2): odd
    sizes at every level.  Sub-pixel at level 0 only."""
    par = (7, 7, 3, 1.7) if crop == CROP_97 else (3, 3, 2, 1.0)
    got = pyramid_model(crop, par, levels, r, k, True)
    want = W.pyramid(*frames(crop), *par, levels, r, k, subpixel=True)
    assert_bit_equal(got, want)
    assert np.abs(got[0]).max() <= W.reach(par[0], levels, r) + 0.5
    integer = pyramid_model(crop, par, levels, r, k, False)
    assert np.array_equal(bits(integer[1]), bits(got[1])) and np.abs(integer[0] - got[0]).max() <= 0.5


@pytest.mark.parametrize("crop", [CROP_97, R.CROPS[4]], ids=str)
def test_one_level_is_the_plain_matcher(crop):
    from gqmap_opticalflow_amd import block_match
    par = (7, 7, 3, 1.7)
    A, B = frames(crop)
    assert_bit_equal(pyramid_model(crop, par, 1, 1, 1, False), block_match(A, B, *par, host=True))
    assert_bit_equal(pyramid_model(crop, par, 1, 0, 2, True),
                     [a[..., 0] for a in block_match(A, B, *par, host=True, subpixel=True)])


def test_reach():
    from gqmap_opticalflow_amd import block_match_reach
    for U, levels, r in ((7, 1, 1), (7, 2, 1), (20, 3, 1), (25, 4, 2), (64, 2, 0), (0, 3, 4), (1024, 6, 4)):
        assert block_match_reach(U, levels, r) == W.reach(U, levels, r)
    assert block_match_reach(7, 2, 1) == 9 and block_match_reach(20, 3, 1) == 23
    with pytest.raises(ValueError):
        block_match_reach(7, 7, 1)


def known_aepe(gt, flow):
    known = np.all(np.abs(gt) <= 1e9, axis=2)
    return float(np.sqrt(np.sum((gt - flow) ** 2, axis=2))[known].mean())


def test_rubberwhale_pyramid_start_is_as_good_as_the_full_search():
    """388 x 584, (7, 7, 3, 1.7), integer flow, known pixels: two levels, r = 1,
    k = 1 against the full search of the host model at the same U, V.  Measured:
    0.50739 against 0.50003."""
    from gqmap_opticalflow_amd import block_match_init
    I1, I2, gt = R.rubberwhale()
    full, rng = block_match_init(I1, I2, host=True)
    pyr, prng = block_match_init(I1, I2, host=True, levels=2)
    assert rng == dict(minu=-7.0, maxu=7.0, minv=-7.0, maxv=7.0) and prng == dict(minu=-9.0, maxu=9.0, minv=-9.0, maxv=9.0)
    a, b = known_aepe(gt, full), known_aepe(gt, pyr)
    print(f"full search AEPE {a:.5f}, pyramid AEPE {b:.5f}")
    assert b <= a + 0.05


def test_urban3_pyramid_start_beats_the_full_search():
    """480 x 640, (20, 20, 3, 1.7), integer flow, known pixels: three levels,
    r = 1, k = 1 against the full search of the host model at the same U, V.
    Measured: 3.89960 against 5.02733."""
    from gqmap_opticalflow_amd import block_match_pyramid, load_pair
    I1, I2, gt = load_pair("Urban3")
    full = block_match_pyramid(I1, I2, 20, 20, 3, 1.7, levels=1, host=True)[0]
    pyr = block_match_pyramid(I1, I2, 20, 20, 3, 1.7, levels=3, r=1, k=1, host=True)[0]
    a, b = known_aepe(gt, 0.0 - full), known_aepe(gt, 0.0 - pyr)
    print(f"full search AEPE {a:.5f}, pyramid AEPE {b:.5f}")
    assert b < a


# ---- block_match_init(levels=) -----------------------------------------------------------------

PAR = (3, 3, 2, 1.0)
INIT_KW = [dict(), dict(hypotheses=3), dict(hypotheses=3, sep=3), dict(engine="super"), dict(engine="super", hypotheses=3),
           dict(subpixel=True), dict(hypotheses=3, subpixel=True), dict(hypotheses=3, subpixel=True, sigma_from_cost=True),
           dict(subpixel=True, sigma_from_cost=True, lambdad=4.0, sigma_min=0.1),
           dict(engine="super", hypotheses=3, subpixel=True, sigma_from_cost=True),
           dict(consistency=True), dict(subpixel=True, consistency=True, fill=True),
           dict(hypotheses=3, subpixel=True, sigma_from_cost=True, consistency=True, fill=True, fill_r=2),
           dict(engine="super", hypotheses=3, subpixel=True, sigma_from_cost=True, consistency=True)]


def same(a, b):
    if isinstance(a, dict):
        return a == b
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True) and \
        (a.dtype != np.float64 or np.array_equal(bits(a), bits(b)))


@pytest.mark.parametrize("kw", INIT_KW, ids=str)
def test_levels_1_returns_what_block_match_init_returned(kw):
    """The keyword combinations of tests/test_init_flow.py, tests/test_block_match_*.py
    and tests/test_flow_check.py: same arity, same bits; pyr_r and pyr_k reach nothing."""
    from gqmap_opticalflow_amd import block_match_init
    I1, I2 = R.crop_pair(R.CROPS[0])
    a = block_match_init(I1, I2, *PAR, host=True, **kw)
    b = block_match_init(I1, I2, *PAR, host=True, levels=1, pyr_r=3, pyr_k=2, **kw)
    assert len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))


def test_levels_2_is_the_pyramid_at_rank_0():
    from gqmap_opticalflow_amd import block_match_init, block_match_pyramid
    I1, I2 = R.crop_pair(R.CROPS[0])
    out, cost, curv = block_match_pyramid(I1, I2, *PAR, levels=2, r=2, k=0, subpixel=True, host=True)
    flow, ranges = block_match_init(I1, I2, *PAR, host=True, levels=2, pyr_r=2, pyr_k=0, subpixel=True)
    assert ranges == dict(minu=-6.0, maxu=6.0, minv=-6.0, maxv=6.0)  # reach(3, 2, 2) = 2 * 2 + 2
    assert flow.shape == (40, 48, 2) and np.array_equal(flow, 0.0 - out)
    plain, _ = block_match_init(I1, I2, *PAR, host=True, levels=2, pyr_r=2, pyr_k=0)
    assert plain.shape == (40, 48, 2)
    one, _ = block_match_init(I1, I2, *PAR, host=True, levels=2, pyr_r=2, pyr_k=0, hypotheses=1)
    assert one.shape == (40, 48, 2, 1) and np.array_equal(one[..., 0], plain)
    _, _, sig = block_match_init(I1, I2, *PAR, host=True, levels=2, pyr_r=2, pyr_k=0, subpixel=True, sigma_from_cost=True)
    pos = curv > 0
    assert sig.shape == (40, 48, 2) and pos.any() and np.all(np.isnan(sig[~pos]))
    assert np.array_equal(sig[pos], np.maximum(np.sqrt(1.0 / curv[pos]), 0.5))
    # U beyond 32: fine while its coarsest level is not
    wide, wrng = block_match_init(I1, I2, 40, 36, 2, 1.0, host=True, levels=2)
    assert wide.shape == (40, 48, 2) and wrng == dict(minu=-37.0, maxu=37.0, minv=-41.0, maxv=41.0)


def test_levels_2_with_consistency_and_fill():
    from gqmap_opticalflow_amd import block_match_init, block_match_pyramid, flow_consistency
    I1, I2 = R.crop_pair(R.CROPS[0])
    kw = dict(host=True, levels=2, subpixel=True, sigma_from_cost=True)
    raw, rng, rsig = block_match_init(I1, I2, *PAR, **kw)
    flow, rng2, sig, cons = block_match_init(I1, I2, *PAR, consistency=True, **kw)
    assert rng == rng2 and flow.shape == raw.shape == sig.shape == (40, 48, 2) and cons.shape == (40, 48)
    assert cons.dtype == bool and cons.any() and (~cons).any()
    back = 0.0 - block_match_pyramid(I2, I1, *PAR, levels=2, subpixel=True, host=True)[0]
    assert np.array_equal(cons, flow_consistency(raw, back, host=True)[1])
    assert np.array_equal(flow[cons], raw[cons]) and np.all(np.isnan(flow[~cons])) and np.all(np.isnan(sig[~cons]))
    fill, _, fsig, fcons = block_match_init(I1, I2, *PAR, consistency=True, fill=True, **kw)
    assert np.array_equal(fcons, cons) and np.array_equal(fill[cons], raw[cons])
    assert np.isnan(fill).sum() < np.isnan(flow).sum() and np.array_equal(fsig, sig, equal_nan=True)
    nodes, _, nsig, ncons = block_match_init(I1, I2, *PAR, engine="super", consistency=True, fill=True, **kw)
    assert nodes.shape == nsig.shape == (10, 12, 2) and ncons.shape == (40, 48)


def test_levels_2_with_several_hypotheses_raises():
    from gqmap_opticalflow_amd import block_match_init
    I1, I2 = R.crop_pair(R.CROPS[0])
    with pytest.raises(ValueError):
        block_match_init(I1, I2, *PAR, host=True, levels=2, hypotheses=2)


# ---- the kernels' listing ------------------------------------------------------------------------

# the occupancy step (128 VGPRs: four workgroups of 256 lanes per CU, 168: three) of each instantiation of
# k_block_match_window<NPT, REFINE, RANKED>, by the template arguments in the mangled name
VGPR_STEP = {
    "ILi1ELb0ELb0E": 128, "ILi2ELb0ELb0E": 128, "ILi4ELb0ELb0E": 128,  # plain, integer
    "ILi1ELb1ELb0E": 128, "ILi2ELb1ELb0E": 128, "ILi4ELb1ELb0E": 168,  # plain, sub-pixel
    "ILi1ELb0ELb1E": 128, "ILi2ELb0ELb1E": 128, "ILi4ELb0ELb1E": 168,  # ranked, integer
    "ILi1ELb1ELb1E": 128, "ILi2ELb1ELb1E": 128, "ILi4ELb1ELb1E": 168,  # ranked, sub-pixel
}


@pytest.mark.skipif(not _codeobj.available(), reason="library or ROCm LLVM tools absent")
def test_window_kernels_have_no_scratch_and_bounded_registers():
    """The gfx950 code object's metadata (tests/_codeobj.py).  Twelve
    instantiations of k_block_match_window (tile widths 8, 16, 32; integer and
    sub-pixel; plain and ranked) beside k_bm_half and k_bm_window_up, none with
    scratch or spills, and no separate ranked kernel.  The plain integer kernels
    stay within the 128 VGPRs that allow four workgroups per CU; the plain
    sub-pixel kernel at 32 columns carries four neighbour costs per output on
    top and may use up to 168 (three workgroups per CU).  The earlier ranks'
    keys (three ints per output) and the rank loop cost registers: at 32 columns
    both ranked modes sit in the 168 step, where the tile's LDS allows no more
    than three workgroups per CU anyway.  Static LDS (the union box and the
    vote) stays small beside the dynamic tile."""
    every = _codeobj.kernels()
    # the family has one tile kernel (the full search's k_block_match<...> mangles without the underscore)
    assert not [k for k in every if "k_block_match_" in k and "k_block_match_window" not in k]
    seen = {k: v for k, v in every.items() if "k_block_match_window" in k or "k_bm_half" in k or "k_bm_window_up" in k}
    window = {k: v for k, v in seen.items() if "k_block_match_window" in k}
    assert len(window) == 12 and len(seen) == 14, sorted(seen)
    for name, v in seen.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0, name
    steps = dict(VGPR_STEP)
    for name, v in window.items():
        tag = [t for t in steps if t in name]
        assert len(tag) == 1, name
        print(name, v)
        assert v["vgpr_count"] <= steps.pop(tag[0]), (name, v)
        assert v["group_segment_fixed_size"] <= 1024, (name, v)
    assert not steps, sorted(steps)
