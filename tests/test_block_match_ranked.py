"""Ranked hypotheses over per-pixel windows and through the coarse-to-fine
matcher, host models (gqmap_block_match_window_multi_host,
gqmap_block_match_pyramid_multi_host) against the numpy restatement of
tests/_blockmatch_ranked_np.py, bit for bit; the three identities of the header
against the existing host models; missing ranks; argument errors;
block_match_init(pyr_ranked=True); the quality of three ranks on whole frames.
The kernels' code object is checked in tests/test_block_match_window.py.  No
device."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from tests import _blockmatch_np as R
from tests import _blockmatch_ranked_np as K
from tests import _blockmatch_window_np as W

NAN_BITS = 0x7FF8000000000000
CROP_97 = "97x130"
HS = ((2, 1), (3, 2), (4, 3))  # (H, sep)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def assert_bit_equal(got, want, names=("flow", "cost", "curv")):
    assert len(got) == len(want)
    for g, w, what in zip(got, want, names):
        assert g.shape == w.shape, what
        diff = bits(g) != bits(w)
        assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} entries differ"


def rank(out, j):
    return [a[..., j] for a in out]


def frames(crop):
    return W.pair_97x130() if crop == CROP_97 else R.crop_pair(crop)


@functools.lru_cache(maxsize=None)
def model(crop, params, kind, H, sep, subpixel):
    from gqmap_opticalflow_amd import block_match_window
    out = block_match_window(*R.crop_pair(crop), K.windows(crop, params, kind, H), params[2], params[3],
                             subpixel=subpixel, host=True, hypotheses=H, sep=sep)
    for a in out:
        a.setflags(write=False)
    return out


# ---- the ranked window matcher -----------------------------------------------------------------

def trimmed_cases():
    """R.CROPS x R.PARAMS[:3] x both kinds of window x HS x integer / sub-pixel, trimmed to keep
    the file quick: the two small crops (33 x 17, 5 x 7) run the whole product; each 40 x 48 crop
    runs every (params, kind) once, (H, sep) and integer / sub-pixel taking turns, so that every
    (H, sep) meets every params, both kinds and both modes there."""
    cases = []
    for i, (crop, params, kind) in enumerate(itertools.product(R.CROPS, R.PARAMS[:3], W.KINDS)):
        if crop[2] * crop[3] < 1000:
            cases += [(crop, params, kind, hs, sub) for hs in HS for sub in (False, True)]
        else:
            cases.append((crop, params, kind, HS[(i + i // 6) % 3], bool((i + i // 3) % 2)))
    return cases


@pytest.mark.parametrize("crop,params,kind,hs,subpixel", trimmed_cases(), ids=str)
def test_host_model_equals_restatement_bit_for_bit(crop, params, kind, hs, subpixel):
    got = model(crop, params, kind, *hs, subpixel)
    want = K.reference(crop, params, kind, *hs, subpixel)
    assert len(got) == (3 if subpixel else 2)
    assert got[0].shape == (crop[2], crop[3], 2, hs[0]) and got[1].shape == (crop[2], crop[3], hs[0])
    assert_bit_equal(got, want[:len(got)])


def test_the_trimmed_cases_cover_every_combination_pairwise():
    cases = trimmed_cases()
    big = [c for c in cases if c[0][2] * c[0][3] >= 1000]
    assert {c[3] for c in big} == set(HS) and {c[4] for c in big} == {False, True}
    assert {(c[1], c[3]) for c in big} == set(itertools.product(R.PARAMS[:3], HS))
    assert {(c[2], c[3], c[4]) for c in cases} == set(itertools.product(W.KINDS, HS, (False, True)))


@pytest.mark.parametrize("crop", R.CROPS, ids=str)
def test_missing_ranks(crop):
    """The pixels that K.make_ranked_windows plants, and what the matcher makes of them."""
    par = R.PARAMS[0]
    _, _, M, N = crop
    win = K.windows(crop, par, "mixed", 3)
    flow, cost, curv = model(crop, par, "mixed", 3, 2, True)
    at = -model(crop, par, "mixed", 3, 2, False)[0][:, :, ::-1, :]  # the integer picks (du, dv)

    def missing(m, n, j):
        return (np.all(bits(flow[m, n, :, j]) == NAN_BITS) and np.isposinf(cost[m, n, j]) and
                np.all(curv[m, n, :, j] == 0))

    # box 1 empty while box 2 is not: rank 1 is missing, rank 2 goes on and keeps clear of rank 0 only
    assert tuple(win[0, 1, :, 1]) == (1, 0, 0, 0) and missing(0, 1, 1)
    assert not missing(0, 1, 0) and not missing(0, 1, 2)
    assert np.max(np.abs(at[0, 1, :, 0] - at[0, 1, :, 2])) >= 2
    # the same single displacement in every box: ranks >= 1 have nothing allowed
    assert tuple(flow[0, 2, :, 0]) == (2.0, -1.0) and missing(0, 2, 1) and missing(0, 2, 2)
    # one 3 x 3 box at every rank, sep 2: every later pick at least two away from every earlier one
    p = [at[M - 3, N - 2, :, j] for j in range(3)]
    assert not missing(M - 3, N - 2, 0)
    for a in range(3):
        for b in range(a):
            if not missing(M - 3, N - 2, a) and not missing(M - 3, N - 2, b):
                assert np.max(np.abs(p[a] - p[b])) >= 2
    # sep 3 leaves nothing of a 3 x 3 box beside rank 0
    f3, c3, _ = model(crop, par, "mixed", 4, 3, True)
    assert np.all(np.isnan(f3[M - 3, N - 2, :, 1:])) and np.all(np.isposinf(c3[M - 3, N - 2, 1:]))
    # two ranks with disjoint boxes 40 apart: both found, each in its own box
    assert not missing(M - 1, 0, 0) and not missing(M - 1, 0, 1)
    assert -flow[M - 1, 0, 0, 0] <= -19.5 and -flow[M - 1, 0, 0, 1] >= 19.5
    # every rank stays inside its own box, within half a pixel of an integer
    for j in range(3):
        found = ~np.isnan(flow[:, :, 0, j])
        f, w = flow[:, :, :, j][found], win[:, :, :, j][found]
        assert np.all(-f[:, 1] >= w[:, 0] - 0.5) and np.all(-f[:, 1] <= w[:, 1] + 0.5)
        assert np.all(-f[:, 0] >= w[:, 2] - 0.5) and np.all(-f[:, 0] <= w[:, 3] + 0.5)
        empty = (win[:, :, 0, j] > win[:, :, 1, j]) | (win[:, :, 2, j] > win[:, :, 3, j])
        assert np.all(~found[empty]) and np.all(np.isposinf(cost[:, :, j][~found]))


# ---- the identities ----------------------------------------------------------------------------

@pytest.mark.parametrize("subpixel", [False, True], ids=["integer", "subpixel"])
@pytest.mark.parametrize("kind", W.KINDS)
@pytest.mark.parametrize("crop", R.CROPS[2:], ids=str)
def test_identity_1_and_2_rank_0_is_the_window_matcher(crop, kind, subpixel):
    """H = 1 is gqmap_block_match_window; rank 0 of any H and sep is
    gqmap_block_match_window on box 0."""
    from gqmap_opticalflow_amd import block_match_window
    par = R.PARAMS[2]
    A, B = R.crop_pair(crop)
    win1 = K.windows(crop, par, kind, 1)
    plain = block_match_window(A, B, win1[..., 0], par[2], par[3], subpixel=subpixel, host=True)
    one = block_match_window(A, B, win1, par[2], par[3], subpixel=subpixel, host=True, hypotheses=1, sep=2)
    assert_bit_equal(rank(one, 0), plain)
    for H, sep in HS:
        win = K.windows(crop, par, kind, H)
        want = block_match_window(A, B, win[..., 0], par[2], par[3], subpixel=subpixel, host=True)
        assert_bit_equal(rank(model(crop, par, kind, H, sep, subpixel), 0), want)


@pytest.mark.parametrize("hs", HS + ((3, 7), (4, 1)), ids=str)
@pytest.mark.parametrize("params", R.PARAMS, ids=str)
def test_identity_3_equal_boxes_are_the_multi_matcher(params, hs):
    """All H boxes [-U, U] x [-V, V]: gqmap_block_match_multi and
    gqmap_block_match_refine at the same H and sep, missing ranks included
    (sep = 7 leaves nothing beside rank 0 at U = V = 3); a broadcast M x N x 4
    window is the same call."""
    from gqmap_opticalflow_amd import block_match, block_match_window
    H, sep = hs
    crop = R.CROPS[3]
    A, B = R.crop_pair(crop)
    U, V, ft, sigma = params
    win = W.constant_window(*A.shape, U, V)
    multi = block_match(A, B, *params, host=True, hypotheses=H, sep=sep)
    assert_bit_equal(block_match_window(A, B, win, ft, sigma, host=True, hypotheses=H, sep=sep), multi)
    assert_bit_equal(block_match_window(A, B, K.same_window(win, H), ft, sigma, host=True, hypotheses=H, sep=sep), multi)
    fine = block_match(A, B, *params, host=True, hypotheses=H, sep=sep, subpixel=True)
    assert_bit_equal(block_match_window(A, B, win, ft, sigma, subpixel=True, host=True, hypotheses=H, sep=sep), fine)


def test_identity_3_on_nan_frames():
    """Costs that are never < +Inf: every rank names the first allowed
    displacement in ascending (dv, du), as gqmap_block_match_multi does."""
    from gqmap_opticalflow_amd import block_match, block_match_pyramid, block_match_window
    A = np.full((6, 5), np.nan, order="F")
    for H, sep in HS + ((4, 4),):
        want = block_match(A, A, 2, 1, 1, 1.0, host=True, hypotheses=H, sep=sep, subpixel=True)
        got = block_match_window(A, A, W.constant_window(6, 5, 2, 1), 1, 1.0, subpixel=True, host=True, hypotheses=H,
                                 sep=sep)
        assert_bit_equal(got, want)
        assert_bit_equal(block_match_pyramid(A, A, 2, 1, 1, 1.0, levels=1, subpixel=True, host=True, hypotheses=H,
                                             sep=sep), want)
        assert np.all(np.isposinf(got[1]))
    # by hand: rank 0 is (du, dv) = (-2, -1), the first of the box; at sep = 1 rank 1 is the next, (-1, -1)
    got = block_match_window(A, A, W.constant_window(6, 5, 2, 1), 1, 1.0, host=True, hypotheses=2, sep=1)
    assert np.all(got[0][:, :, 0, 0] == 1) and np.all(got[0][:, :, 1, 0] == 2) and np.all(got[0][:, :, 1, 1] == 1)


@functools.lru_cache(maxsize=None)
def pyramid_model(crop, params, levels, r, k, H, sep, subpixel):
    from gqmap_opticalflow_amd import block_match_pyramid
    out = block_match_pyramid(*frames(crop), *params, levels=levels, r=r, k=k, subpixel=subpixel, host=True,
                              hypotheses=H, sep=sep)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("levels", [1, 2, 3])
@pytest.mark.parametrize("crop", [CROP_97, R.CROPS[4]], ids=str)
def test_identities_through_the_levels(crop, levels):
    """H = 1 through the levels, and rank 0 of H = 3, are gqmap_block_match_pyramid;
    levels = 1 is gqmap_block_match_multi / gqmap_block_match_refine."""
    from gqmap_opticalflow_amd import block_match, block_match_pyramid
    par = (7, 7, 3, 1.7) if crop == CROP_97 else (3, 3, 2, 1.0)
    A, B = frames(crop)
    for subpixel in (False, True):
        plain = block_match_pyramid(A, B, *par, levels=levels, r=1, k=1, subpixel=subpixel, host=True)
        assert_bit_equal(rank(pyramid_model(crop, par, levels, 1, 1, 1, 2, subpixel), 0), plain)
        assert_bit_equal(rank(pyramid_model(crop, par, levels, 1, 1, 3, 2, subpixel), 0), plain)
        assert_bit_equal(rank(pyramid_model(crop, par, levels, 1, 1, 4, 3, subpixel), 0), plain)
        if levels == 1:
            assert_bit_equal(pyramid_model(crop, par, 1, 1, 1, 3, 2, subpixel),
                             block_match(A, B, *par, host=True, hypotheses=3, sep=2, subpixel=subpixel))


# ---- the ranked pyramid ------------------------------------------------------------------------

@pytest.mark.parametrize("levels,r,k,hs", [(2, 1, 1, (3, 2)), (3, 1, 1, (3, 2)), (2, 0, 0, (2, 1)), (3, 2, 2, (4, 3)),
                                           (2, 1, 2, (4, 3))], ids=str)
@pytest.mark.parametrize("crop", [CROP_97, R.CROPS[4]], ids=str)
def test_pyramid_host_model_equals_restatement_bit_for_bit(crop, levels, r, k, hs):
    """97 x 130 (49 x 65 and 25 x 33 above it) and 5 x 7 (3 x 4, 2 x 2): odd sizes
    at every level.  Sub-pixel at level 0 only; the integer call has the same
    costs and flows within half a pixel."""
    par = (7, 7, 3, 1.7) if crop == CROP_97 else (3, 3, 2, 1.0)
    got = pyramid_model(crop, par, levels, r, k, *hs, True)
    want = K.ranked_pyramid(*frames(crop), *par, levels, r, k, *hs, subpixel=True)
    assert_bit_equal(got, want)
    found = ~np.isnan(got[0])
    assert np.abs(got[0][found]).max() <= W.reach(par[0], levels, r) + 0.5
    integer = pyramid_model(crop, par, levels, r, k, *hs, False)
    assert np.array_equal(bits(integer[1]), bits(got[1]))
    assert np.array_equal(np.isnan(integer[0]), ~found) and np.abs(integer[0][found] - got[0][found]).max() <= 0.5
    if crop == CROP_97 and r > 0:  # r = 0, k = 0: every box is one displacement, nothing to refine
        assert found[..., 1:].any() and np.any(got[2][..., 1:] > 0)


# ---- argument errors ---------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(H=0), dict(H=5), dict(sep=0), dict(sep=66), dict(bound=2049), dict(bound=-2049),
                                dict(win=None), dict(ft=5), dict(M=0)], ids=str)
@pytest.mark.parametrize("entry", ["gqmap_block_match_window_multi_host", "gqmap_block_match_window_multi"])
def test_window_multi_argument_errors_write_nothing(entry, kw):
    """The bound out of range sits in slice H - 1."""
    from gqmap_opticalflow_amd import _lib
    lib = _lib.load()
    a = dict(H=3, sep=2, ft=1, sigma=1.0, M=4, bound=1, win=True)
    a.update(kw)
    A = np.zeros((4, 4), order="F")
    win = K.same_window(W.constant_window(4, 4, 1, 1), 4)
    win[2, 3, 1, max(0, min(a["H"], 4) - 1)] = a["bound"]
    flow, cost, curv = (np.full(s, 77.0, order="F") for s in ((4, 4, 2, 4), (4, 4, 4), (4, 4, 2, 4)))
    ms = C.c_double(-1.0)
    args = [_lib.dptr(A), _lib.dptr(A), win.ctypes.data_as(C.POINTER(C.c_int)) if a["win"] else None, a["M"], 4, a["ft"],
            a["sigma"], a["H"], a["sep"], 1, _lib.dptr(flow), _lib.dptr(cost), _lib.dptr(curv)]
    if entry == "gqmap_block_match_window_multi":
        args += [C.cast(C.byref(ms), _lib._D), 0]
    assert getattr(lib, entry)(*args) == 1  # GQMAP_ERR_INVALID_ARG
    assert entry.encode() in lib.gqmap_last_error()
    assert np.all(flow == 77.0) and np.all(cost == 77.0) and np.all(curv == 77.0) and ms.value == -1.0


@pytest.mark.parametrize("kw", [dict(H=0), dict(H=5), dict(sep=0), dict(sep=66), dict(levels=7), dict(r=5), dict(k=3),
                                dict(U=65)], ids=str)
@pytest.mark.parametrize("entry", ["gqmap_block_match_pyramid_multi_host", "gqmap_block_match_pyramid_multi"])
def test_pyramid_multi_argument_errors_write_nothing(entry, kw):
    from gqmap_opticalflow_amd import _lib
    lib = _lib.load()
    a = dict(levels=2, r=1, k=1, U=64, V=2, ft=1, sigma=1.0, M=4, H=4, sep=65)
    A = np.zeros((4, 4), order="F")
    flow, cost, curv = (np.full(s, 77.0, order="F") for s in ((4, 4, 2, 4), (4, 4, 4), (4, 4, 2, 4)))

    def call(a):
        ms = C.c_double(-1.0)
        args = [_lib.dptr(A), _lib.dptr(A), a["M"], 4, a["U"], a["V"], a["ft"], a["sigma"], a["levels"], a["r"], a["k"],
                a["H"], a["sep"], 1, _lib.dptr(flow), _lib.dptr(cost), _lib.dptr(curv)]
        if entry == "gqmap_block_match_pyramid_multi":
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


def test_python_argument_errors():
    from gqmap_opticalflow_amd import block_match_pyramid, block_match_window
    A = np.zeros((4, 4), order="F")
    win = W.constant_window(4, 4, 1, 1)
    for H in (0, 5):
        with pytest.raises(ValueError):
            block_match_window(A, A, win, 1, 1.0, host=True, hypotheses=H)
        with pytest.raises(ValueError):
            block_match_pyramid(A, A, 2, 2, 1, 1.0, host=True, hypotheses=H)
    with pytest.raises(ValueError):
        block_match_window(A, A, K.same_window(win, 3), 1, 1.0, host=True, hypotheses=2)
    with pytest.raises(ValueError):
        block_match_window(A, A, K.same_window(win, 2), 1, 1.0, host=True)
    with pytest.raises(RuntimeError):
        block_match_window(A, A, win, 1, 1.0, host=True, hypotheses=2, sep=66)


def test_cost_and_curv_may_be_null():
    from gqmap_opticalflow_amd import _lib
    lib = _lib.load()
    crop, par = R.CROPS[4], R.PARAMS[2]
    A, B = R.crop_pair(crop)
    win = K.windows(crop, par, "mixed", 3)
    flow = np.zeros((5, 7, 2, 3), order="F")
    assert lib.gqmap_block_match_window_multi_host(_lib.dptr(A), _lib.dptr(B), win.ctypes.data_as(C.POINTER(C.c_int)), 5,
                                                   7, par[2], par[3], 3, 2, 1, _lib.dptr(flow), None, None) == 0
    assert np.array_equal(bits(flow), bits(model(crop, par, "mixed", 3, 2, True)[0]))
    assert lib.gqmap_block_match_pyramid_multi_host(_lib.dptr(A), _lib.dptr(B), 5, 7, 3, 3, par[2], par[3], 2, 1, 1, 3, 2,
                                                    1, _lib.dptr(flow), None, None) == 0
    assert np.array_equal(bits(flow), bits(pyramid_model(crop, par, 2, 1, 1, 3, 2, True)[0]))


# ---- block_match_init(pyr_ranked=True) ---------------------------------------------------------

PAR = (3, 3, 2, 1.0)


def test_block_match_init_takes_its_ranks_from_the_ranked_pyramid():
    from gqmap_opticalflow_amd import block_match_init, block_match_pyramid
    from gqmap_opticalflow_amd.engine import _super_hypotheses
    I1, I2 = R.crop_pair(R.CROPS[0])
    kw = dict(host=True, levels=2, pyr_r=2, pyr_k=0)
    out, cost, curv = block_match_pyramid(I1, I2, *PAR, levels=2, r=2, k=0, subpixel=True, host=True, hypotheses=3, sep=2)
    flow, ranges = block_match_init(I1, I2, *PAR, hypotheses=3, pyr_ranked=True, subpixel=True, **kw)
    assert ranges == dict(minu=-6.0, maxu=6.0, minv=-6.0, maxv=6.0)  # +-reach(3, 2, 2), as without the ranks
    assert flow.shape == (40, 48, 2, 3) and np.array_equal(flow, 0.0 - out, equal_nan=True)
    # rank 0 is the start without pyr_ranked, integer and sub-pixel
    for sub in (False, True):
        ranked, _ = block_match_init(I1, I2, *PAR, hypotheses=3, pyr_ranked=True, subpixel=sub, **kw)
        plain, _ = block_match_init(I1, I2, *PAR, subpixel=sub, **kw)
        assert np.array_equal(bits(ranked[..., 0]), bits(plain))
    # pyr_ranked without further hypotheses, or at one level, changes nothing
    a, b = block_match_init(I1, I2, *PAR, pyr_ranked=True, **kw)[0], block_match_init(I1, I2, *PAR, **kw)[0]
    assert np.array_equal(bits(a), bits(b))
    a = block_match_init(I1, I2, *PAR, host=True, hypotheses=3, pyr_ranked=True)[0]
    assert np.array_equal(bits(a), bits(block_match_init(I1, I2, *PAR, host=True, hypotheses=3)[0]))
    # sigma: NaN where curv is 0, shaped as flow
    _, _, sig = block_match_init(I1, I2, *PAR, hypotheses=3, pyr_ranked=True, subpixel=True, sigma_from_cost=True, **kw)
    pos = curv > 0
    assert sig.shape == (40, 48, 2, 3) and pos[..., 1:].any() and np.all(np.isnan(sig[~pos]))
    assert np.array_equal(sig[pos], np.maximum(np.sqrt(1.0 / curv[pos]), 0.5))
    # the super node rule: rank 0 the block mean, rank k >= 1 the cheapest pixel's flow
    nodes, _, nsig = block_match_init(I1, I2, *PAR, engine="super", hypotheses=3, pyr_ranked=True, subpixel=True,
                                      sigma_from_cost=True, **kw)
    want, wcurv = _super_hypotheses(np.asfortranarray(0.0 - out), cost, curv)
    assert nodes.shape == nsig.shape == (10, 12, 2, 3) and np.array_equal(nodes, want, equal_nan=True)
    assert np.array_equal(nodes[..., 0], (0.0 - out[..., 0]).reshape(10, 4, 12, 4, 2).mean(axis=(1, 3)))
    m, n = np.unravel_index(np.argmin(cost[:4, :4, 1].T), (4, 4))[::-1]  # column-major order of the block
    assert np.array_equal(nodes[0, 0, :, 1], 0.0 - out[m, n, :, 1])
    assert np.array_equal(np.isnan(nsig), ~(wcurv > 0))


def test_block_match_init_ranked_with_consistency_and_fill():
    """The forward pass is ranked, the backward pass the plain pyramid with one hypothesis."""
    from gqmap_opticalflow_amd import block_match_init, block_match_pyramid, flow_consistency
    I1, I2 = R.crop_pair(R.CROPS[0])
    kw = dict(host=True, levels=2, hypotheses=3, pyr_ranked=True, subpixel=True, sigma_from_cost=True)
    raw, rng, rsig = block_match_init(I1, I2, *PAR, **kw)
    flow, rng2, sig, cons = block_match_init(I1, I2, *PAR, consistency=True, **kw)
    assert rng == rng2 and flow.shape == raw.shape == sig.shape == (40, 48, 2, 3)
    assert cons.shape == (40, 48, 3) and cons.dtype == bool and cons.any() and (~cons).any()
    back = 0.0 - block_match_pyramid(I2, I1, *PAR, levels=2, subpixel=True, host=True)[0]
    for j in range(3):
        assert np.array_equal(cons[:, :, j], flow_consistency(np.asfortranarray(raw[..., j]), back, host=True)[1])
        assert np.array_equal(flow[..., j][cons[:, :, j]], raw[..., j][cons[:, :, j]])
        assert np.all(np.isnan(flow[..., j][~cons[:, :, j]])) and np.all(np.isnan(sig[..., j][~cons[:, :, j]]))
    one = block_match_init(I1, I2, *PAR, host=True, levels=2, subpixel=True, sigma_from_cost=True, consistency=True)
    assert np.array_equal(cons[:, :, 0], one[3]) and np.array_equal(flow[..., 0], one[0], equal_nan=True)
    fill, _, fsig, fcons = block_match_init(I1, I2, *PAR, consistency=True, fill=True, **kw)
    assert np.array_equal(fcons, cons) and np.isnan(fill[..., 0]).sum() < np.isnan(flow[..., 0]).sum()
    assert np.array_equal(fill[..., 1:], flow[..., 1:], equal_nan=True) and np.array_equal(fsig, sig, equal_nan=True)
    nodes, _, nsig, ncons = block_match_init(I1, I2, *PAR, engine="super", consistency=True, fill=True, **kw)
    assert nodes.shape == nsig.shape == (10, 12, 2, 3) and ncons.shape == (40, 48, 3)


def test_levels_2_with_several_hypotheses_still_raises_by_default():
    from gqmap_opticalflow_amd import block_match_init
    I1, I2 = R.crop_pair(R.CROPS[0])
    with pytest.raises(ValueError):
        block_match_init(I1, I2, *PAR, host=True, levels=2, hypotheses=2, pyr_ranked=False)


# ---- quality on whole frames -------------------------------------------------------------------

def known_epe(gt, flow):
    """End-point error at the known pixels; a missing rank counts as +Inf."""
    known = np.all(np.abs(gt) <= 1e9, axis=2)
    epe = np.sqrt(np.sum((gt - flow) ** 2, axis=2))[known]
    return np.where(np.isnan(epe), np.inf, epe)


def best_of_ranks(name, par, levels):
    """(rank 0 AEPE, best-of-3 AEPE) over the known pixels: r = k = 1, H = 3, sep = 2, integer flow."""
    from gqmap_opticalflow_amd import block_match_pyramid, load_pair
    I1, I2, gt = load_pair(name)
    plain = block_match_pyramid(I1, I2, *par, levels=levels, r=1, k=1, host=True)
    ranked = block_match_pyramid(I1, I2, *par, levels=levels, r=1, k=1, host=True, hypotheses=3, sep=2)
    assert_bit_equal(rank(ranked, 0), plain)
    epe = np.stack([known_epe(gt, 0.0 - ranked[0][..., j]) for j in range(3)])
    a, b = float(epe[0].mean()), float(epe.min(axis=0).mean())
    print(f"{name}: rank 0 AEPE {a:.5f}, best of 3 ranks {b:.5f}")
    return a, b


def test_rubberwhale_three_ranks_beat_rank_0():
    """388 x 584, (7, 7, 3, 1.7), two levels.  Measured: rank 0 0.50739, best of 3 ranks 0.37314."""
    a, b = best_of_ranks("rubberwhale", (7, 7, 3, 1.7), 2)
    assert b < a


def test_urban3_three_ranks_beat_rank_0():
    """480 x 640, (20, 20, 3, 1.7), three levels.  Measured: rank 0 3.89960, best of 3 ranks 2.53447."""
    a, b = best_of_ranks("Urban3", (20, 20, 3, 1.7), 3)
    assert b < a
