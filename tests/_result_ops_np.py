"""Plain references and seeded inputs for the ops that turn a converged state
into the answer: the mixture MAP, the simplex projection and the flow colour.

Nothing here shares code with the kernels (csrc/gqmap_ops.hip) or with their C
restatement (oracle/gqmap_oracle.c).  The MAP is not recomputed: a second
Brent search would repeat the first one's mistakes.  It is *checked*, through
three properties that any correct answer of findMixMax.m has and a wrong one
does not (map_properties).  The projection is the sort-and-threshold form in
np.longdouble.

The input families are functions of nothing but the seeds below, so the CPU
tests (tests/test_result_ops.py) and the device tests
(tests/test_gpu_result_ops.py) see the same arrays.
"""
from __future__ import annotations

import functools

import numpy as np

M, N = 37, 29  # MN = 1073: no multiple of the 256-thread block
SQRT_EPS = float(np.sqrt(np.finfo(np.float64).eps))
TOLX = 1e-4  # fminbnd's TolX in findMixMax.m


# ---- the mixture density ------------------------------------------------------

def _terms(x, a, u, o):
    x = np.asarray(x, dtype=np.float64)[..., None]
    z = (x - u) / o
    with np.errstate(under="ignore"):
        return x, np.asarray(a, dtype=np.float64) * np.exp(-0.5 * z * z) / (np.sqrt(2.0 * np.pi) * o)


def density(x, a, u, o):
    """sum_l a_l N(x; u_l, o_l) in numpy fp64.  x: (...), a: (L,), u, o: (..., L)."""
    return _terms(x, a, u, o)[1].sum(axis=-1)


def ddensity(x, a, u, o):
    """d density / dx."""
    x, t = _terms(x, a, u, o)
    with np.errstate(under="ignore"):
        return (t * (-(x - u) / (o * o))).sum(axis=-1)


def tol1(g):
    """Brent's tol1 at the point g (MATLAB fminbnd: sqrt(eps) |x| + TolX / 3)."""
    return SQRT_EPS * np.abs(g) + TOLX / 3.0


def map_properties(g, a, u, o):
    """(P1, P2, P3), boolean arrays shaped as g, of a claimed mixture MAP g.
    g: (...), a: (L,), u, o: (..., L) -- one axis of the flow; map_properties_uv
    takes both.

    P1  density(g) >= max_l density(u_l) (1 - 1e-12): the search result is
        returned only if it beats the best mean (under the device's exp; the
        1e-12 covers its 1-ulp difference from numpy's).
    P2  min u <= g <= max u.
    P3  g is some u_l bit for bit, or ddensity(g - d) >= 0 >= ddensity(g + d)
        with d = 3 tol1(g): Brent's stopping rule leaves the bracket's ends
        within 2 tol1 of the point returned, with a local minimum between
        them; the third tol1 covers rounding of the derivative."""
    g = np.asarray(g, dtype=np.float64)
    at_means = np.stack([density(u[..., l], a, u, o) for l in range(u.shape[-1])], axis=-1)
    p1 = density(g, a, u, o) >= at_means.max(axis=-1) * (1 - 1e-12)
    p2 = (u.min(axis=-1) <= g) & (g <= u.max(axis=-1))
    d = 3.0 * tol1(g)
    p3 = is_a_mean(g, u) | ((ddensity(g - d, a, u, o) >= 0) & (0 >= ddensity(g + d, a, u, o)))
    return p1, p2, p3


def is_a_mean(g, u):
    return (np.asarray(g)[..., None] == u).any(axis=-1)


def map_properties_uv(mp, fam):
    """map_properties of an M x N x 2 map on a family / state dict (alpha, muu,
    sigu, muv, sigv): three M x N x 2 boolean arrays."""
    pu = map_properties(mp[:, :, 0], fam["alpha"], fam["muu"], fam["sigu"])
    pv = map_properties(mp[:, :, 1], fam["alpha"], fam["muv"], fam["sigv"])
    return tuple(np.stack([x, y], axis=2) for x, y in zip(pu, pv))


def least_likely_mean(fam):
    """Per pixel and axis the mean at which the mixture is smallest: a wrong answer that P2 and P3 accept."""
    out = []
    for u, o in ((fam["muu"], fam["sigu"]), (fam["muv"], fam["sigv"])):
        at = np.stack([density(u[..., l], fam["alpha"], u, o) for l in range(u.shape[-1])], axis=-1)
        out.append(np.take_along_axis(u, at.argmin(axis=-1)[..., None], axis=-1)[..., 0])
    return np.asfortranarray(np.stack(out, axis=2))


# ---- mixture families -------------------------------------------------------------

def _fam(alpha, muu, sigu, muv, sigv):
    d = dict(alpha=np.asarray(alpha, dtype=np.float64), **{k: np.asfortranarray(v) for k, v in
                                                           (("muu", muu), ("sigu", sigu), ("muv", muv), ("sigv", sigv))})
    for v in d.values():
        v.setflags(write=False)
    return d


def _random(L, seed):
    rng = np.random.default_rng(seed)
    mu = [2.0 * rng.normal(size=(M, N, L)) for _ in range(2)]
    sg = [0.05 + 2.0 * rng.random((M, N, L)) for _ in range(2)]
    alpha = rng.random(L) + 0.1
    return alpha / alpha.sum(), mu[0], sg[0], mu[1], sg[1]


@functools.lru_cache(maxsize=None)
def random(L):
    """mu ~ 2 N(0,1), sigma ~ U[0.05, 2.05], alpha random and normalised."""
    return _fam(*_random(L, 1000 + L))


@functools.lru_cache(maxsize=None)
def interior(L):
    """L odd.  The middle component weighs 0.6; the others, of the same width,
    sit at -+ k s sigma with s ~ U(3, 6) per side: the answer lies inside the
    bracket, next to the middle mean but not on it."""
    rng = np.random.default_rng(2000 + L)
    h = L // 2
    alpha = np.full(L, 0.4 / (L - 1))
    alpha[h] = 0.6
    out = []
    for _ in range(2):
        c = 2.0 * rng.normal(size=(M, N))
        sg = 0.3 + 1.2 * rng.random((M, N))
        mu = np.empty((M, N, L))
        mu[:, :, h] = c
        for side in (-1, 1):
            s = rng.uniform(3.0, 6.0, size=(M, N))
            for k in range(1, h + 1):
                mu[:, :, h + side * k] = c + side * k * s * sg
        out += [mu, np.repeat(sg[:, :, None], L, axis=2)]
    return _fam(alpha, *out)


@functools.lru_cache(maxsize=None)
def sym_pair():
    """Two equal components at c -+ d, d in [0.05, 0.9], sigma 1: unimodal (d < sigma), the answer is c."""
    rng = np.random.default_rng(3000)
    out = []
    for _ in range(2):
        c = 2.0 * rng.normal(size=(M, N))
        d = rng.uniform(0.05, 0.9, size=(M, N))
        out += [np.stack([c - d, c + d], axis=2), np.ones((M, N, 2))]
    fam = _fam([0.5, 0.5], *out)
    return fam


def sym_pair_centre(fam):
    return np.stack([0.5 * (fam["muu"][:, :, 0] + fam["muu"][:, :, 1]),
                     0.5 * (fam["muv"][:, :, 0] + fam["muv"][:, :, 1])], axis=2)


@functools.lru_cache(maxsize=None)
def same_mean():
    """Three components on one mean, three widths: a bracket of zero width.  The answer is that mean."""
    a, mu, sg, mv, sv = _random(3, 4000)
    return _fam(a, np.repeat(mu[:, :, :1], 3, axis=2), sg, np.repeat(mv[:, :, :1], 3, axis=2), sv)


@functools.lru_cache(maxsize=None)
def single():
    """L = 1: the bracket has zero width, the loop is never entered, the mean comes back."""
    return _fam(*_random(1, 5000))


@functools.lru_cache(maxsize=None)
def spike():
    """random(3) with the middle width 1e-6 at weight 0.1: a peak of height 4e4
    that a search at TolX 1e-4 cannot see.  The answer is the middle mean."""
    a, mu, sg, mv, sv = _random(3, 1003)
    a = np.array([a[0], 0.0, a[2]])
    a = 0.9 * a / a.sum()
    a[1] = 0.1
    sg[:, :, 1] = 1e-6
    sv[:, :, 1] = 1e-6
    return _fam(a, mu, sg, mv, sv)


@functools.lru_cache(maxsize=None)
def far():
    """Means at c and c -+ U(36, 39), sigma 1: -z^2/2 spans about -648 .. -760,
    where exp returns subnormals and, past -745, zeros."""
    rng = np.random.default_rng(6000)
    out = []
    for _ in range(2):
        c = 2.0 * rng.normal(size=(M, N))
        out += [np.stack([c - rng.uniform(36, 39, (M, N)), c, c + rng.uniform(36, 39, (M, N))], axis=2),
                np.ones((M, N, 3))]
    alpha = rng.random(3) + 0.1
    return _fam(alpha / alpha.sum(), *out)


@functools.lru_cache(maxsize=None)
def zero_alpha():
    """alpha = (0, 1, 0) on random means and widths: the answer is the middle mean."""
    _, mu, sg, mv, sv = _random(3, 7000)
    return _fam([0.0, 1.0, 0.0], mu, sg, mv, sv)


FAMILIES = {
    "random2": lambda: random(2), "random3": lambda: random(3), "random4": lambda: random(4),
    "random8": lambda: random(8), "interior3": lambda: interior(3), "interior5": lambda: interior(5),
    "sym_pair": sym_pair, "same_mean": same_mean, "single": single, "spike": spike, "far": far,
    "zero_alpha": zero_alpha,
}
# families whose answer is known exactly: the component whose mean it is
EXACT = {"same_mean": 0, "single": 0, "spike": 1, "zero_alpha": 1}


def exact_answer(name):
    fam, l = FAMILIES[name](), EXACT[name]
    return np.stack([fam["muu"][:, :, l], fam["muv"][:, :, l]], axis=2)


CROPS = [(1, 1), (1, 7), (7, 1), (16, 16), (3, 86)]  # MN = 1, 7, 7, 256, 258


def crop(fam, m, n):
    """The first m n pixels of a family (column-major order) as an m x n grid.
    The pixels are independent draws, so this is a crop in everything but the
    shape -- and 3 x 86 does not fit inside 37 x 29."""
    L = fam["muu"].shape[2]
    take = lambda a: np.asfortranarray(a.reshape((M * N, L), order="F")[:m * n].reshape((m, n, L), order="F"))
    return dict(alpha=fam["alpha"], **{k: take(fam[k]) for k in ("muu", "sigu", "muv", "sigv")})


def state_family(st):
    """An engine state (alpha, muu, ...) in the layout of a family."""
    return {k: np.asarray(getattr(st, k)) for k in ("alpha", "muu", "sigu", "muv", "sigv")}


# ---- simplex projection ---------------------------------------------------------------

def projsplx_ld(y):
    """Euclidean projection onto the probability simplex: sort, find the
    threshold, shift and clip -- in np.longdouble."""
    y = np.asarray(y, dtype=np.longdouble)
    if y.ndim == 2:  # every column
        s = -np.sort(-y, axis=0)
        css = np.cumsum(s, axis=0) - np.longdouble(1)
        j = np.arange(1, y.shape[0] + 1).astype(np.longdouble)[:, None]
        rho = y.shape[0] - 1 - np.argmax((s - css / j > 0)[::-1], axis=0)  # the last row that is still positive
        tau = np.take_along_axis(css, rho[None, :], axis=0) / (rho + 1).astype(np.longdouble)
        return np.maximum(y - tau, np.longdouble(0))
    s = np.sort(y)[::-1]
    css = np.cumsum(s) - np.longdouble(1)
    j = np.arange(1, y.size + 1).astype(np.longdouble)
    rho = np.nonzero(s - css / j > 0)[0][-1]
    return np.maximum(y - css[rho] / j[rho], np.longdouble(0))


PROJ_N = [1, 2, 3, 5, 8, 63, 64]
PROJ_NCOLS = [1, 255, 256, 257, 3000]
PROJ_KINDS = ["normal", "simplex", "equal", "ties", "large", "negative"]


@functools.lru_cache(maxsize=None)
def proj_input(n, kind, ncols=3000):
    """n x ncols columns to project (Fortran order); narrower inputs are its first columns."""
    rng = np.random.default_rng(8000 + 10 * n + PROJ_KINDS.index(kind))
    if kind == "normal":
        Y = rng.normal(size=(n, ncols))
    elif kind == "simplex":  # already on the simplex
        Y = rng.random((n, ncols)) + 1e-3
        Y = Y / Y.sum(axis=0)
    elif kind == "equal":  # every entry of a column equal
        Y = np.repeat(rng.normal(size=(1, ncols)), n, axis=0)
    elif kind == "ties":  # small integers: many equal entries
        Y = rng.integers(-3, 4, size=(n, ncols)).astype(np.float64)
    elif kind == "large":
        Y = 1e6 * rng.normal(size=(n, ncols))
    else:  # all negative
        Y = -np.abs(rng.normal(size=(n, ncols))) - 0.1
    Y = np.asfortranarray(Y)
    Y.setflags(write=False)
    return Y


def check_projection(x, y):
    """The bounds a projection x of y (a column, or every column of a matrix)
    must meet against projsplx_ld, each with the column's own scale.  Returns
    the largest (error / bound, |sum - 1| / bound) after asserting both and
    x >= 0.
      error      <= 1e-14 max(1, max|y|): the threshold is a sum of at most n
                 entries divided once, a few ulps of the largest entry;
      |sum - 1|  <= 2 n^2 eps max(1, max|y|): n entries, each off by the
                 threshold's error of at most n ulps of the scale."""
    x, y = (np.asarray(a).reshape(np.shape(a)[0], -1) for a in (x, y))
    n = y.shape[0]
    sc = np.maximum(1.0, np.max(np.abs(y), axis=0))
    err = np.max(np.abs(x.astype(np.longdouble) - projsplx_ld(y)), axis=0).astype(np.float64) / (1e-14 * sc)
    dsum = np.abs(np.sum(x.astype(np.longdouble), axis=0) - 1).astype(np.float64) / (
        2.0 * n * n * np.finfo(np.float64).eps * sc)
    assert np.all(x >= 0)
    assert err.max() <= 1, (n, int(err.argmax()), float(err.max()))
    assert dsum.max() <= 1, (n, int(dsum.argmax()), float(dsum.max()))
    return float(err.max()), float(dsum.max())


# ---- flow fields for the colour pass -----------------------------------------------------------

def _flow(m, n, seed):
    return np.asfortranarray(3.0 * np.random.default_rng(seed).normal(size=(m, n, 2)))


def mixed_flow():
    """37 x 29 with every special pixel of flowToColor.m in its first column."""
    f = _flow(M, N, 9005)
    f[0, 0] = (1e10, 0.3)        # unknown through u
    f[1, 0] = (0.2, -2e9)        # unknown through v
    f[2, 0] = (np.nan, np.nan)
    f[3, 0] = (np.nan, 1.0)      # NaN in u only
    f[4, 0] = (0.0, 0.0)
    f[5, 0] = (2.0, -0.0)        # atan2(+0, -2) = +pi: k0 = ncols, k1 wraps to 1
    f[6, 0] = (2.0, 0.0)         # atan2(-0, -2) = -pi: k0 = 1
    f[7, 0] = (-1.0, 0.0)
    return f


@functools.lru_cache(maxsize=None)
def flow_cases():
    """name -> (flow, max_flow)."""
    cases = {f"random_{m}x{n}": (_flow(m, n, 9000 + k), 0.0)
             for k, (m, n) in enumerate([(1, 1), (1, 7), (16, 17), (M, N)])}
    cases["mixed"] = (mixed_flow(), 0.0)
    cases["mixed_maxflow"] = (mixed_flow(), 2.5)
    cases["zeros"] = (np.zeros((5, 6, 2), order="F"), 0.0)
    cases["unknown"] = (np.full((5, 6, 2), 1e10, order="F"), 0.0)
    cases["nan"] = (np.full((5, 6, 2), np.nan, order="F"), 0.0)
    for f, _ in cases.values():
        f.setflags(write=False)
    return cases
