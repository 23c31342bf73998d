"""Numpy restatement of the per-pixel-window matcher and of the coarse-to-fine
scheme (csrc/gqmap_blockmatch.h, "Per-pixel windows" and "Coarse to fine"),
written from the header's text.  The filtered cost of one signed displacement is
built in the header's separable order (rows, then columns, ascending taps,
every product and sum a separate fp64 operation; weights as
tests/_blockmatch_refine_np.py), so the library's host models agree with it BIT
FOR BIT.  The pick is stated here as a scan in ascending (dv, du) that replaces
on a strictly smaller cost, the first displacement taking the pick whatever its
cost: the order the header's tie rule is equivalent to.  Independent of the
library."""
import functools

import numpy as np

from tests import _blockmatch_np as R
from tests._blockmatch_refine_np import refine_axis, weights

NOPICK = 0x7FFFFFFF


def shifted(B, du, dv):
    """B(m + du, n + dv), zero outside the frame."""
    M, N = B.shape
    out = np.zeros((M, N))
    m0, m1, n0, n1 = max(0, -du), min(M, M - du), max(0, -dv), min(N, N - dv)
    if m0 < m1 and n0 < n1:
        out[m0:m1, n0:n1] = B[m0 + du:m1 + du, n0 + dv:n1 + dv]
    return out


def cost_plane(A, B, du, dv, w):
    """The filtered cost of every pixel at one displacement."""
    M, N = A.shape
    ft = (len(w) - 1) // 2
    D = np.zeros((M + 2 * ft, N + 2 * ft))
    D[ft:ft + M, ft:ft + N] = np.abs(A - shifted(B, du, dv))
    T = np.zeros((M, N + 2 * ft))
    for i in range(2 * ft + 1):
        T = T + w[i] * D[i:i + M, :]
    c = np.zeros((M, N))
    for j in range(2 * ft + 1):
        c = c + w[j] * T[:, j:j + N]
    return c


def window(A, B, win, ft, sigma, subpixel=False):
    """(flow, cost, curv, pick): pick = (du0, dv0) planes, NOPICK without a pick."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    M, N = A.shape
    w = weights(ft, sigma)
    ulo, uhi, vlo, vhi = (win[:, :, q].astype(np.int64) for q in range(4))
    some = (ulo <= uhi) & (vlo <= vhi)
    best = np.full((M, N), np.inf)
    pu, pv = np.full((M, N), NOPICK, dtype=np.int64), np.full((M, N), NOPICK, dtype=np.int64)
    planes = {}
    if some.any():
        for dv in range(int(vlo[some].min()), int(vhi[some].max()) + 1):
            for du in range(int(ulo[some].min()), int(uhi[some].max()) + 1):
                inside = some & (ulo <= du) & (du <= uhi) & (vlo <= dv) & (dv <= vhi)
                if not inside.any():
                    continue
                c = planes[(du, dv)] = cost_plane(A, B, du, dv, w)
                take = inside & ((pu == NOPICK) | (c < best))
                best = np.where(inside & (c < best), c, best)
                pu, pv = np.where(take, du, pu), np.where(take, dv, pv)
    found = pu != NOPICK
    flow = np.full((M, N, 2), np.nan)
    flow[:, :, 0], flow[:, :, 1] = np.where(found, (-pv).astype(np.float64), np.nan), \
        np.where(found, (-pu).astype(np.float64), np.nan)
    curv = np.zeros((M, N, 2))
    if subpixel:
        cm, cp = np.full((M, N, 2), np.nan), np.full((M, N, 2), np.nan)  # axis 0: u, axis 1: v
        for m, n in zip(*np.nonzero(found)):
            u0, v0 = int(pu[m, n]), int(pv[m, n])
            if ulo[m, n] < u0 < uhi[m, n]:
                cm[m, n, 0], cp[m, n, 0] = planes[(u0 - 1, v0)][m, n], planes[(u0 + 1, v0)][m, n]
            if vlo[m, n] < v0 < vhi[m, n]:
                cm[m, n, 1], cp[m, n, 1] = planes[(u0, v0 - 1)][m, n], planes[(u0, v0 + 1)][m, n]
        du_, ku = refine_axis(cm[:, :, 0], best, cp[:, :, 0], found & (ulo < pu) & (pu < uhi))
        dv_, kv = refine_axis(cm[:, :, 1], best, cp[:, :, 1], found & (vlo < pv) & (pv < vhi))
        flow[:, :, 0] = np.where(found, (-pv).astype(np.float64) - dv_, np.nan)
        flow[:, :, 1] = np.where(found, (-pu).astype(np.float64) - du_, np.nan)
        curv[:, :, 0], curv[:, :, 1] = np.where(found, kv, 0.0), np.where(found, ku, 0.0)
    return flow, best, curv, np.stack([pu, pv], axis=2)


def half(P):
    """bm_half: ((P(2i, 2j) + P(2i+1, 2j)) + (P(2i, 2j+1) + P(2i+1, 2j+1))) * 0.25, odd edges clamped."""
    M, N = P.shape
    r0, c0 = np.arange(0, M, 2), np.arange(0, N, 2)
    r1, c1 = np.minimum(r0 + 1, M - 1), np.minimum(c0 + 1, N - 1)
    return ((P[np.ix_(r0, c0)] + P[np.ix_(r1, c0)]) + (P[np.ix_(r0, c1)] + P[np.ix_(r1, c1)])) * 0.25


def window_up(pick, M, N, r, k):
    """The boxes of the M x N fine pixels from the coarse picks (Mc x Nc x 2)."""
    Mc, Nc = pick.shape[:2]
    mm, nn = np.meshgrid(np.arange(M) >> 1, np.arange(N) >> 1, indexing="ij")
    big = np.iinfo(np.int64).max
    ulo, vlo = np.full((M, N), big), np.full((M, N), big)
    uhi, vhi = np.full((M, N), -big), np.full((M, N), -big)
    for a in range(-k, k + 1):
        for b in range(-k, k + 1):
            i, j = np.clip(mm + a, 0, Mc - 1), np.clip(nn + b, 0, Nc - 1)
            du, dv = pick[i, j, 0], pick[i, j, 1]
            has = du != NOPICK
            ulo, uhi = np.where(has, np.minimum(ulo, du), ulo), np.where(has, np.maximum(uhi, du), uhi)
            vlo, vhi = np.where(has, np.minimum(vlo, dv), vlo), np.where(has, np.maximum(vhi, dv), vhi)
    some = ulo != big
    win = np.stack([np.where(some, 2 * ulo - r, 1), np.where(some, 2 * uhi + r, 0), np.where(some, 2 * vlo - r, 1),
                    np.where(some, 2 * vhi + r, 0)], axis=2)
    return np.asfortranarray(win.astype(np.int32))


def constant_window(M, N, U, V):
    win = np.zeros((M, N, 4), dtype=np.int32, order="F")
    win[:, :, 0], win[:, :, 1], win[:, :, 2], win[:, :, 3] = -U, U, -V, V
    return win


def pyramid(A, B, U, V, ft, sigma, levels, r, k, subpixel=False):
    """(flow, cost, curv) of level 0."""
    frames = [(np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64))]
    for _ in range(1, levels):
        frames.append(tuple(half(P) for P in frames[-1]))
    c = levels - 1
    Uc, Vc = -(-U // 2 ** c), -(-V // 2 ** c)
    win = constant_window(*frames[c][0].shape, Uc, Vc)
    for l in range(c, -1, -1):
        if l < c:
            win = window_up(pick, *frames[l][0].shape, r, k)  # noqa: F821 (set by the level above)
        flow, cost, curv, pick = window(*frames[l], win, ft, sigma, subpixel and l == 0)
    return flow, cost, curv


def reach(U, levels, r):
    c = levels - 1
    return -(-U // 2 ** c) * 2 ** c + r * (2 ** c - 1)


# ---- the windows of the tests ----------------------------------------------------------------

KINDS = ("mixed", "halves")


def make_windows(M, N, U, V, kind, seed=0):
    """mixed: boxes drawn around centres in [-U, U] x [-V, V] with half extents 0..3,
    and among them an empty window, a single displacement and a window wholly off
    the frame (B is zero there: every cost of it ties).  halves: the left half of
    the frame searches dv in [-22, -20], the right half dv in [20, 22] -- 40
    apart, and both inside one tile."""
    rng = np.random.default_rng(seed)
    if kind == "halves":
        win = np.zeros((M, N, 4), dtype=np.int32, order="F")
        win[:, :, 0], win[:, :, 1] = -2, 1
        win[:, :N // 2, 2], win[:, :N // 2, 3] = -22, -20
        win[:, N // 2:, 2], win[:, N // 2:, 3] = 20, 22
        return win
    cu, cv = rng.integers(-U, U + 1, (M, N)), rng.integers(-V, V + 1, (M, N))
    hu, hv = rng.integers(0, 4, (M, N)), rng.integers(0, 4, (M, N))
    win = np.asfortranarray(np.stack([cu - hu, cu + hu, cv - hv, cv + hv], axis=2).astype(np.int32))
    win[0, 0] = (1, 0, -1, 1)  # empty
    win[M // 2, N // 2] = (3, 2, 5, 4)  # empty on both axes
    win[M - 1, N - 1] = (2, 2, -1, -1)  # one displacement
    win[1, 2] = (M + 4, M + 6, -1, 1)  # wholly off the frame
    win[M - 2, 1] = (-1, 1, -(N + 9), -(N + 7))
    return win


@functools.lru_cache(maxsize=None)
def windows(crop, params, kind):
    win = make_windows(crop[2], crop[3], params[0], params[1], kind, seed=crop[0] + params[0])
    win.setflags(write=False)
    return win


def pair_97x130():
    I1, I2, _ = R.rubberwhale()
    return tuple(np.asfortranarray(a[60:157, 210:340]) for a in (I1, I2))


@functools.lru_cache(maxsize=None)
def reference(crop, params, kind, subpixel):
    """The restatement on one crop and one kind of window, computed once and shared (read-only)."""
    out = window(*R.crop_pair(crop), windows(crop, params, kind), params[2], params[3], subpixel)[:3]
    for a in out:
        a.setflags(write=False)
    return out
