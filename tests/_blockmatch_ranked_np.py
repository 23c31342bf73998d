"""Numpy restatement of the ranked window matcher and of the ranked
coarse-to-fine scheme (csrc/gqmap_blockmatch.h, "Ranked windows" and "Ranked
coarse to fine"), written from the header's text.  The filtered cost of a
displacement, the halving, the window rule, the weights and the parabola are
those of tests/_blockmatch_window_np.py and tests/_blockmatch_refine_np.py, so
the library's host models agree with it BIT FOR BIT.  Rank j is stated as a scan
in ascending (dv, du) over the displacements of box j that are at least sep away
from the pick of every earlier rank that has one; the first of them takes the
pick whatever its cost, a later one replaces it on a strictly smaller cost.
Independent of the library."""
import functools

import numpy as np

from tests import _blockmatch_np as R
from tests import _blockmatch_window_np as W
from tests._blockmatch_refine_np import refine_axis, weights
from tests._blockmatch_window_np import cost_plane, half, window_up

NOPICK = W.NOPICK


def ranked_window(A, B, win, ft, sigma, sep, subpixel=False):
    """win: M x N x 4 x H.  (flow M x N x 2 x H, cost M x N x H, curv M x N x 2 x H,
    pick M x N x 2 x H = (du0, dv0) planes per rank, NOPICK without a pick)."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    M, N = A.shape
    H = win.shape[3]
    w = weights(ft, sigma)
    planes = {}

    def plane(du, dv):
        if (du, dv) not in planes:
            planes[(du, dv)] = cost_plane(A, B, du, dv, w)
        return planes[(du, dv)]

    flow, cost = np.full((M, N, 2, H), np.nan), np.full((M, N, H), np.inf)
    curv, pick = np.zeros((M, N, 2, H)), np.full((M, N, 2, H), NOPICK, dtype=np.int64)
    for j in range(H):
        ulo, uhi, vlo, vhi = (win[:, :, q, j].astype(np.int64) for q in range(4))
        some = (ulo <= uhi) & (vlo <= vhi)
        best = np.full((M, N), np.inf)
        pu, pv = np.full((M, N), NOPICK, dtype=np.int64), np.full((M, N), NOPICK, dtype=np.int64)
        if some.any():
            for dv in range(int(vlo[some].min()), int(vhi[some].max()) + 1):
                for du in range(int(ulo[some].min()), int(uhi[some].max()) + 1):
                    allowed = some & (ulo <= du) & (du <= uhi) & (vlo <= dv) & (dv <= vhi)
                    for i in range(j):  # a missing earlier rank excludes nothing
                        eu, ev = pick[:, :, 0, i], pick[:, :, 1, i]
                        allowed &= (eu == NOPICK) | (np.maximum(np.abs(du - eu), np.abs(dv - ev)) >= sep)
                    if not allowed.any():
                        continue
                    c = plane(du, dv)
                    take = allowed & ((pu == NOPICK) | (c < best))
                    best = np.where(allowed & (c < best), c, best)
                    pu, pv = np.where(take, du, pu), np.where(take, dv, pv)
        found = pu != NOPICK
        pick[:, :, 0, j], pick[:, :, 1, j], cost[:, :, j] = pu, pv, best
        fu, fv = (-pu).astype(np.float64), (-pv).astype(np.float64)
        if subpixel:
            cm, cp = np.full((M, N, 2), np.nan), np.full((M, N, 2), np.nan)  # axis 0: u, axis 1: v
            for m, n in zip(*np.nonzero(found)):
                u0, v0 = int(pu[m, n]), int(pv[m, n])
                if ulo[m, n] < u0 < uhi[m, n]:  # the plain costs, allowed at this rank or not
                    cm[m, n, 0], cp[m, n, 0] = plane(u0 - 1, v0)[m, n], plane(u0 + 1, v0)[m, n]
                if vlo[m, n] < v0 < vhi[m, n]:
                    cm[m, n, 1], cp[m, n, 1] = plane(u0, v0 - 1)[m, n], plane(u0, v0 + 1)[m, n]
            du_, ku = refine_axis(cm[:, :, 0], best, cp[:, :, 0], found & (ulo < pu) & (pu < uhi))
            dv_, kv = refine_axis(cm[:, :, 1], best, cp[:, :, 1], found & (vlo < pv) & (pv < vhi))
            fu, fv = fu - du_, fv - dv_
            curv[:, :, 0, j], curv[:, :, 1, j] = np.where(found, kv, 0.0), np.where(found, ku, 0.0)
        flow[:, :, 0, j], flow[:, :, 1, j] = np.where(found, fv, np.nan), np.where(found, fu, np.nan)
    return flow, cost, curv, pick


def ranked_pyramid(A, B, U, V, ft, sigma, levels, r, k, H, sep, subpixel=False):
    """(flow, cost, curv) of level 0."""
    frames = [(np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64))]
    for _ in range(1, levels):
        frames.append(tuple(half(P) for P in frames[-1]))
    c = levels - 1
    Uc, Vc = -(-U // 2 ** c), -(-V // 2 ** c)
    win = same_window(W.constant_window(*frames[c][0].shape, Uc, Vc), H)
    for l in range(c, -1, -1):
        if l < c:  # box j from the rank-j picks of the level above
            win = np.stack([window_up(pick[:, :, :, j], *frames[l][0].shape, r, k) for j in range(H)],  # noqa: F821
                           axis=3)
        flow, cost, curv, pick = ranked_window(*frames[l], win, ft, sigma, sep, subpixel and l == 0)
    return flow, cost, curv


def same_window(win, H):
    """One M x N x 4 window at every rank."""
    return np.asfortranarray(np.repeat(win[..., None], H, axis=3))


# ---- the ranked windows of the tests ---------------------------------------------------------

def make_ranked_windows(M, N, U, V, kind, H, seed=0):
    """W.make_windows with another seed per rank, M x N x 4 x H.  On top, for
    "mixed" (pixels away from those W.make_windows sets):
      (0, 1)          box 1 empty while box 2 is not (H >= 3);
      (0, 2)          all H boxes the same single displacement: ranks >= 1 missing;
      (M - 3, N - 2)  all H boxes the same 3 x 3 box: at sep = 2 rank 1 is left
                      with what lies two away from rank 0's pick, at sep = 3
                      with nothing;
      (M - 1, 0)      ranks 0 and 1 with disjoint boxes 40 apart."""
    win = np.stack([W.make_windows(M, N, U, V, kind, seed=seed + 101 * j) for j in range(H)], axis=3)
    if kind == "mixed":
        if H >= 3:
            win[0, 1, :, 0] = (-1, 1, -1, 1)
            win[0, 1, :, 1] = (1, 0, 0, 0)
            win[0, 1, :, 2] = (-1, 1, 2, 4)
        win[0, 2] = np.array((1, 1, -2, -2))[:, None]
        win[M - 3, N - 2] = np.array((-1, 1, 0, 2))[:, None]
        win[M - 1, 0, :, 0] = (-1, 0, -21, -20)
        if H >= 2:
            win[M - 1, 0, :, 1] = (0, 1, 20, 21)
    return np.asfortranarray(win.astype(np.int32))


@functools.lru_cache(maxsize=None)
def windows(crop, params, kind, H):
    win = make_ranked_windows(crop[2], crop[3], params[0], params[1], kind, H, seed=crop[0] + params[0])
    win.setflags(write=False)
    return win


@functools.lru_cache(maxsize=None)
def reference(crop, params, kind, H, sep, subpixel):
    """The restatement on one crop and one kind of window, computed once and shared (read-only)."""
    out = ranked_window(*R.crop_pair(crop), windows(crop, params, kind, H), params[2], params[3], sep, subpixel)[:3]
    for a in out:
        a.setflags(write=False)
    return out
