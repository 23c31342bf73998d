"""Numpy restatement of the several-hypotheses rule of the block matcher
(csrc/gqmap_blockmatch.h, "Several hypotheses per pixel") on the FULL cost
volume of tests/_blockmatch_np.py: rank 0 is the first minimum; rank k >= 1 is
the first minimum over the displacements (u, v) with
max(|u - u_j|, |v - v_j|) >= sep for the pick of every earlier rank j < k; a
rank with no displacement left is missing (index -1, cost +Inf), and so are
all later ones.  Independent of the library."""
import functools

import numpy as np

from tests import _blockmatch_np as R


def far_from(idx, U, V, sep):
    """M x N x nd mask: displacement (linear index u + v(2U+1)) at least sep
    away (Chebyshev) from the pick idx (M x N); a missing pick (-1) forbids
    nothing."""
    nu = 2 * U + 1
    lin = np.arange(nu * (2 * V + 1))
    uu, vv = lin % nu, lin // nu
    pu, pv = (idx % nu)[:, :, None], (idx // nu)[:, :, None]
    far = np.maximum(np.abs(uu - pu), np.abs(vv - pv)) >= sep
    return far | (idx < 0)[:, :, None]


def allowed_after(picks, U, V, sep, shape):
    """The displacements allowed once `picks` (a list of M x N index arrays) are taken."""
    M, N = shape
    ok = np.ones((M, N, (2 * U + 1) * (2 * V + 1)), dtype=bool)
    for p in picks:
        ok &= far_from(p, U, V, sep)
    return ok


def greedy(vol, U, V, H, sep):
    """vol: M x N x nd.  Returns idx (M x N x H, -1 = missing), cost (M x N x H,
    +Inf = missing) and gap (M x N x H: second-smallest minus smallest allowed
    cost, +Inf with fewer than two allowed)."""
    M, N, nd = vol.shape
    idx = np.full((M, N, H), -1)
    cost = np.full((M, N, H), np.inf)
    gap = np.full((M, N, H), np.inf)
    ok = np.ones((M, N, nd), dtype=bool)
    for k in range(H):
        masked = np.where(ok, vol, np.inf)
        has = ok.any(axis=2)
        first = np.argmin(masked, axis=2)  # the first minimum
        idx[:, :, k] = np.where(has, first, -1)
        cost[:, :, k] = np.where(has, np.take_along_axis(masked, first[:, :, None], axis=2)[:, :, 0], np.inf)
        if nd > 1:
            two = np.partition(masked, 1, axis=2)[:, :, :2]
            with np.errstate(invalid="ignore"):
                g = two[:, :, 1] - two[:, :, 0]
            gap[:, :, k] = np.where(ok.sum(axis=2) >= 2, g, np.inf)
        ok = ok & far_from(idx[:, :, k], U, V, sep) & has[:, :, None]
    return idx, cost, gap


def flow_to_index(flow, U, V):
    """flow M x N x 2 x H = (V - v, U - u) -> linear index u + v(2U+1), -1 where NaN."""
    missing = np.isnan(flow[:, :, 0]) | np.isnan(flow[:, :, 1])
    f = np.where(np.isnan(flow), 0.0, flow)
    idx = (U - f[:, :, 1]).astype(int) + (V - f[:, :, 0]).astype(int) * (2 * U + 1)
    return np.where(missing, -1, idx)


@functools.lru_cache(maxsize=None)
def reference(crop, params, H, sep):
    """The greedy restatement on one crop, computed once and shared (read-only)."""
    vol = R.reference(crop, params)[2]
    out = greedy(vol, params[0], params[1], H, sep)
    for a in out:
        a.setflags(write=False)
    return out
