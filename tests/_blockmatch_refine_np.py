"""Numpy restatement of the sub-pixel refinement of the block matcher
(csrc/gqmap_blockmatch.h, "Sub-pixel refinement") on top of a full cost volume.

Unlike tests/_blockmatch_np.py (the literal 49-tap conv2), the volume here is
built in the HEADER's order: the separable filter, rows first and then columns,
taps in ascending order starting from 0, every product and sum a separate fp64
operation (numpy contracts nothing), the weights from math.exp normalised as
bm_filter does.  Built that way the library's host model agrees with it bit
for bit, which tests/test_block_match_refine.py asserts; the tolerance route
is not needed.  The ranks come from the greedy rule of
tests/_blockmatch_multi_np.py, the refinement is written from the header's
text.  Independent of the library."""
import functools
import math

import numpy as np

from tests import _blockmatch_multi_np as RM
from tests import _blockmatch_np as R


def weights(ft, sigma):
    """bm_filter: e_i = exp(-(i-ft)^2 / 2 / sigma / sigma), s = ((e_0 + e_1) + ...), w_i = e_i / s."""
    e = []
    for i in range(2 * ft + 1):
        k = float(i - ft)
        e.append(math.exp(-(k * k) / 2 / sigma / sigma))
    s = 0.0
    for x in e:
        s = s + x
    return [x / s for x in e]


def cost_volume(A, B, U, V, ft, sigma):
    """M x N x (2U+1) x (2V+1): T = rows of |A - B shifted| (B zero outside the
    frame, D zero outside the frame), cost = columns of T, ascending taps."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    M, N = A.shape
    w = weights(ft, sigma)
    Bext = np.zeros((M + 2 * U, N + 2 * V))
    Bext[U:U + M, V:V + N] = B
    vol = np.zeros((M, N, 2 * U + 1, 2 * V + 1))
    for u in range(2 * U + 1):
        for v in range(2 * V + 1):
            D = np.zeros((M + 2 * ft, N + 2 * ft))
            D[ft:ft + M, ft:ft + N] = np.abs(A - Bext[u:M + u, v:N + v])
            T = np.zeros((M, N + 2 * ft))
            for i in range(2 * ft + 1):
                T = T + w[i] * D[i:i + M, :]
            c = np.zeros((M, N))
            for j in range(2 * ft + 1):
                c = c + w[j] * T[:, j:j + N]
            vol[:, :, u, v] = c
    return vol


def refine_axis(cm, c0, cp, in_window):
    """bm_refine on arrays: (delta, den), both 0 where the axis is not refinable."""
    with np.errstate(invalid="ignore", divide="ignore"):
        den = (cm - c0) + (cp - c0)
        ok = in_window & (cm >= c0) & (cp >= c0) & (den > 0)
        delta = np.fmin(np.fmax((cm - cp) / (den + den), -0.5), 0.5)
    return np.where(ok, delta, 0.0), np.where(ok, den, 0.0)


def refine(vol4, idx, U, V):
    """vol4: M x N x (2U+1) x (2V+1); idx: M x N x H linear picks (-1: missing).
    Returns flow, curv (M x N x 2 x H, plane 0 horizontal) and c0 (M x N x H)."""
    M, N, H = idx.shape
    nu = 2 * U + 1
    mm, nn = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    flow = np.full((M, N, 2, H), np.nan)
    curv = np.zeros((M, N, 2, H))
    c0s = np.full((M, N, H), np.inf)
    for k in range(H):
        found = idx[:, :, k] >= 0
        u0, v0 = np.where(found, idx[:, :, k] % nu, 0), np.where(found, idx[:, :, k] // nu, 0)
        at = lambda u, v: vol4[mm, nn, np.clip(u, 0, 2 * U), np.clip(v, 0, 2 * V)]
        c0 = at(u0, v0)
        du, ku = refine_axis(at(u0 - 1, v0), c0, at(u0 + 1, v0), found & (u0 >= 1) & (u0 <= 2 * U - 1))
        dv, kv = refine_axis(at(u0, v0 - 1), c0, at(u0, v0 + 1), found & (v0 >= 1) & (v0 <= 2 * V - 1))
        flow[:, :, 0, k] = np.where(found, (V - v0).astype(np.float64) - dv, np.nan)
        flow[:, :, 1, k] = np.where(found, (U - u0).astype(np.float64) - du, np.nan)
        curv[:, :, 0, k] = np.where(found, kv, 0.0)
        curv[:, :, 1, k] = np.where(found, ku, 0.0)
        c0s[:, :, k] = np.where(found, c0, np.inf)
    return flow, curv, c0s


@functools.lru_cache(maxsize=None)
def volume(crop, params):
    vol = cost_volume(*R.crop_pair(crop), *params)
    vol.setflags(write=False)
    return vol


@functools.lru_cache(maxsize=None)
def reference(crop, params, H, sep):
    """(flow, curv, cost, idx) of the restatement on one crop, computed once and shared (read-only)."""
    vol4 = volume(crop, params)
    M, N = vol4.shape[:2]
    U, V = params[0], params[1]
    idx, _, _ = RM.greedy(vol4.reshape(M, N, -1, order="F"), U, V, H, sep)
    out = refine(vol4, idx, U, V) + (idx,)
    for a in out:
        a.setflags(write=False)
    return out
