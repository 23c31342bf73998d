"""Numpy restatement of the forward-backward check and the fill
(csrc/gqmap_flowcheck.h), written from the header's text in the header's
operation order: every product and sum a separate fp64 operation (numpy
contracts nothing), the fill's weights from math.exp, rows before columns,
taps ascending from 0.  Built that way the library's host models agree with it
bit for bit, which tests/test_flow_check.py asserts.  Independent of the
library; the fields the tests feed it come from the host matcher."""
import functools
import math

import numpy as np

from tests import _blockmatch_np as R

UNFILLED = 255
# (U, V, ft, sigma) of R.PARAMS the flow-check tests run on every crop
PARAMS = (R.PARAMS[0], R.PARAMS[2], R.PARAMS[4])


def check(fwd, bwd, a1, a2):
    """(err, mask) of fc_check on whole fields; fwd, bwd M x N x 2."""
    fwd, bwd = np.asarray(fwd, dtype=np.float64), np.asarray(bwd, dtype=np.float64)
    M, N, _ = fwd.shape
    m, n = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    u, v = fwd[:, :, 0], fwd[:, :, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        x, y = n.astype(np.float64) + u, m.astype(np.float64) + v
        inside = (x >= 0) & (x <= N - 1) & (y >= 0) & (y <= M - 1)
        xs, ys = np.where(inside, x, 0.0), np.where(inside, y, 0.0)
        j0 = np.minimum(np.floor(xs).astype(np.int64), max(N - 2, 0))
        i0 = np.minimum(np.floor(ys).astype(np.int64), max(M - 2, 0))
        j1, i1 = np.minimum(j0 + 1, N - 1), np.minimum(i0 + 1, M - 1)
        fx, fy = xs - j0.astype(np.float64), ys - i0.astype(np.float64)

        def sample(P):
            return ((P[i0, j0] * (1 - fy) + P[i1, j0] * fy) * (1 - fx)) + ((P[i0, j1] * (1 - fy) + P[i1, j1] * fy) * fx)

        b0, b1 = sample(bwd[:, :, 0]), sample(bwd[:, :, 1])
        ru, rv = u + b0, v + b1
        e2 = ru * ru + rv * rv
        mag = (u * u + v * v) + (b0 * b0 + b1 * b1)
        thr = a1 * mag + a2
        ok = inside & (e2 <= thr)
    return np.where(inside, e2, np.inf), ok


def fill_weights(r, sigma):
    w = []
    for i in range(2 * r + 1):
        k = float(i - r)
        w.append(math.exp(-(k * k) / 2 / sigma / sigma))
    return w


def _filter(X, r, w):
    """Y_X: rows then columns of X (M x N, zero outside), ascending taps from 0."""
    M, N = X.shape
    P = np.zeros((M + 2 * r, N + 2 * r))
    P[r:r + M, r:r + N] = X
    T = np.zeros((M, N + 2 * r))
    for i in range(2 * r + 1):
        T = T + w[i] * P[i:i + M, :]
    Y = np.zeros((M, N))
    for j in range(2 * r + 1):
        Y = Y + w[j] * T[:, j:j + N]
    return Y


def fill(flow, mask, r, sigma, passes):
    """(out, filled) of the fill; flow M x N x 2, mask M x N (non-zero = valid)."""
    out = np.array(flow, dtype=np.float64, order="F")
    state = np.where(np.asarray(mask) != 0, 0, UNFILLED).astype(np.uint8)
    w = fill_weights(r, sigma)
    for p in range(1, passes + 1):
        valid = state != UNFILLED
        yv = _filter(np.where(valid, 1.0, 0.0), r, w)
        ys = [_filter(np.where(valid, out[:, :, c], 0.0), r, w) for c in (0, 1)]
        take = ~valid & (yv > 0)
        for c in (0, 1):
            with np.errstate(invalid="ignore", divide="ignore"):
                out[:, :, c] = np.where(take, ys[c] / yv, out[:, :, c])
        state = np.where(take, p, state).astype(np.uint8)
    return out, state


@functools.lru_cache(maxsize=None)
def fields(crop, params, subpixel=True):
    """(fwd, bwd) of the host matcher on one crop, both directions, in
    block_match_init's convention; computed once and shared (read-only)."""
    from gqmap_opticalflow_amd import block_match_init
    A, B = R.crop_pair(crop)
    fwd = block_match_init(A, B, *params, host=True, subpixel=subpixel)[0]
    bwd = block_match_init(B, A, *params, host=True, subpixel=subpixel)[0]
    for a in (fwd, bwd):
        a.setflags(write=False)
    return fwd, bwd


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)
