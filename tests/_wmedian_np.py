"""Numpy restatement of the weighted median filter (csrc/gqmap_wmedian.h),
written from the header's text: the spatial taps from math.exp, every product,
sum and quotient of a weight a separate fp64 operation (numpy contracts
nothing), the weights taken to integers, the window stacked as shifted copies,
sorted by key, the integer weights summed from the smallest key up.  Built that
way the library's host model agrees with it bit for bit, which
tests/test_flow_wmedian.py asserts.  Independent of the library."""
import math

import numpy as np

SIGN = np.uint64(0x8000000000000000)
NAN_BITS = np.uint64(0x7FF8000000000000)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def taps(r, sigma_s):
    s = []
    for i in range(2 * r + 1):
        k = float(i - r)
        s.append(math.exp(-(k * k) / 2 / sigma_s / sigma_s))
    return s


def key(b):
    """The monotone key of a double's bits: sign set, all bits flipped; else the sign bit flipped."""
    return np.where(b >> np.uint64(63) != 0, ~b, b ^ SIGN)


def unkey(k):
    return np.where(k >> np.uint64(63) != 0, k ^ SIGN, ~k)


def _pad(X, r, fill, dtype):
    M, N = X.shape
    P = np.full((M + 2 * r, N + 2 * r), fill, dtype=dtype)
    P[r:r + M, r:r + N] = X
    return P


def weights(guide, conf, r, sigma_s, sigma_c):
    """wq of every entry: (2r+1)^2 x M x N integers, entry e = di + (2r+1) dj the
    pixel (m - r + di, n - r + dj); 0 outside the frame."""
    guide = np.asarray(guide, dtype=np.float64)
    M, N = guide.shape
    D = 2 * r + 1
    s = taps(r, sigma_s)
    G = _pad(guide, r, 0.0, np.float64)
    C = None if conf is None else _pad(np.asarray(conf, dtype=np.float64), r, 0.0, np.float64)
    inside = _pad(np.ones((M, N), dtype=bool), r, False, bool)
    wq = np.zeros((D * D, M, N), dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for dj in range(D):
            for di in range(D):
                win = (slice(di, di + M), slice(dj, dj + N))
                d = (G[win] - guide) / sigma_c
                w = (s[di] * s[dj]) * (1.0 / (1.0 + d * d))
                if C is not None:
                    w = w * C[win]
                ok = (w >= 2.0 ** -16) & inside[win]  # false on NaN
                wq[di + D * dj] = np.where(ok, np.where(w < 1.0, w, 1.0) * 65536.0, 0.0).astype(np.int64)
    return wq


def wmedian(flow, guide, r=2, sigma_s=2.0, sigma_c=10.0, passes=1, conf=None, history=False):
    """The filtered flow; flow M x N x 2, guide M x N, conf M x N or None.
    history=True returns the list of the outputs of passes 1..passes."""
    out = np.array(flow, dtype=np.float64, order="F")
    M, N, _ = out.shape
    D = 2 * r + 1
    wq = weights(guide, conf, r, sigma_s, sigma_c)
    outs = []
    for _ in range(passes):
        nxt = np.empty_like(out)
        for c in (0, 1):
            b = bits(out[:, :, c])
            P = _pad(b, r, NAN_BITS, np.uint64)
            K = np.stack([key(P[di:di + M, dj:dj + N]) for dj in range(D) for di in range(D)])
            isnan = np.stack([np.isnan(P[di:di + M, dj:dj + N].view(np.float64)) for dj in range(D) for di in range(D)])
            wl = np.where(isnan, 0, wq)  # the live weights
            order = np.argsort(K, axis=0, kind="stable")
            Ks, ws = np.take_along_axis(K, order, axis=0), np.take_along_axis(wl, order, axis=0)
            cum = np.cumsum(ws, axis=0)
            total = cum[-1]
            first = np.argmax((ws > 0) & (2 * cum >= total), axis=0)
            pick = unkey(np.take_along_axis(Ks, first[None], axis=0)[0])
            nxt[:, :, c] = np.where(total == 0, b, pick).view(np.float64)
        out = nxt
        outs.append(out)
    return outs if history else out


# ---- fields shared by the CPU and the GPU tests ---------------------------------------------

def noisy(M, N, seed=0):
    """A flow on a quarter-pixel lattice, so that a window holds equal values."""
    rng = np.random.default_rng(seed)
    return np.asfortranarray(np.round(rng.uniform(-4, 4, (M, N, 2)) * 4) / 4)


def special(M, N, seed=0):
    """noisy() with NaN, +-Inf and +-0 strewn in: about one pixel in eight of each plane."""
    rng = np.random.default_rng(seed + 100)
    f = noisy(M, N, seed)
    what = rng.integers(0, 40, (M, N, 2))
    for code, v in ((0, np.nan), (1, np.inf), (2, -np.inf), (3, 0.0), (4, -0.0)):
        f[what == code] = v
    return f


def guide_of(M, N, seed=0, nans=False):
    """A piecewise-constant image with noise: steps of 60 grey levels every 9 rows and 13 columns."""
    rng = np.random.default_rng(seed + 200)
    m, n = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    g = 60.0 * ((m // 9 + n // 13) % 4) + rng.uniform(0, 12, (M, N))
    if nans:
        g[rng.integers(0, 25, (M, N)) == 0] = np.nan
    return np.asfortranarray(g)


def conf_of(M, N, seed=0, nans=False):
    """Confidences in [0, 1] with exact zeros, values below 2^-16 and, on request, NaN."""
    rng = np.random.default_rng(seed + 300)
    c = rng.uniform(0, 1, (M, N))
    what = rng.integers(0, 20, (M, N))
    c[what == 0] = 0.0
    c[what == 1] = 1e-6
    if nans:
        c[what == 2] = np.nan
    return np.asfortranarray(c)
