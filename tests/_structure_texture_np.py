"""numpy restatement of the structure-texture preprocessing (ROF decomposition
by Chambolle's dual projection), written from the specification in
csrc/gqmap_rof.h / DESIGN.md, independent of the library.

fp64 element-wise numpy: every +, -, *, /, sqrt and maximum is one correctly
rounded IEEE operation, nothing is contracted, so the order written here IS
the arithmetic.  m = row (axis 0), n = column (axis 1), planes on axis 2.
"""
import numpy as np


def _div(p1, p2):
    """d(m,n) = (p1(m,n) - p1(m,n-1)) + (p2(m,n) - p2(m-1,n)), p = +0 outside."""
    w = np.zeros_like(p1)
    w[:, 1:] = p1[:, :-1]
    n = np.zeros_like(p2)
    n[1:, :] = p2[:-1, :]
    return (p1 - w) + (p2 - n)


def structure_texture_np(im, theta=0.125, n_iter=100, alp=0.95):
    """Returns (texture in [0, 255], structure in the [-1, 1] domain), both
    M x N x C.  Raises ValueError where the library returns INVALID_ARG for a
    zero or non-finite range."""
    im = np.asarray(im, dtype=np.float64)
    if im.ndim == 2:
        im = im[:, :, None]
    theta, alp = np.float64(theta), np.float64(alp)
    lo, hi = im.min(), im.max()
    if not (np.isfinite(im).all() and hi - lo > 0 and np.isfinite(hi - lo)):
        raise ValueError("structure_texture: zero or non-finite input range")
    x = ((im - lo) / (hi - lo)) * 2.0 + (-1.0)
    delta = np.float64(1.0) / (np.float64(4.0) * theta)
    p1 = np.zeros_like(x)
    p2 = np.zeros_like(x)
    for _ in range(n_iter):
        u = x + theta * _div(p1, p2)
        ix = np.zeros_like(u)
        ix[:, :-1] = u[:, 1:] - u[:, :-1]
        iy = np.zeros_like(u)
        iy[:-1, :] = u[1:, :] - u[:-1, :]
        q1 = p1 + delta * ix
        q2 = p2 + delta * iy
        r = np.maximum(1.0, np.sqrt(q1 * q1 + q2 * q2))
        p1 = q1 / r
        p2 = q2 / r
    s = x + theta * _div(p1, p2)
    t = x - alp * s
    tlo, thi = t.min(), t.max()
    if not (np.isfinite(t).all() and thi - tlo > 0 and np.isfinite(thi - tlo)):
        raise ValueError("structure_texture: zero or non-finite texture range")
    texture = ((t - tlo) / (thi - tlo)) * 255.0 + 0.0
    return texture, s


# ---- shared by tests/test_structure_texture.py and tests/test_gpu_structure_texture.py ----
import functools  # noqa: E402

PARAMS = ((0.125, 0.95), (0.1, 0.7))  # (theta, alp): the reference's, and one where theta*d is inexact


def random_frames(shape, C, seed=0):
    """Seeded frames in the greyscale range, M x N x C column-major (not integer-valued)."""
    rng = np.random.default_rng([seed, shape[0], shape[1], C])
    return np.asfortranarray(rng.uniform(0.0, 255.0, size=tuple(shape) + (C,)))


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@functools.lru_cache(maxsize=None)
def rubberwhale_np():
    """(im, texture, structure) of the restatement on the full RubberWhale pair, computed once."""
    from gqmap_opticalflow_amd import load_pair
    I1, I2, _ = load_pair("rubberwhale")
    im = np.asfortranarray(np.stack([I1, I2], axis=2))
    tex, s = structure_texture_np(im)
    for a in (im, tex, s):
        a.setflags(write=False)
    return im, tex, s


def bad_cases():
    """name -> (im, overridden arguments): calls the library refuses with INVALID_ARG."""
    ok = random_frames((4, 5), 2)
    nan = ok.copy(order="F")
    nan[1, 2, 1] = np.nan
    return {
        "constant": (np.full((4, 5, 2), 3.0, order="F"), {}),
        "nan": (nan, {}),
        "theta0": (ok, dict(theta=0.0)),
        "C9": (random_frames((4, 5), 9), {}),
        "M0": (ok, dict(M=0)),
    }
