"""What the GPU tests of the block matcher share (tests/test_gpu_block_match*.py):
device against host model bit for bit, the forced tile width, and the small
engine problems of the seeded inits."""
import ctypes as C

import numpy as np

from tests import _golden as G
from tests._initflow import make_flow

KEYS = G.STATE_KEYS
NAN_BITS = 0x7FF8000000000000


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def both(A, B, params, **kw):
    """(device, host model) results of one block_match call."""
    from gqmap_opticalflow_amd import block_match
    return block_match(A, B, *params, **kw), block_match(A, B, *params, host=True, **kw)


def assert_bit_equal(dev, host):
    """(flow, cost) or (flow, cost, curv) tuples, entry by entry as bit patterns."""
    assert len(dev) == len(host) and len(dev) in (2, 3)
    for d, h, what in zip(dev, host, ("flow", "cost", "curv")):
        assert d.shape == h.shape
        diff = bits(d) != bits(h)
        assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} entries differ"


def force_cols(cols):
    from gqmap_opticalflow_amd import _lib
    f = _lib.load().gqmap_debug_block_match_cols
    f.restype, f.argtypes = C.c_int, [C.c_int]
    assert f(cols) == 0


# ---- gqmap_init_state_flows / gqmap_init_state_seeded ---------------------------

def problem(engine):
    """Golden frames and options (tests/test_gpu_init_flow.py), L = 3: the
    mixture cases on a 24 x 20 corner, the super case on a 32 x 32 corner
    (node grid 8 x 8).  The golden ranges (about [-1.6, 1.4]) are
    narrower than make_flow's [-4, 4], so clamping happens."""
    d = G.load("super_L3")
    if engine == "super":
        I1, I2 = (np.asfortranarray(d[k][:32, :32]) for k in ("I1", "I2"))
        return I1, I2, dict(d["opts"], L=3), (8, 8)
    o = dict(G.load("mixture_L3_T")["opts"], L=3)
    I1, I2 = (np.asfortranarray(d[k][:24, :20]) for k in ("I1", "I2"))
    return I1, I2, o, (24, 20)


def flows(M, N, H, seed):
    f = np.asfortranarray(np.stack([make_flow(M, N, seed=seed + h) for h in range(H)], axis=3))
    if H > 1:
        f[5, 4, :, 1] = np.nan  # a missing rank
    return f


def as_fp32(st):
    for k in KEYS[:6]:
        setattr(st, k, np.asfortranarray(getattr(st, k).astype(np.float32).astype(np.float64)))
    return st


def assert_state_equal(a, b, what=""):
    for k in KEYS:
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=f"{what} {k}")
    assert a.it == b.it and a.T == b.T
