"""Shared input of the flow-seeded-init tests (CPU and GPU)."""
import numpy as np


def make_flow(M, N, seed=0, amp=4.0):
    """A flow wider than any test range, with NaN and .flo-unknown entries."""
    rng = np.random.default_rng(seed)
    f = np.asfortranarray(rng.uniform(-amp, amp, (M, N, 2)))
    f[1, 2, 0] = np.nan
    f[M - 1, N - 1, 1] = np.nan
    f[2, 1, 0] = 1e10
    f[0, 0, 1] = -1e10
    f[3, 3] = (1.666666666e9, 0.25)  # the .flo mark itself
    return f
