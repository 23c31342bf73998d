"""The case table of the option-range tests (tests/test_wide_options.py on the
CPU, tests/test_gpu_wide_options.py on the device): gqmap_create takes L in
[1, GQMAP_LMAX = 8] and K in [2, GQMAP_KMAX = 16]; the table walks that range
at every lanes-per-node count Q the engines take.

Options are tests/test_small_grids.small_case's (alpha update from iteration
10, temperature decay every 20) on larger crops:

  mixture, ctf   36 x 42 nodes.  At Q = 1 3 x 3 tiles of 16 x 16: the last tile
                 row holds 4 node rows (the grouped dataflow item), the last
                 tile column 10 node columns.  Ragged on at least one axis at
                 every tile shape (test_frames_have_the_tiles_they_are_for).
  super          a 48 x 72 image, 12 x 18 nodes: 1 x 2 partial tiles at Q = 1
                 (the second holds 2 node columns), 2 x 3 tiles at Q = 4,
                 3 x 5 at Q = 16, each with a ragged edge.

K = 2 carries no sigma gradient from the potentials (two Gauss-Hermite nodes:
ptdsigma ~ 1e-15 at temperature 0, test_two_point_rule_has_no_sigma_gradient;
only the entropy term T / sigma is left), so K = 3 stands beside it as the
smallest K that exercises the sigma update.  K = 16 fills the quadrature
table exactly (K^2 = 256 = TAB_STRIDE); only the fp64 cases resolve its last
point, whose weight (~1e-19 of the sum) is below fp32 rounding.  K = 2 at
Q >= 8, K = 3 at Q >= 16 and K = 4 at Q = 64 leave lanes of a node without a
sample (K^2 < Q).

Lanes per node: every one the engine takes for mixture (8,16), mixture (1,16),
ctf (1,16) and super (8,16); Q = 8, 16, 64 for every K = 2 and K = 3 case of
mixture and ctf, mixture (8,3) included (lanes without a sample together
with the NFIX + 8 sums and the 8-weight alpha update); Q = 1, 4, 64 (super:
1, 16) for the rest."""
import dataclasses

import numpy as np

from tests.test_small_grids import small_case

ITS = 40
ROLE = -1  # GQMAP_SPLIT_ROLE: the Q = 1 arithmetic on 16 x 8 tiles
FRAME = (36, 42)
SUPER_FRAME = (48, 72)
ALL_SPLITS = [1, 2, 4, 8, 16, 64, ROLE]
SUPER_SPLITS = [1, 4, 16]
# rows x cols of a tile in nodes, per lanes per node (tests/test_gpu_small_grids.py)
TILE = {1: (16, 16), 2: (16, 8), ROLE: (16, 8), 4: (8, 8), 8: (8, 4), 16: (4, 4), 64: (5, 1)}

CASES = [("mixture", 2, 4), ("mixture", 4, 6), ("mixture", 5, 13), ("mixture", 8, 16), ("mixture", 8, 3),
         ("mixture", 1, 16), ("mixture", 1, 4), ("mixture", 1, 3), ("mixture", 1, 2),
         ("super", 2, 5), ("super", 4, 4), ("super", 8, 16), ("super", 8, 3),
         ("ctf", 1, 16), ("ctf", 1, 12), ("ctf", 1, 4), ("ctf", 1, 3), ("ctf", 1, 2)]
EVERY_SPLIT = [("mixture", 8, 16), ("mixture", 1, 16), ("ctf", 1, 16), ("super", 8, 16)]


def frame(engine):
    return SUPER_FRAME if engine == "super" else FRAME


def nodes(engine):
    M, N = frame(engine)
    return (M // 4, N // 4) if engine == "super" else (M, N)


def splits(engine, L, K):
    """The lanes per node the table runs a case at."""
    if (engine, L, K) in EVERY_SPLIT:
        return SUPER_SPLITS if engine == "super" else ALL_SPLITS
    if engine == "super":
        return [1, 16]
    if K <= 3:  # mixture and ctf, every L: mixture (8, 3) too
        return [8, 16, 64]  # K = 2: lanes without a sample at all three; K = 3: at 16 and 64
    return [1, 4, 64]


TABLE = [(e, L, K, q) for e, L, K in CASES for q in splits(e, L, K)]


def case(engine, L, K, split=None, **extra):
    """Frames, options and seeded initial state (small_case at the table's frame)."""
    if split is not None:
        extra["split"] = split
    return small_case(engine, L, K, *frame(engine), **extra)


# ---- exact zero weights --------------------------------------------------------
# The `if a ~= 0` guard (options guard_a) only branches where a weight is
# exactly 0.  projsplx keeps such a weight at 0 when it starts there, and
# drives weights to 0 by itself with a large enough alpha_lr.

ZERO_K = 4
ZERO_SPLIT = {"mixture": 1, "super": 4}
ZERO_CASES = [(e, L, g) for e in ("mixture", "super") for L in (4, 8) for g in (0, 1)]
ZEROING = ("super", 8, 4)  # with ZEROING_OPTS: weights reach exactly 0 by themselves
ZEROING_OPTS = dict(alpha_mode=1, alpha_lr=1e-3)
ZEROING_SPLIT = 4


def zero_alpha(L):
    a = np.zeros(L)
    a[0], a[2] = 0.625, 0.375
    return a


def zero_weight_case(engine, L, guard_a, split=None):
    """A projsplx case whose state starts with alpha = [0.625, 0, 0.375, 0, ...]."""
    I1, I2, o, st = case(engine, L, ZERO_K, ZERO_SPLIT[engine] if split is None else split,
                         alpha_mode=1, guard_a=guard_a)
    return I1, I2, o, dataclasses.replace(st, alpha=zero_alpha(L))


def zeroing_case(split=ZEROING_SPLIT):
    return case(*ZEROING, split, **ZEROING_OPTS)
