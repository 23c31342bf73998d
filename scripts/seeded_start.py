"""Does a solve started from block matching converge faster or further than one
started at random?  Full RubberWhale, mixture engine with the optical_flow.m
options (L = 3, K = 9, lambdas = 5, lambdad = 1, fp64), the range taken from
block_match_init for every start, one seed throughout.  The starts:
  random   gqmap_init_state
  seed-1   component 0 from the block-matching argmin
  seed-3   components 0..2 from the three best separated displacements (--sep)
  sub-3    as seed-3 with the sub-pixel flows (block_match_init(subpixel=True))
  sub-3+s  as sub-3 with sigma of those components from the cost's curvature
           (sigma_from_cost=True, lambdad of the options, --sigma-min)
  fb-3+s   as sub-3+s after the forward-backward check (consistency=True): a
           rank that fails it keeps the random draw, mean and sigma
  fbf-3+s  as fb-3+s with rank 0 of the rejected pixels refilled from the
           consistent ones around them (fill=True; sigma there stays the draw)
AEPE (against the .flo ground truth, which no start sees) and Energy at
iterations 1, 300, 600, ... (profiles/block_match_multi_start.txt for the
first three, profiles/block_match_refine_start.txt with five,
profiles/block_match_fb_start.txt with all seven).

usage: seeded_start.py [--its 3000] [--every 300] [--seed 0] [--sep 2] [--sigma-min 0.5] [--pair rubberwhale]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gqmap_opticalflow_amd import block_match_init, flow_to_color, gqmap_gpu_mixture, load_pair  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--its", type=int, default=3000)
ap.add_argument("--every", type=int, default=300)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--sep", type=int, default=2)
ap.add_argument("--sigma-min", type=float, default=0.5)
ap.add_argument("--pair", default="rubberwhale")
a = ap.parse_args()

I1, I2, gt = load_pair(a.pair)
_, flo, _, unk = flow_to_color(gt)
flow3, ranges = block_match_init(I1, I2, hypotheses=3, sep=a.sep)
flow1, _ = block_match_init(I1, I2)
assert np.array_equal(flow1, flow3[..., 0])
sub3, _, sig3 = block_match_init(I1, I2, hypotheses=3, sep=a.sep, subpixel=True, sigma_from_cost=True, lambdad=1.0,
                                 sigma_min=a.sigma_min)
fb3, _, fbsig, cons = block_match_init(I1, I2, hypotheses=3, sep=a.sep, subpixel=True, sigma_from_cost=True, lambdad=1.0,
                                       sigma_min=a.sigma_min, consistency=True)
fbf3, _, fbfsig, cons2 = block_match_init(I1, I2, hypotheses=3, sep=a.sep, subpixel=True, sigma_from_cost=True,
                                          lambdad=1.0, sigma_min=a.sigma_min, consistency=True, fill=True)
assert np.array_equal(cons, cons2) and np.array_equal(fbsig, fbfsig, equal_nan=True)
opts = dict(trueFlow=flo, unknownIdx=unk, its=a.its, K=9, L=3, temperature=0.0, drate=0.5, epsn=0.001 ** 2,
            lambdas=5.0, lambdad=1.0, **ranges)
M, N = I1.shape
print(f"{a.pair} {M}x{N} mixture L=3 K=9 lambdas=5 lambdad=1 fp64, range {ranges}, seed {a.seed}, sep {a.sep}; "
      f"{int(np.isnan(flow3[:, :, 0, 1:]).sum())} missing rank entries", flush=True)
known = ~np.asarray(unk, dtype=bool)
for name, f in (("integer", flow1), ("sub-pixel", sub3[..., 0])):
    print(f"raw rank-0 {name} flow: known-pixel AEPE {np.sqrt(np.sum((flo - f) ** 2, axis=2))[known].mean():.5f}")
print(f"sigma from the cost (floor {a.sigma_min}): {100 * np.isnan(sig3).mean():.2f}% not refinable (keep the draw), "
      f"{100 * np.mean(sig3[~np.isnan(sig3)] == a.sigma_min):.1f}% of the rest at the floor, percentiles 1/50/99 "
      + "/".join(f"{x:.3f}" for x in np.nanpercentile(sig3, (1, 50, 99))), flush=True)
epe0 = np.sqrt(np.sum((flo - sub3[..., 0]) ** 2, axis=2))
ok0 = cons[:, :, 0]
print("forward-backward check (a1 0.01, a2 0.5): consistent share per rank " +
      " ".join(f"{cons[:, :, k].mean():.4f}" for k in range(3)) +
      f"; rank-0 known-pixel AEPE consistent {epe0[known & ok0].mean():.5f}, rejected {epe0[known & ~ok0].mean():.5f}, "
      f"refilled start {np.sqrt(np.sum((flo - fbf3[..., 0]) ** 2, axis=2))[known].mean():.5f} "
      f"({int(np.isnan(fbf3[:, :, 0, 0]).sum())} pixels left unfilled)", flush=True)
marks = [1] + list(range(a.every, a.its + 1, a.every))
rows = {}
for name, init, sig in (("random", None, None), ("seed-1", flow1, None), ("seed-3", flow3, None),
                        ("sub-3", sub3, None), ("sub-3+s", sub3, sig3), ("fb-3+s", fb3, fbsig),
                        ("fbf-3+s", fbf3, fbfsig)):
    _, _, _, AEPE, Energy, _ = gqmap_gpu_mixture(opts, I1, I2, seed=a.seed, init_flow=init, init_sigma=sig,
                                                 eval_every=a.every)
    rows[name] = (AEPE, Energy)
    print(f"{name}: done", flush=True)
print(f"{'it':>5s} " + " ".join(f"{n + ' AEPE':>12s} {n + ' Energy':>16s}" for n in rows))
for it in marks:
    print(f"{it:5d} " + " ".join(f"{r[0][it - 1]:12.5f} {r[1][it - 1]:16.8e}" for r in rows.values()), flush=True)
