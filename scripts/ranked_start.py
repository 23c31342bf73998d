"""Does a start seeded by the ranked coarse-to-fine matcher help a solve whose
motions are out of the plain matcher's reach?  Urban3, super engine with the C4
options of bench.py (L = 3, K = 11, temperature 0.2, drate 0.75, lambdas 16,
lambdad 1, fp64), one seed and one range (+-block_match_reach) throughout.  The
starts, in the manner of scripts/seeded_start.py:
  random     gqmap_init_state
  pyr-1      component 0 from block_match_init(levels=3, U=V=20)
  pyr-3      components 0..2 from the same with hypotheses=3, pyr_ranked=True
AEPE (against the .flo ground truth, which no start sees) and Energy at
iterations 1, --every, 2 --every, ... (profiles/block_match_ranked_start.txt).

usage: ranked_start.py [--its 3000] [--every 300] [--seed 0] [--sep 2] [--pair Urban3] [--U 20] [--levels 3]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gqmap_opticalflow_amd import block_match_init, flow_to_color, gqmap_gpuSuper_mix_entropy, load_pair  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--its", type=int, default=3000)
ap.add_argument("--every", type=int, default=300)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--sep", type=int, default=2)
ap.add_argument("--pair", default="Urban3")
ap.add_argument("--U", type=int, default=20)
ap.add_argument("--levels", type=int, default=3)
a = ap.parse_args()

I1, I2, gt = load_pair(a.pair)
_, flo, _, unk = flow_to_color(gt)
known = ~np.asarray(unk, dtype=bool)
kw = dict(U=a.U, V=a.U, levels=a.levels)
pix1, ranges = block_match_init(I1, I2, **kw)
pix3, _ = block_match_init(I1, I2, hypotheses=3, sep=a.sep, pyr_ranked=True, **kw)
assert np.array_equal(pix1, pix3[..., 0])
epe = np.stack([np.sqrt(np.sum((flo - pix3[..., j]) ** 2, axis=2)) for j in range(3)])
epe = np.where(np.isnan(epe), np.inf, epe)
node1, _ = block_match_init(I1, I2, engine="super", **kw)
node3, _ = block_match_init(I1, I2, engine="super", hypotheses=3, sep=a.sep, pyr_ranked=True, **kw)
M, N = I1.shape
print(f"{a.pair} {M}x{N} super L=3 K=11 T=0.2 drate=0.75 lambdas=16 lambdad=1 fp64, U=V={a.U} levels={a.levels} r=1 k=1, "
      f"range {ranges}, seed {a.seed}, sep {a.sep}; {int(np.isnan(pix3[:, :, 0, 1:]).sum())} missing rank entries on the "
      f"pixel grid, {int(np.isnan(node3[:, :, 0, 1:]).sum())} on the node grid", flush=True)
print(f"raw integer flow on the pixel grid, known-pixel AEPE: rank 0 {epe[0][known].mean():.5f}, best of 3 ranks "
      f"{epe.min(axis=0)[known].mean():.5f}", flush=True)
opts = dict(trueFlow=flo, unknownIdx=unk, its=a.its, K=11, L=3, temperature=0.2, drate=0.75, epsn=0.001 ** 2,
            lambdas=16.0, lambdad=1.0, **ranges)
marks = [1] + list(range(a.every, a.its + 1, a.every))
rows = {}
for name, init in (("random", None), ("pyr-1", node1), ("pyr-3", node3)):
    _, _, _, AEPE, Energy, _ = gqmap_gpuSuper_mix_entropy(opts, I1, I2, seed=a.seed, init_flow=init, eval_every=a.every)
    rows[name] = (AEPE, Energy)
    print(f"{name}: done", flush=True)
print(f"{'it':>5s} " + " ".join(f"{n + ' AEPE':>12s} {n + ' Energy':>16s}" for n in rows))
for it in marks:
    print(f"{it:5d} " + " ".join(f"{r[0][it - 1]:12.5f} {r[1][it - 1]:16.8e}" for r in rows.values()), flush=True)
