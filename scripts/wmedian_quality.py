"""What the weighted median filter does to the flows this library produces:
AEPE (engine.aepe, crop 1, unknown pixels zeroed, as bench.py reports it; a
flow that is still NaN counts as 0, the value block_match_flow starts such a
pixel from) on whole frames before and after flow_wmedian with the first frame
as guide, for

  integer     block_match_init(I1, I2): the integer block-matching start
  refilled    block_match_init(subpixel=True, consistency=True, fill=True)
  bm_flow     block_match_flow(I1, I2): refilled, then denoised
  map         the MAP flow of one C2 solve (bench.py's options: mixture, L = 1,
              K = 9, seed 0, --its iterations), only with --solve (needs a GPU)

each at two settings of the filter (one pass r = 2, sigma_s = 2; three passes
r = 7, sigma_s = 5; sigma_c = 10 both), with the guide on and effectively off
(sigma_c = 1e9) and with the confidence off and on: flow_confidence of the
cost-derived width (integer, refilled), of block_match_flow's width, of the
solve's sigma (s0 = 1, untuned).  A record, not a gate ("Weighted
median filter").  --host runs every stage but the solve on the host models;
the results are bit-identical.

usage: wmedian_quality.py [--pairs rubberwhale Urban3] [--solve] [--its 500] [--host]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", nargs="+", default=["rubberwhale", "Urban3"])
ap.add_argument("--solve", action="store_true")
ap.add_argument("--its", type=int, default=500)
ap.add_argument("--host", action="store_true")
a = ap.parse_args()

if a.solve:
    import torch  # the HIP runtime torch bundles first, as bench.py and the tests load it
    torch.cuda.init()

from gqmap_opticalflow_amd import (Engine, aepe, block_match_flow, block_match_init, flow_confidence,  # noqa: E402
                                   flow_wmedian, load_pair)

def score(flow):
    return aepe(flo, np.nan_to_num(flow, nan=0.0), unk)


SETTINGS = (("1 x r=2 s=2", dict(r=2, sigma_s=2.0, passes=1)), ("3 x r=7 s=5", dict(r=7, sigma_s=5.0, passes=3)))

for name in a.pairs:
    I1, I2, gt = load_pair(name)
    unk = np.any(np.abs(gt) > 1e9, axis=2)  # flowToColor's UNKNOWN_FLOW_THRESH
    flo = np.where(unk[:, :, None], 0.0, gt)
    flows = {}
    flows["integer"] = (block_match_init(I1, I2, host=a.host)[0], None)
    fill, _, sig, _ = block_match_init(I1, I2, subpixel=True, sigma_from_cost=True, consistency=True, fill=True,
                                       host=a.host)
    flows["integer"] = (flows["integer"][0], flow_confidence(sig))
    flows["refilled"] = (fill, flow_confidence(sig))
    mu, sg, _ = block_match_flow(I1, I2, host=a.host)
    flows["bm_flow"] = (mu, flow_confidence(sg))
    if a.solve:
        from bench import gt_options
        opts = gt_options(name, 1, 9)[4]
        with Engine(dict(opts, its=a.its), I1, I2, "mixture", "fp64", device=0) as eng:
            eng.init_state(seed=0)
            done, _ = eng.run(a.its)
            st, mp = eng.get_state(), eng.map()
        flows["map"] = (mp, flow_confidence(np.stack([st.sigu[:, :, 0], st.sigv[:, :, 0]], axis=2)))
        print(f"{name}: solve ran {done} iterations", flush=True)
    M, N = I1.shape
    print(f"{name} {M}x{N}: AEPE before -> after (guide on / off) x (conf off / on)", flush=True)
    for what, (flow, conf) in flows.items():
        share = float(np.mean(np.nan_to_num(conf, nan=0.0)))
        print(f"  {what:9s} before {score(flow):.4f}   NaN {int(np.isnan(flow).sum())}, mean conf {share:.3f}")
        for label, kw in SETTINGS:
            cells = []
            for sigma_c in (10.0, 1e9):
                for c in (None, conf):
                    out = flow_wmedian(flow, I1, sigma_c=sigma_c, conf=c, host=a.host, **kw)
                    cells.append(f"{score(out):.4f}")
            print(f"    {label}: guide on {cells[0]} (conf {cells[1]}), guide off {cells[2]} (conf {cells[3]})", flush=True)
