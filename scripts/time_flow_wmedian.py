"""Kernel time of gqmap_flow_wmedian (HIP events, copies excluded) on the full
RubberWhale frame: the sub-pixel block-matching flow of the pair, frame 1 as
guide, at r = 2, 4, 8 (sigma_s = r / 2 + 1, sigma_c = 10) and passes = 1, 3,
without a confidence map and, at one pass, with flow_confidence of the
cost-derived widths.  Every entry is the median of --runs timed calls after a
warm-up that keeps the GPU busy for --settle seconds (at least one call).

Beside each time the work of the selection, pixels x passes x 2 planes x
(2r+1)^2 entries, as entries per second, and the bytes the launches must move,
every array once, no halo (flow 16 + guide 8 [+ conf 8] read, flow 16 written
per pixel and pass).  The kernel is bound by the selection, not by those bytes.
gqmap_flow_fill at its defaults (r = 8, two passes) on the same flow and the
forward-backward mask stands beside it for scale.  There is no parent kernel:
the numbers are a record, not a target (profiles/flow_wmedian_times.txt).

usage: time_flow_wmedian.py [--runs 5] [--settle 0.5]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gqmap_opticalflow_amd import (block_match_init, flow_confidence, flow_consistency, flow_fill, flow_wmedian,  # noqa: E402
                                   load_pair)

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--settle", type=float, default=0.5)
a = ap.parse_args()


def median_ms(call):
    t0, warm = time.perf_counter(), []
    while not warm or time.perf_counter() - t0 < a.settle:
        warm.append(call()[-1])
    ms = [call()[-1] for _ in range(a.runs)]
    return statistics.median(ms), ms, len(warm)


def report(what, entries, nbytes, call):
    med, ms, warm = median_ms(call)
    rate = f"{entries / (med * 1e-3) / 1e9:.1f} G entries/s, " if entries else ""
    print(f"{what}: warm-up {warm} calls, runs " + " ".join(f"{x:.4f}" for x in ms) + f" ms, median {med:.4f} ms; "
          f"{rate}{nbytes / 1e6:.2f} MB, {nbytes / (med * 1e-3) / 1e12:.3f} TB/s", flush=True)


I1, I2, _ = load_pair("rubberwhale")
fwd, _, sig = block_match_init(I1, I2, subpixel=True, sigma_from_cost=True)
bwd = block_match_init(I2, I1, subpixel=True)[0]
M, N, _ = fwd.shape
mask = flow_consistency(fwd, bwd)[1]
conf = flow_confidence(sig)
print(f"frame {M}x{N}", flush=True)
report(f"{M}x{N} fill r=8 passes=2 (for scale)", 0, 34 * 2 * M * N, lambda: flow_fill(fwd, mask, 8, 4.0, 2, timed=True))
for r in (2, 4, 8):
    for passes, c in ((1, None), (3, None), (1, conf)):
        entries = M * N * passes * 2 * (2 * r + 1) ** 2
        nbytes = (40 if c is None else 48) * passes * M * N
        report(f"{M}x{N} wmedian r={r} passes={passes}{'' if c is None else ' conf'}", entries, nbytes,
               lambda: flow_wmedian(fwd, I1, r, r / 2 + 1, 10.0, passes, c, timed=True))
