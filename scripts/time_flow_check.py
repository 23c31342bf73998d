"""Kernel time of gqmap_flow_consistency and gqmap_flow_fill (HIP events, copies
excluded) on the RubberWhale flows: the sub-pixel block-matching flow of the
pair in both directions at full size, and the same two fields repeated 4 x 4
and scaled by 4 (a 1552 x 2336 frame with the same geometry, no second match).
The fill runs on the check's own mask at r = 4, 8, 16 (sigma = r / 2) and
passes = 1, 2.  Every entry is the median of --runs timed calls after a warm-up
that keeps the GPU busy for --settle seconds (at least one call).

Beside each time the bytes the launches must move, every array once, no halo:
  check   fwd 16 + the bwd samples 16 + err 8 + mask 1        = 41 B per pixel
  fill    per pass flow 16 + state 1 read, the same written   = 34 B per pixel
and the floor those bytes set at the 6.29 TB/s a streaming copy reaches on the
MI355X.  There is no parent kernel: the numbers are a record, not a target
(profiles/flow_check_times.txt).

usage: time_flow_check.py [--runs 5] [--settle 0.5]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gqmap_opticalflow_amd import block_match_init, flow_consistency, flow_fill, load_pair  # noqa: E402

COPY_RATE = 6.29e12  # B/s

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


def report(what, nbytes, call):
    med, ms, warm = median_ms(call)
    floor = nbytes / COPY_RATE * 1e3
    print(f"{what}: warm-up {warm} calls, runs " + " ".join(f"{x:.4f}" for x in ms) + f" ms, median {med:.4f} ms; "
          f"{nbytes / 1e6:.2f} MB, floor {floor:.4f} ms, {med / floor:.1f} x the floor, "
          f"{nbytes / (med * 1e-3) / 1e12:.3f} TB/s", flush=True)


I1, I2, _ = load_pair("rubberwhale")
fwd = block_match_init(I1, I2, subpixel=True)[0]
bwd = block_match_init(I2, I1, subpixel=True)[0]
up = lambda f: np.asfortranarray(4.0 * np.repeat(np.repeat(f, 4, axis=0), 4, axis=1))
for name, f, b in (("full", fwd, bwd), ("4x", up(fwd), up(bwd))):
    M, N, _ = f.shape
    mask = flow_consistency(f, b)[1]
    print(f"{name} frame {M}x{N}: consistent share {mask.mean():.4f}", flush=True)
    report(f"{name} {M}x{N} check", 41 * M * N, lambda: flow_consistency(f, b, timed=True))
    for r in (4, 8, 16):
        for passes in (1, 2):
            left = int((flow_fill(f, mask, r, r / 2, passes)[1] == 255).sum())
            report(f"{name} {M}x{N} fill r={r} passes={passes} ({left} pixels left)", 34 * passes * M * N,
                   lambda: flow_fill(f, mask, r, r / 2, passes, timed=True))
