"""Kernel time of gqmap_structure_texture (HIP events, copies excluded) on the
RubberWhale frame pair (M x N x 2) at every forced T (iterations per launch:
1 = the plain kernel, 2, 4, 8 = the fused LDS-tile kernel): per T the median of
--runs timed calls after a warm-up that keeps the GPU busy for --settle seconds
(at least one call), so the clock has ramped.  spread = max - min of the runs.
Beside it the rate in pixel-iterations per second and, from the estimate of 50
fp64 VALU operations per pixel-iteration, the fraction of the 78.6 TF fp64
vector peak (a multiply-add counts 2 there, so ops / (peak / 2) is an upper
bound on the achieved fraction; the halo repeats of the fused form are not
counted as work).

usage: time_structure_texture.py [--scale S ...] [--n-iter K] [--runs R] [--T 1 2 4 8]
  issue cases: --scale 1 4  (388 x 584 x 2 and 1552 x 2336 x 2, 100 iterations)"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gqmap_opticalflow_amd import _lib, imresize, load_pair, structure_texture  # noqa: E402

PEAK_FP64 = 78.6e12
OPS = 50  # fp64 VALU operations per pixel-iteration (DESIGN, structure-texture subsection)

ap = argparse.ArgumentParser()
ap.add_argument("--scale", type=float, nargs="+", default=[1.0, 4.0])
ap.add_argument("--n-iter", type=int, default=100)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--settle", type=float, default=0.5)
ap.add_argument("--T", type=int, nargs="+", default=[1, 2, 4, 8])
a = ap.parse_args()

lib = _lib.load()
force = lib.gqmap_debug_rof_T
force.restype, force.argtypes = C.c_int, [C.c_int]
lib.gqmap_debug_rof_default_T.restype = C.c_int
print(f"default T = {lib.gqmap_debug_rof_default_T()}", flush=True)

I1, I2, _ = load_pair("rubberwhale")
for scale in a.scale:
    A, B = (I1, I2) if scale == 1 else (imresize(I1, scale), imresize(I2, scale))
    im = np.asfortranarray(np.stack([A, B], axis=2))
    M, N, Cn = im.shape
    work = float(M) * N * Cn * a.n_iter
    for T in a.T:
        assert force(T) == 0
        t0, warm = time.perf_counter(), []
        while not warm or time.perf_counter() - t0 < a.settle:
            warm.append(structure_texture(im, n_iter=a.n_iter, timed=True)[1])
        ms = [structure_texture(im, n_iter=a.n_iter, timed=True)[1] for _ in range(a.runs)]
        med = statistics.median(ms)
        print(f"structure_texture {M}x{N}x{Cn} n_iter={a.n_iter} T={T}: warm-up {len(warm)} calls "
              f"(first {warm[0]:.3f} ms), runs " + " ".join(f"{x:.3f}" for x in ms) +
              f" ms, median {med:.3f} ms, spread {max(ms) - min(ms):.3f} ms, "
              f"{work / (med * 1e-3) / 1e9:.2f} Gpx-it/s, "
              f"{100 * work * OPS / (med * 1e-3) / (PEAK_FP64 / 2):.1f}% of the fp64 vector issue peak", flush=True)
    force(0)
