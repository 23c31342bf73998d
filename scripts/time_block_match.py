"""Kernel time of gqmap_block_match (HIP events, copies excluded) on a
RubberWhale frame pair: median of --runs timed calls after a warm-up that keeps
the GPU busy for --settle seconds (at least one call), so the clock has ramped.
Beside it the achieved fraction of the 78.6 TF fp64 vector peak, from the
flops of the separable form per pixel and displacement: (2ft+1) x (subtract,
multiply, add) in the row pass + (2ft+1) x (multiply, add) in the column pass
(the row pass repeated in a tile's column halo is not counted).

--hypotheses H times gqmap_block_match_multi (H ranks, separation --sep)
instead; its flops are H times the single pass (the exclusion test is integer
work and not counted).  --subpixel times gqmap_block_match_refine (H ranks,
default 1): H + 1 scans, so the expectation is (H + 1) / H of the multi time at
the same H; the flops counted are those of the H + 1 scans
(profiles/block_match_refine_times.txt).

--against PATH loads a second libgqmap.so beside this tree's (the parent
commit's, built into a directory outside the tree) and times the same call on
both in this one process: --rounds rounds in alternating order, each library
per round a --settle warm-up and then --runs timed calls.  It prints each
library's round medians, the median of them, and whether the two libraries'
outputs are bit-identical (profiles/block_match_unified_times.txt).

usage: time_block_match.py [--scale S] [--U U] [--V V] [--ft FT] [--sigma SG] [--runs R] [--cols 0|8|16|32]
                           [--hypotheses H] [--sep S] [--subpixel] [--against PATH [--rounds N]]
  issue cases: (a) --scale 1 --U 7;  (b) --scale 4 --U 25"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gqmap_opticalflow_amd import _lib, block_match, imresize, load_pair  # noqa: E402

PEAK_FP64 = 78.6e12

ap = argparse.ArgumentParser()
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--U", type=int, default=7)
ap.add_argument("--V", type=int, default=None)
ap.add_argument("--ft", type=int, default=3)
ap.add_argument("--sigma", type=float, default=1.7)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--settle", type=float, default=0.5)
ap.add_argument("--cols", type=int, default=0, help="force the tile width (0: the library's choice)")
ap.add_argument("--hypotheses", type=int, default=None, help="H ranks through gqmap_block_match_multi")
ap.add_argument("--sep", type=int, default=2)
ap.add_argument("--subpixel", action="store_true", help="gqmap_block_match_refine: H + 1 scans")
ap.add_argument("--against", default=None, metavar="PATH", help="a second libgqmap.so to time beside this tree's")
ap.add_argument("--rounds", type=int, default=3, help="alternating rounds with --against")
a = ap.parse_args()
V = a.U if a.V is None else a.V

I1, I2, _ = load_pair("rubberwhale")
if a.scale != 1:
    I1, I2 = imresize(I1, a.scale), imresize(I2, a.scale)
M, N = I1.shape


def load_library(path=None):
    """This tree's libgqmap.so, or the one at path, with the tile width forced."""
    if path is not None:
        _lib._lib, _lib.LIB_PATH = None, path
    lib = _lib.load()
    f = lib.gqmap_debug_block_match_cols
    f.restype, f.argtypes = C.c_int, [C.c_int]
    assert f(a.cols) == 0
    return lib


def call(lib):
    _lib._lib = lib  # the library block_match runs on
    return block_match(I1, I2, a.U, V, a.ft, a.sigma, timed=True, hypotheses=a.hypotheses, sep=a.sep,
                       subpixel=a.subpixel)


def timed_runs(lib):
    t0, warm = time.perf_counter(), []
    while not warm or time.perf_counter() - t0 < a.settle:
        warm.append(call(lib)[-1])
    return warm, [call(lib)[-1] for _ in range(a.runs)]


what = "block_match" if a.hypotheses is None else f"block_match_multi H={a.hypotheses} sep={a.sep}"
if a.subpixel:
    what = f"block_match_refine H={a.hypotheses or 1} sep={a.sep}"
what += f" {M}x{N} U={a.U} V={V} ft={a.ft} sigma={a.sigma} cols={a.cols or 'auto'}"
mine = load_library()
if a.against is None:
    warm, ms = timed_runs(mine)
    med = statistics.median(ms)
    scans = (a.hypotheses or 1) + (1 if a.subpixel else 0)
    flops = float(M) * N * (2 * a.U + 1) * (2 * V + 1) * (2 * a.ft + 1) * 5 * scans
    print(f"{what}: warm-up {len(warm)} calls (first {warm[0]:.3f} ms), runs " + " ".join(f"{x:.3f}" for x in ms) +
          f" ms, median {med:.3f} ms, {flops / 1e9:.2f} GFLOP, {flops / (med * 1e-3) / 1e12:.2f} TF/s = "
          f"{100 * flops / (med * 1e-3) / PEAK_FP64:.1f}% of the fp64 vector peak", flush=True)
    sys.exit(0)

libs = {"this tree": mine, "against": load_library(os.path.abspath(a.against))}
same = all(np.array_equal(x.view(np.uint64), y.view(np.uint64))
           for x, y in zip(call(libs["this tree"])[:-1], call(libs["against"])[:-1]))
meds = {k: [] for k in libs}
for r in range(a.rounds):
    for k in list(libs)[::1 if r % 2 == 0 else -1]:
        meds[k].append(statistics.median(timed_runs(libs[k])[1]))
        print(f"{what}: round {r} {k}: median of {a.runs} {meds[k][-1]:.3f} ms", flush=True)
mid = {k: statistics.median(v) for k, v in meds.items()}
print(f"{what}: medians of {a.rounds} round medians: " +
      ", ".join(f"{k} {mid[k]:.3f} ms (rounds {min(v):.3f}..{max(v):.3f})" for k, v in meds.items()) +
      f"; this tree / against {mid['this tree'] / mid['against']:.4f}; this tree not above the slowest round of "
      f"against: {mid['this tree'] <= max(meds['against'])}; outputs bit-identical: {same}", flush=True)
