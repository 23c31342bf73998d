"""Kernel time of gqmap_block_match_pyramid (HIP events over all kernels of the
call, copies excluded) on a RubberWhale frame pair, beside the full search of
the same U, V (gqmap_block_match, with --subpixel gqmap_block_match_refine at
H = 1): median of --runs timed calls after a warm-up that keeps the GPU busy for
--settle seconds (at least one call), so the clock has ramped.

Per level it prints what the library's counters say (gqmap_debug_block_match_stats,
one extra call with counting on, not among the timed ones): the time of the
level's kernels, the mean box area per pixel, and the mean number of
displacements a tile evaluated in its first walk -- the union of its pixels'
boxes after skipping, the quantity to look at when the time disappoints.

--against PATH loads a second libgqmap.so (the parent commit's, built into a
directory outside the tree) and times the full search on both libraries in this
one process, so that drift of the existing entry points is visible, and says
whether their outputs are bit-identical.

usage: time_block_match_pyramid.py [--scale S] [--U U] [--V V] [--ft FT] [--sigma SG] [--levels L [L ...]] [--r R]
                                   [--k K] [--subpixel] [--runs R] [--against PATH]
  issue cases: (a) --scale 1 --U 7 --levels 2;  (b) --scale 4 --U 25 --levels 3 4, with and without --subpixel"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gqmap_opticalflow_amd import _lib, block_match, block_match_pyramid, imresize, load_pair  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--U", type=int, default=7)
ap.add_argument("--V", type=int, default=None)
ap.add_argument("--ft", type=int, default=3)
ap.add_argument("--sigma", type=float, default=1.7)
ap.add_argument("--levels", type=int, nargs="+", default=[2])
ap.add_argument("--r", type=int, default=1)
ap.add_argument("--k", type=int, default=1)
ap.add_argument("--subpixel", action="store_true")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--settle", type=float, default=0.5)
ap.add_argument("--against", default=None, metavar="PATH", help="a second libgqmap.so: the full search on both")
a = ap.parse_args()
V = a.U if a.V is None else a.V

I1, I2, _ = load_pair("rubberwhale")
if a.scale != 1:
    I1, I2 = imresize(I1, a.scale), imresize(I2, a.scale)
M, N = I1.shape
mine = _lib.load()
mine.gqmap_debug_block_match_stats.restype = C.c_int
mine.gqmap_debug_block_match_stats.argtypes = [C.c_int, C.POINTER(C.c_double)]


def timed_runs(call):
    t0, warm = time.perf_counter(), []
    while not warm or time.perf_counter() - t0 < a.settle:
        warm.append(call()[-1])
    return [call()[-1] for _ in range(a.runs)]


def full(lib):
    _lib._lib = lib  # the library block_match runs on
    return block_match(I1, I2, a.U, V, a.ft, a.sigma, timed=True, subpixel=a.subpixel)


what = f"{M}x{N} U={a.U} V={V} ft={a.ft} sigma={a.sigma} {'sub-pixel' if a.subpixel else 'integer'}"
base = None
if a.U <= 32 and V <= 32:
    ms = timed_runs(lambda: full(mine))
    base = statistics.median(ms)
    print(f"{what}: full search, this tree: runs " + " ".join(f"{x:.3f}" for x in ms) + f" ms, median {base:.3f} ms",
          flush=True)
    if a.against:
        other = C.CDLL(os.path.abspath(a.against))  # an older library: only the entry points timed here
        for name in ("gqmap_block_match", "gqmap_block_match_refine", "gqmap_last_error"):
            getattr(other, name).restype = getattr(mine, name).restype
            getattr(other, name).argtypes = getattr(mine, name).argtypes
        same = all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(full(mine)[:-1], full(other)[:-1]))
        oms = timed_runs(lambda: full(other))
        print(f"{what}: full search, against: runs " + " ".join(f"{x:.3f}" for x in oms) +
              f" ms, median {statistics.median(oms):.3f} ms; this tree / against {base / statistics.median(oms):.4f}; "
              f"outputs bit-identical: {same}", flush=True)
        _lib._lib = mine
for levels in a.levels:
    def call():
        return block_match_pyramid(I1, I2, a.U, V, a.ft, a.sigma, levels, a.r, a.k, subpixel=a.subpixel, timed=True)
    ms = timed_runs(call)
    med = statistics.median(ms)
    print(f"{what}: pyramid levels={levels} r={a.r} k={a.k}: runs " + " ".join(f"{x:.3f}" for x in ms) +
          f" ms, median {med:.3f} ms" + (f", full search / pyramid {base / med:.2f}" if base else ""), flush=True)
    stats = (C.c_double * 30)()
    mine.gqmap_debug_block_match_stats(1, None)
    call()
    mine.gqmap_debug_block_match_stats(0, stats)
    for l in range(levels - 1, -1, -1):
        pixels, tiles, scanned, area, lms = stats[5 * l:5 * l + 5]
        print(f"    level {l}: {lms:.3f} ms, {int(pixels)} pixels in {int(tiles)} tiles, mean box {area / pixels:.1f} "
              f"displacements per pixel, mean {scanned / tiles:.1f} evaluated per tile", flush=True)
