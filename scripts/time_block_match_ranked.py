"""Kernel time of gqmap_block_match_pyramid_multi (HIP events over all kernels
of the call, copies excluded) on a RubberWhale frame pair at H = 1 and H = --H,
beside its two yardsticks timed in the same process: gqmap_block_match_pyramid
(what one hypothesis costs) and the full search that the ranked pyramid replaces,
gqmap_block_match_multi / gqmap_block_match_refine at the same U, V and H.
Median of --runs timed calls after a warm-up that keeps the GPU busy for
--settle seconds (at least one call), integer and sub-pixel.

Per level it prints what the library's counters say for the ranked call
(gqmap_debug_block_match_stats, one extra call with counting on, not among the
timed ones; summed over the ranks): the time of the level's kernels, the mean
box area per pixel and rank, and the mean number of displacements a tile
evaluated in its selection walks per rank.

usage: time_block_match_ranked.py [--scale S] [--U U] [--levels L] [--H H] [--sep S] [--r R] [--k K] [--runs R]
  issue cases: (a) --scale 1 --U 7 --levels 2;  (b) --scale 4 --U 25 --levels 3
  (profiles/block_match_ranked_times.txt)"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gqmap_opticalflow_amd import _lib, block_match, block_match_pyramid, imresize, load_pair  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--U", type=int, default=7)
ap.add_argument("--ft", type=int, default=3)
ap.add_argument("--sigma", type=float, default=1.7)
ap.add_argument("--levels", type=int, default=2)
ap.add_argument("--H", type=int, default=3)
ap.add_argument("--sep", type=int, default=2)
ap.add_argument("--r", type=int, default=1)
ap.add_argument("--k", type=int, default=1)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--settle", type=float, default=0.5)
a = ap.parse_args()

I1, I2, _ = load_pair("rubberwhale")
if a.scale != 1:
    I1, I2 = imresize(I1, a.scale), imresize(I2, a.scale)
M, N = I1.shape
lib = _lib.load()
lib.gqmap_debug_block_match_stats.restype = C.c_int
lib.gqmap_debug_block_match_stats.argtypes = [C.c_int, C.POINTER(C.c_double)]


def median_ms(call):
    t0, warm = time.perf_counter(), []
    while not warm or time.perf_counter() - t0 < a.settle:
        warm.append(call()[-1])
    ms = [call()[-1] for _ in range(a.runs)]
    return statistics.median(ms), " ".join(f"{x:.3f}" for x in ms)


for subpixel in (False, True):
    what = (f"{M}x{N} U=V={a.U} ft={a.ft} sigma={a.sigma} levels={a.levels} r={a.r} k={a.k} sep={a.sep} "
            f"{'sub-pixel' if subpixel else 'integer'}")
    pyr = dict(levels=a.levels, r=a.r, k=a.k, subpixel=subpixel, timed=True)

    def ranked(H):
        return lambda: block_match_pyramid(I1, I2, a.U, a.U, a.ft, a.sigma, hypotheses=H, sep=a.sep, **pyr)

    plain, runs = median_ms(lambda: block_match_pyramid(I1, I2, a.U, a.U, a.ft, a.sigma, **pyr))
    print(f"{what}: plain pyramid: runs {runs} ms, median {plain:.3f} ms", flush=True)
    one, runs = median_ms(ranked(1))
    print(f"{what}: ranked pyramid H=1: runs {runs} ms, median {one:.3f} ms, / plain pyramid {one / plain:.2f}", flush=True)
    many, runs = median_ms(ranked(a.H))
    print(f"{what}: ranked pyramid H={a.H}: runs {runs} ms, median {many:.3f} ms, / plain pyramid {many / plain:.2f}, "
          f"per rank / plain pyramid {many / a.H / plain:.2f}", flush=True)
    if a.U <= 32:
        full, runs = median_ms(lambda: block_match(I1, I2, a.U, a.U, a.ft, a.sigma, hypotheses=a.H, sep=a.sep,
                                                   subpixel=subpixel, timed=True))
        print(f"{what}: full search H={a.H} ({'refine' if subpixel else 'multi'}): runs {runs} ms, median {full:.3f} ms, "
              f"full search / ranked pyramid {full / many:.2f}", flush=True)
    stats = (C.c_double * 30)()
    lib.gqmap_debug_block_match_stats(1, None)
    ranked(a.H)()
    lib.gqmap_debug_block_match_stats(0, stats)
    for l in range(a.levels - 1, -1, -1):
        pixels, tiles, scanned, area, lms = stats[5 * l:5 * l + 5]
        print(f"    H={a.H} level {l}: {lms:.3f} ms, {int(pixels)} pixels in {int(tiles)} tiles, mean box "
              f"{area / pixels / a.H:.1f} displacements per pixel and rank, mean {scanned / tiles / a.H:.1f} evaluated per "
              f"tile and rank", flush=True)
    lib.gqmap_debug_block_match_stats(1, None)
    block_match_pyramid(I1, I2, a.U, a.U, a.ft, a.sigma, **pyr)
    lib.gqmap_debug_block_match_stats(0, stats)
    for l in range(a.levels - 1, -1, -1):
        pixels, tiles, scanned, area, lms = stats[5 * l:5 * l + 5]
        print(f"    plain level {l}: {lms:.3f} ms, mean box {area / pixels:.1f} displacements per pixel, mean "
              f"{scanned / tiles:.1f} evaluated per tile", flush=True)
