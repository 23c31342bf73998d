"""Cut 64 x 64 windows out of the reference's preprocessed (structure-texture)
frames (middlebury/preprocessed/<name>.mat: img1, img2, fp64) into
tests/golden/preprocessed_windows.npz: per pair <name>_img1, <name>_img2
(float64 64 x 64) and <name>_off (2 x 2 int: row, column offset of each
window).  img1's window is the frame's top-left corner, img2's the bottom-right
one, so both frame borders are inside a window.  The full frames are over the
size a committed file may have; tests compare the same window of the
full-frame result.  scipy.io.loadmat parses the MAT v5 data only.
usage: python scripts/make_preprocessed_windows.py <dir with the .mat files> [names...]"""
import os
import sys

import numpy as np
import scipy.io as sio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 64
src = sys.argv[1]
names = sys.argv[2:] or ["Dimetrodon", "Hydrangea", "Venus"]
out = {}
for n in names:
    d = sio.loadmat(os.path.join(src, n + ".mat"))
    img1, img2 = (np.asarray(d[k], np.float64) for k in ("img1", "img2"))
    M, N = img1.shape
    off = np.array([[0, 0], [M - W, N - W]], dtype=np.int64)
    out[n + "_img1"] = img1[:W, :W].copy()
    out[n + "_img2"] = img2[M - W:, N - W:].copy()
    out[n + "_off"] = off
    print(n, img1.shape, off.tolist())
path = os.path.join(ROOT, "tests", "golden", "preprocessed_windows.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes")
