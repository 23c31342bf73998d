"""Standalone device ops of libgqmap.so beside the iteration.

flow_to_color   flowToColor_mex (legacy/flowToColor.m:37-87 + legacy/computeColor.m:33-115)
mixture_map     get_map_mex     (legacy/findMixMax.m:39-70 semantics, fminbnd TolX 1e-4)
projsplx        projsplx.m:15-30, batched over columns (projsplx.m:34-67)
gauss_hermite   GaussHermite_2.m (host)
imresize        imresize(A, scale) bicubic + antialias (legacy/optical_flow_ctf.m:26-29)
warp_image      interp2 linear + fillmissing nearest (legacy/optical_flow_ctf.m:30-32)
block_match     Gaussian-filtered SAD block matching (legacy/optical_flow_temp.m:13-32)
block_match_window   the same cost over a search window per pixel (csrc/gqmap_blockmatch.h)
block_match_pyramid  coarse-to-fine block matching on block_match_window
structure_texture  ROF structure-texture frames (optical_flowSuper.m:7-14, preprocessed=true)
flow_consistency   forward-backward check of two flows (csrc/gqmap_flowcheck.h)
flow_fill          rejected pixels refilled from the valid ones around them
flow_denoise       weighted flow denoising: per-pixel variance, missing data, adjoint scatter (csrc/gqmap_denoise.h)
flow_wmedian       weighted median filter guided by an image and a confidence map (csrc/gqmap_wmedian.h)
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, dptr, f64, u8ptr


def flow_to_color(flow, max_flow: float = 0.0, device: int = 0):
    """[img, flo, minu, maxu, minv, maxv, idxUnknown] = flowToColor(flow)
    returned as (img uint8 MxNx3, flo MxNx2, (minu,maxu,minv,maxv), unknown MxN bool)."""
    flow = f64(flow)
    if flow.ndim != 3 or flow.shape[2] != 2:
        raise ValueError("flowToColor: image must have two bands")
    M, N, _ = flow.shape
    img = np.zeros((M, N, 3), dtype=np.uint8, order="F")
    flo = np.zeros((M, N, 2), order="F")
    stats = np.zeros(4)
    unk = np.zeros((M, N), dtype=np.uint8, order="F")
    check(_lib.load().gqmap_flow_to_color(dptr(flow), M, N, float(max_flow), u8ptr(img), dptr(flo),
                                          dptr(stats), u8ptr(unk), device), "gqmap_flow_to_color")
    return img, flo, tuple(float(x) for x in stats), unk.astype(bool)


def mixture_map(alpha, muu, sigu, muv, sigv, device: int = 0) -> np.ndarray:
    muu, sigu, muv, sigv = map(f64, (muu, sigu, muv, sigv))
    if muu.ndim == 2:
        muu, sigu, muv, sigv = (a[:, :, None] for a in (muu, sigu, muv, sigv))
        muu, sigu, muv, sigv = map(f64, (muu, sigu, muv, sigv))
    alpha = f64(np.ravel(alpha))
    M, N, L = muu.shape
    out = np.zeros((M, N, 2), order="F")
    check(_lib.load().gqmap_mixture_map(dptr(alpha), dptr(muu), dptr(sigu), dptr(muv), dptr(sigv),
                                        M, N, L, dptr(out), device), "gqmap_mixture_map")
    return out


def projsplx(Y, device: int = 0) -> np.ndarray:
    """Project y (vector) or every column of Y onto the probability simplex."""
    Y = np.asarray(Y, dtype=np.float64)
    vec = Y.ndim == 1
    Yc = f64(Y.reshape(-1, 1) if vec else Y)
    n, ncols = Yc.shape
    X = np.zeros((n, ncols), order="F")
    check(_lib.load().gqmap_projsplx(dptr(Yc), dptr(X), n, ncols, device), "gqmap_projsplx")
    return X.ravel() if vec else X


def gauss_hermite(K: int):
    x, w = np.zeros(K), np.zeros(K)
    check(_lib.load().gqmap_gauss_hermite(K, dptr(x), dptr(w)), "gqmap_gauss_hermite")
    return x, w


def resize_len(n: int, scale: float) -> int:
    """imresize output length ceil(scale * n)."""
    return int(_lib.load().gqmap_resize_len(int(n), float(scale)))


def imresize(A, scale: float, antialias: bool = True, device: int = 0) -> np.ndarray:
    """imresize(A, scale) with MATLAB's defaults ('bicubic', Antialiasing on
    when shrinking) for an M x N (x C) double array, resampled on the device."""
    A = f64(A)
    M, N = A.shape[:2]
    Cn = 1 if A.ndim == 2 else int(np.prod(A.shape[2:]))
    oM, oN = resize_len(M, scale), resize_len(N, scale)
    out = np.zeros((oM, oN) + A.shape[2:], order="F")
    check(_lib.load().gqmap_imresize(dptr(A), M, N, Cn, float(scale), int(antialias), dptr(out),
                                     device), "gqmap_imresize")
    return out


def warp_image(V, warp, fill: bool = True, device: int = 0) -> np.ndarray:
    """interp2(V, x - warp(:,:,1), y - warp(:,:,2)) (linear, NaN outside),
    then fillmissing(.,'nearest',1) and (.,'nearest',2) when fill."""
    V, warp = f64(V), f64(warp)
    M, N = V.shape
    if warp.shape != (M, N, 2):
        raise ValueError(f"warp must be {M}x{N}x2, got {warp.shape}")
    out = np.zeros((M, N), order="F")
    check(_lib.load().gqmap_warp_image(dptr(V), M, N, dptr(warp), int(fill), dptr(out), device),
          "gqmap_warp_image")
    return out


def block_match(A, B, U: int = 7, V: int = 7, ft: int = 3, sigma: float = 1.7, device: int = 0,
                host: bool = False, timed: bool = False, hypotheses: int | None = None, sep: int = 2,
                subpixel: bool = False):
    """legacy/optical_flow_temp.m:13-32: per pixel the displacement of the
    (2U+1) x (2V+1) window with the smallest Gaussian-filtered |A - B shifted|
    (first minimum).  Returns (flow M x N x 2 = cat(3, vmt, umt), cost M x N):
    A(m, n) matches B(m - umt, n - vmt).  The reference call is A = img_2,
    B = img_1.  host=True runs the library's host model of the same arithmetic
    (no device; bit-identical).  timed=True also returns the kernel time in ms.

    hypotheses=H (1..4) returns the H best mutually separated displacements
    (gqmap_block_match_multi): flow M x N x 2 x H, cost M x N x H.  Rank 0 is
    the result above; rank k is the first minimum over the displacements at
    least `sep` away (larger of the row and column distance) from every earlier
    pick.  A rank with no displacement left is NaN in flow and +Inf in cost.

    subpixel=True (gqmap_block_match_refine; hypotheses defaults to 1, shapes as
    with hypotheses=) returns (flow, cost, curv): per rank and axis a three-point
    parabola through the cost at the pick and at its two neighbours moves the
    flow by at most half a pixel, and curv (M x N x 2 x H, laid out as flow) is
    the parabola's second difference cm - 2 c0 + cp; an axis whose pick sits on
    the window's edge, or is not a strict enough minimum of its three points,
    keeps the integer flow and has curv 0.  cost stays the cost at the integer
    pick.  A missing rank is NaN / +Inf / 0."""
    A, B = f64(A), f64(B)
    if A.ndim != 2 or A.shape != B.shape:
        raise ValueError("block_match: A and B must be equal-size 2-D images")
    M, N = A.shape
    lib = _lib.load()
    if subpixel and hypotheses is None:
        hypotheses = 1
    name, ranks, rank_args = "gqmap_block_match", (), ()
    if hypotheses is not None:
        H = int(hypotheses)
        if not 1 <= H <= 4:  # the shapes below depend on it; the library checks the rest
            raise ValueError(f"block_match: hypotheses must be in 1..4, got {hypotheses}")
        name, ranks, rank_args = name + ("_refine" if subpixel else "_multi"), (H,), (H, int(sep))
    out = [np.zeros((M, N, 2) + ranks, order="F"), np.zeros((M, N) + ranks, order="F")]  # flow, cost
    if subpixel:
        out.append(np.zeros((M, N, 2) + ranks, order="F"))  # curv
    ms = C.c_double(float("nan"))
    tail = () if host else (C.cast(C.byref(ms), _lib._D) if timed else None, device)
    name += "_host" if host else ""
    check(getattr(lib, name)(dptr(A), dptr(B), M, N, int(U), int(V), int(ft), float(sigma), *rank_args,
                             *map(dptr, out), *tail), name)
    return (*out, ms.value) if timed else tuple(out)


def _match_outputs(lib, name, host, timed, device, M, N, subpixel, head, ranks=()):
    """The (flow, cost[, curv][, ms]) tail of the window and pyramid calls; ranks = (H, sep) for the ranked entry points."""
    tail_shape = ranks[:1]
    flow, cost, curv = (np.zeros(s + tail_shape, order="F") for s in ((M, N, 2), (M, N), (M, N, 2)))
    ms = C.c_double(float("nan"))
    tail = () if host else (C.cast(C.byref(ms), _lib._D) if timed else None, device)
    name += ("_multi" if ranks else "") + ("_host" if host else "")
    check(getattr(lib, name)(*head, *ranks, int(bool(subpixel)), dptr(flow), dptr(cost),
                             dptr(curv) if subpixel else None, *tail), name)
    out = (flow, cost, curv) if subpixel else (flow, cost)
    return (*out, ms.value) if timed else out


def _ranks(who, hypotheses, sep):
    """(H, sep) of a ranked call, () without hypotheses."""
    if hypotheses is None:
        return ()
    H = int(hypotheses)
    if not 1 <= H <= 4:  # the shapes depend on it; the library checks the rest
        raise ValueError(f"{who}: hypotheses must be in 1..4, got {hypotheses}")
    return (H, int(sep))


def block_match_window(A, B, win, ft: int = 3, sigma: float = 1.7, subpixel: bool = False, device: int = 0,
                       host: bool = False, timed: bool = False, hypotheses: int | None = None, sep: int = 2):
    """block_match with a search window per pixel (gqmap_block_match_window).
    win: integer M x N x 4 = (ulo, uhi, vlo, vhi), bounds in [-2048, 2048]: pixel
    (m, n) pairs A(m, n) with B(m + du, n + dv) over ulo <= du <= uhi, vlo <= dv
    <= vhi and takes the first minimum in ascending (dv, du).  Returns (flow
    M x N x 2 = (-dv0, -du0), cost M x N), laid out and signed as block_match's;
    a pixel with an empty window is NaN in flow and +Inf in cost.
    subpixel=True returns (flow, cost, curv): the parabola of
    block_match(subpixel=True) per axis, on an axis whose two neighbours lie inside
    the pixel's own window.  With win = [-U, U] x [-V, V] everywhere the results
    are block_match's, bit for bit.  host=True runs the library's host model (no
    device; bit-identical); timed=True appends the kernel time in ms.

    hypotheses=H (1..4) returns H ranked picks (gqmap_block_match_window_multi):
    win is M x N x 4 x H, a box per rank (an M x N x 4 window is given to every
    rank), and rank j is the pick above over the displacements of box j at least
    `sep` away (larger of the row and column distance) from the pick of every
    earlier rank that has one.  flow and curv are M x N x 2 x H, cost M x N x H,
    as block_match(hypotheses=H)'s; a rank whose box is empty, or in which
    nothing is allowed, is NaN / +Inf / 0, excludes nothing, and later ranks go
    on.  Rank 0 is the call without hypotheses on box 0; with the same box
    [-U, U] x [-V, V] at every rank the results are block_match(hypotheses=H,
    sep=sep)'s, bit for bit."""
    A, B = f64(A), f64(B)
    if A.ndim != 2 or A.shape != B.shape:
        raise ValueError("block_match_window: A and B must be equal-size 2-D images")
    M, N = A.shape
    ranks = _ranks("block_match_window", hypotheses, sep)
    if ranks and np.shape(win) == (M, N, 4):
        win = np.repeat(np.asarray(win)[..., None], ranks[0], axis=3)
    if np.shape(win) != (M, N, 4) + ranks[:1]:
        want = "x".join(map(str, (M, N, 4) + ranks[:1]))
        raise ValueError(f"block_match_window: win must be {want}, got {np.shape(win)}")
    win = np.require(np.asarray(win, dtype=np.int32), requirements=["F_CONTIGUOUS", "ALIGNED"])
    head = (dptr(A), dptr(B), win.ctypes.data_as(C.POINTER(C.c_int)), M, N, int(ft), float(sigma))
    return _match_outputs(_lib.load(), "gqmap_block_match_window", host, timed, device, M, N, subpixel, head, ranks)


def block_match_reach(U: int, levels: int, r: int) -> int:
    """The largest displacement along an axis that block_match_pyramid(U, ..., levels, r) can return."""
    reach = int(_lib.load().gqmap_block_match_reach(int(U), int(levels), int(r)))
    if reach < 0:
        raise ValueError(f"block_match_reach: U={U} levels={levels} r={r} out of range")
    return reach


def block_match_pyramid(A, B, U: int = 7, V: int = 7, ft: int = 3, sigma: float = 1.7, levels: int = 2, r: int = 1,
                        k: int = 1, subpixel: bool = False, device: int = 0, host: bool = False, timed: bool = False,
                        hypotheses: int | None = None, sep: int = 2):
    """Coarse-to-fine block matching (gqmap_block_match_pyramid).  Both frames
    are halved levels - 1 times (2 x 2 means); the coarsest level searches
    +-ceil(U / 2^(levels-1)) x +-ceil(V / 2^(levels-1)) (each <= 32, so U and V may
    exceed 32), and every finer level searches, per pixel, the box spanned by
    twice the picks of the (2k+1) x (2k+1) coarse pixels around it, widened by r
    (block_match_window).  levels in 1..6, r in 0..4, k in 0..2.  Returns (flow,
    cost) of level 0, or (flow, cost, curv) with subpixel=True (applied at level 0
    only), shaped as block_match_window's; levels=1 is block_match, bit for bit.
    The displacements returned lie within +-block_match_reach(U, levels, r).
    host=True runs the library's host model (no device; bit-identical);
    timed=True appends the time of all kernels of the call in ms.

    hypotheses=H (1..4) carries H ranked picks through the levels
    (gqmap_block_match_pyramid_multi): every level runs
    block_match_window(hypotheses=H, sep=sep), all boxes equal at the coarsest,
    and box j of a finer pixel comes from the rank-j picks of the coarse pixels
    around it, so every rank keeps a narrow box of its own.  The outputs carry
    the rank axis as block_match_window(hypotheses=H)'s.  Rank 0 is the call
    without hypotheses, bit for bit; levels=1 is block_match(hypotheses=H)."""
    A, B = f64(A), f64(B)
    if A.ndim != 2 or A.shape != B.shape:
        raise ValueError("block_match_pyramid: A and B must be equal-size 2-D images")
    M, N = A.shape
    ranks = _ranks("block_match_pyramid", hypotheses, sep)
    head = (dptr(A), dptr(B), M, N, int(U), int(V), int(ft), float(sigma), int(levels), int(r), int(k))
    return _match_outputs(_lib.load(), "gqmap_block_match_pyramid", host, timed, device, M, N, subpixel, head, ranks)


def flow_consistency(fwd, bwd, a1: float = 0.01, a2: float = 0.5, device: int = 0, host: bool = False,
                     timed: bool = False):
    """Forward-backward check (gqmap_flow_consistency).  fwd, bwd: M x N x 2,
    plane 0 horizontal, in block_match_init's convention: pixel (m, n) of the
    first frame lies at (m + fwd1, n + fwd0) in the second; bwd lives on the
    second frame's grid and points back.  Returns (err, mask): err = |fwd +
    bwd(target)|^2 with bwd sampled bilinearly at the pixel's target, +Inf where
    the target leaves the frame or is NaN; mask (bool) = err <= a1 (|fwd|^2 +
    |bwd(target)|^2) + a2.  host=True runs the library's host model of the same
    arithmetic (no device; bit-identical).  timed=True appends the kernel time
    in ms."""
    fwd, bwd = f64(fwd), f64(bwd)
    if fwd.ndim != 3 or fwd.shape[2] != 2 or bwd.shape != fwd.shape:
        raise ValueError("flow_consistency: fwd and bwd must be equal-size M x N x 2 flows")
    M, N, _ = fwd.shape
    err = np.zeros((M, N), order="F")
    mask = np.zeros((M, N), dtype=np.uint8, order="F")
    lib = _lib.load()
    ms = C.c_double(float("nan"))
    tail = () if host else (C.cast(C.byref(ms), _lib._D) if timed else None, device)
    name = "gqmap_flow_consistency" + ("_host" if host else "")
    check(getattr(lib, name)(dptr(fwd), dptr(bwd), M, N, float(a1), float(a2), dptr(err), u8ptr(mask), *tail), name)
    out = (err, mask.astype(bool))
    return (*out, ms.value) if timed else out


def flow_fill(flow, mask, r: int = 8, sigma: float = 4.0, passes: int = 2, device: int = 0, host: bool = False,
              timed: bool = False):
    """Refill the pixels whose mask is false from the valid pixels around them
    (gqmap_flow_fill): `passes` Jacobi passes of a normalised convolution with
    the (2r+1)^2 Gaussian of width sigma; a pixel filled in one pass is valid in
    the next.  flow: M x N x 2, mask: M x N.  Returns (flow, filled): filled
    (uint8) is 0 where the pixel was valid on entry, p where pass p filled it and
    255 where it is still not valid (its flow is then the input's, bit for bit).
    What flow holds at a pixel that is not valid (NaN included) reaches nothing.
    host=True runs the library's host model (no device; bit-identical).
    timed=True appends the kernel time in ms."""
    flow = f64(flow)
    if flow.ndim != 3 or flow.shape[2] != 2:
        raise ValueError("flow_fill: flow must be M x N x 2")
    M, N, _ = flow.shape
    if np.shape(mask) != (M, N):
        raise ValueError(f"flow_fill: mask must be {M}x{N}, got {np.shape(mask)}")
    mask = np.require((np.asarray(mask) != 0).astype(np.uint8), requirements=["F_CONTIGUOUS", "ALIGNED"])
    out = np.zeros((M, N, 2), order="F")
    filled = np.zeros((M, N), dtype=np.uint8, order="F")
    lib = _lib.load()
    ms = C.c_double(float("nan"))
    tail = () if host else (C.cast(C.byref(ms), _lib._D) if timed else None, device)
    name = "gqmap_flow_fill" + ("_host" if host else "")
    check(getattr(lib, name)(dptr(flow), u8ptr(mask), M, N, int(r), float(sigma), int(passes), dptr(out), u8ptr(filled),
                             *tail), name)
    return (out, filled, ms.value) if timed else (out, filled)


def flow_wmedian(flow, guide, r: int = 2, sigma_s: float = 2.0, sigma_c: float = 10.0, passes: int = 1, conf=None,
                 device: int = 0, host: bool = False, timed: bool = False):
    """Weighted median filter of a flow (gqmap_flow_wmedian; csrc/gqmap_wmedian.h
    holds the specification): per plane the lower weighted median over the
    (2r+1)^2 window, the entry (i, j) of pixel (m, n) weighing
    exp(-((i-m)^2 + (j-n)^2) / 2 sigma_s^2) / (1 + ((guide(i,j) - guide(m,n)) / sigma_c)^2)
    [* conf(i,j)], taken to 16 fractional bits; `passes` Jacobi passes with
    guide and conf fixed.  flow: M x N x 2, guide: M x N, conf: M x N or None (1
    everywhere).  Returns the filtered flow; every value of it is one of its
    window's own bit patterns.  NaN entries and entries without a weight (below
    2^-16, NaN guide or conf) take no part; a pixel with nothing to choose from
    keeps its bits.  So r = 0 is the identity, a NaN pixel is filled from what is
    in reach, and a pixel with conf = 0 never contributes, even after it has been
    replaced: to inpaint, mark pixels NaN instead.  host=True runs the library's
    host model (no device; bit-identical).  timed=True returns (flow, kernel
    time in ms)."""
    flow = f64(flow)
    if flow.ndim != 3 or flow.shape[2] != 2:
        raise ValueError("flow_wmedian: flow must be M x N x 2")
    M, N, _ = flow.shape
    if np.shape(guide) != (M, N):
        raise ValueError(f"flow_wmedian: guide must be {M}x{N}, got {np.shape(guide)}")
    if conf is not None and np.shape(conf) != (M, N):
        raise ValueError(f"flow_wmedian: conf must be {M}x{N}, got {np.shape(conf)}")
    guide = f64(guide)
    conf = None if conf is None else f64(conf)
    out = np.zeros((M, N, 2), order="F")
    lib = _lib.load()
    ms = C.c_double(float("nan"))
    tail = () if host else (C.cast(C.byref(ms), _lib._D) if timed else None, device)
    name = "gqmap_flow_wmedian" + ("_host" if host else "")
    check(getattr(lib, name)(dptr(flow), dptr(guide), None if conf is None else dptr(conf), M, N, int(r),
                             float(sigma_s), float(sigma_c), int(passes), dptr(out), *tail), name)
    return (out, ms.value) if timed else out


def structure_texture(im, theta: float = 0.125, n_iter: int = 100, alp: float = 0.95, device: int = 0,
                      host: bool = False, structure: bool = False, timed: bool = False):
    """The generator of the reference's preprocessed frames (optical_flowSuper.m:7-14,
    preprocessed=true): ROF structure-texture decomposition by Chambolle's dual
    projection.  im is M x N (x C); all planes are rescaled jointly to [-1, 1],
    the texture t = x - alp*s jointly to [0, 255].  Returns the texture in im's
    shape; structure=True returns (texture, s) with s in the [-1, 1] domain
    (unpinned: the reference holds no structure frames).  host=True runs the
    library's host model of the same arithmetic (no device; bit-identical).
    timed=True appends the kernel time in ms."""
    im = f64(im)
    if im.ndim not in (2, 3):
        raise ValueError("structure_texture: im must be M x N or M x N x C")
    M, N = im.shape[:2]
    Cn = 1 if im.ndim == 2 else im.shape[2]
    tex = np.zeros(im.shape, order="F")
    s = np.zeros(im.shape, order="F") if structure else None
    sp = dptr(s) if structure else None
    lib = _lib.load()
    ms = C.c_double(float("nan"))
    if host:
        check(lib.gqmap_structure_texture_host(dptr(im), M, N, Cn, float(theta), int(n_iter), float(alp), dptr(tex),
                                               sp), "gqmap_structure_texture_host")
    else:
        check(lib.gqmap_structure_texture(dptr(im), M, N, Cn, float(theta), int(n_iter), float(alp), dptr(tex), sp,
                                          C.cast(C.byref(ms), _lib._D) if timed else None, device),
              "gqmap_structure_texture")
    out = (tex, s) if structure else (tex,)
    if timed:
        out += (ms.value,)
    return out if len(out) > 1 else out[0]


def preprocess_pair(I1, I2, **kw):
    """(T1, T2): the texture frames of structure_texture(cat(3, I1, I2), **kw),
    what optical_flowSuper.m loads for a pair when preprocessed=true."""
    I1, I2 = f64(I1), f64(I2)
    if I1.ndim != 2 or I1.shape != I2.shape:
        raise ValueError("preprocess_pair: I1 and I2 must be equal-size 2-D images")
    if kw.get("structure") or kw.get("timed"):
        raise ValueError("preprocess_pair returns the two texture frames only")
    tex = structure_texture(np.stack([I1, I2], axis=2), **kw)
    return np.asfortranarray(tex[:, :, 0]), np.asfortranarray(tex[:, :, 1])


def _scatter_code(scatter) -> int:
    codes = {"reference": _lib.SCATTER_REFERENCE, "adjoint": _lib.SCATTER_ADJOINT}
    if scatter not in codes:
        raise ValueError(f"flow_denoise: scatter must be 'reference' or 'adjoint', got {scatter!r}")
    return codes[scatter]


def denoise_step_bound(o, min_var) -> float:
    """step0 (1 / min observed var + 8 / gama): the ascent of flow_denoise is
    linearly stable while this stays below 2.  min_var None: nothing is observed."""
    return o.step0 * ((0.0 if min_var is None else 1.0 / min_var) + 8.0 / o.gama)


def flow_denoise(flow, var=None, mu0=None, sigma0=None, options=None, scatter: str = "adjoint", seed: int = 0,
                 device: int = 0, host: bool = False, return_trace: bool = False, check_step: bool = True):
    """Weighted flow denoising (gqmap_flow_denoise; csrc/gqmap_denoise.h holds
    the specification): the engine of gqmap_cpu -- a Gaussian observation of a
    flow under truncated-quadratic pairwise terms -- with a variance per pixel
    and axis, missing observations, a start of its own and a choice of scatter.
    Returns (mu, sigma, rou), shaped as gqmap_cpu's; return_trace=True appends
    the its_done x 3 trace of max|dmu|, max|dsigma|, max|drou|.

    flow, var, mu0, sigma0: M x N x 2, plane 0 horizontal.  An entry is observed
    iff flow is finite, var is finite and var > 0 (var=None: iff flow is finite,
    at options["var"]).  An unobserved entry is moved by its edges alone
    (inpainting); what flow and var hold there reaches nothing.  mu0 is the
    start and must be finite; mu0=None starts from flow, which must then be
    finite.  sigma0=None draws U(0,1) + 2 from the library RNG (seed).
    options: the knobs of gqmap_cpu (its, K, var, gama, dta, step0, step_decay,
    corr_tor, tor, min_its).

    scatter="reference" is legacy/gqmap_cpu.m:58-59 as written, which hands an
    edge's second-endpoint gradient to the node two places before that
    endpoint: a shifted second difference that amplifies low frequencies
    ("Weighted flow denoising"); with var=None and mu0=None it is
    gqmap_cpu bit for bit.  scatter="adjoint" hands it to the endpoint.  The
    last row and column own no node term and no edge (the reference's loop
    bounds): under "adjoint" they hang on one edge each.

    Step bound.  To first order the ascent is mu <- mu + step (D + L) mu with
    D = -1/var on the observed entries and L the 4-connected graph Laplacian
    over gama, whose eigenvalues reach -8/gama.  The explicit step is stable
    only while step0 (1 / min observed var + 8 / gama) < 2; at or above it the
    highest frequency grows at every iteration, whatever the data.  The call
    raises ValueError there; check_step=False skips the test.

    host=True runs the library's host model (no device; bit-identical),
    threaded over columns (GQMAP_HOST_THREADS; the result does not depend on
    it)."""
    from .legacy import cpu_options
    flow = f64(flow)
    if flow.ndim != 3 or flow.shape[2] != 2:
        raise ValueError("flow must be M x N x 2")
    M, N, _ = flow.shape
    o = cpu_options(options)
    code = _scatter_code(scatter)
    opt = {}
    for name, a in (("var", var), ("mu0", mu0), ("sigma0", sigma0)):
        opt[name] = None if a is None else f64(a)
        if opt[name] is not None and opt[name].shape != (M, N, 2):
            raise ValueError(f"{name} must be {M} x {N} x 2 like flow, got {opt[name].shape}")
    if check_step:
        with np.errstate(invalid="ignore"):
            seen = np.isfinite(flow)
            if opt["var"] is not None:
                seen &= np.isfinite(opt["var"]) & (opt["var"] > 0)
        vmin = None if not seen.any() else float(opt["var"][seen].min()) if opt["var"] is not None else o.var
        bound = denoise_step_bound(o, vmin)
        if not bound < 2:
            raise ValueError(f"flow_denoise: step0 (1 / min observed var + 8 / gama) = {bound:g} >= 2 (step0 = {o.step0:g}, "
                             f"min observed var = {vmin}, gama = {o.gama:g}): the ascent is linearly unstable; lower "
                             "step0, raise gama or the variances, or pass check_step=False")
    mu = np.zeros((M, N, 2), order="F")
    sigma = np.zeros((M, N, 2), order="F")
    rou = np.zeros((M, N, 2, 2), order="F")
    trace = np.zeros((max(o.its, 1), 3))
    done = C.c_int(0)
    ptr = lambda a: dptr(a) if a is not None else None
    name = "gqmap_flow_denoise" + ("_host" if host else "")
    check(getattr(_lib.load(), name)(C.byref(o), dptr(flow), ptr(opt["var"]), ptr(opt["mu0"]), M, N, ptr(opt["sigma0"]),
                                     C.c_uint64(seed), code, dptr(mu), dptr(sigma), dptr(rou), dptr(trace),
                                     C.byref(done), *(() if host else (device,))), name)
    if return_trace:
        return mu, sigma, rou, trace[:done.value]
    return mu, sigma, rou
