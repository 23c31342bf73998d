// Block-matching initialiser (legacy/optical_flow_temp.m:13-32 with
// legacy/Gaussian_filter.m): the arithmetic, compiled by the kernel
// (gqmap_blockmatch.hip) and by the host model (gqmap_host.cpp).  Both include
// this one header and are built with -ffp-contract=off, so they agree bit for
// bit, ties included.
//
// Specification (fp64, fixed order, no contraction).  Indices are 0-based:
// displacement (u, v), u = 0..2U (rows), v = 0..2V (columns), pairs A(m, n)
// with B(m + u - U, n + v - V).
//   w[i], i = 0..2ft   e_i = exp(-(i-ft)^2 / 2 / sigma / sigma) (host exp),
//                      s = e_0 + e_1 + ... in that order, w_i = e_i / s.
//                      Gaussian_filter is the outer product w w' up to rounding.
//   D(m, n)            |A(m, n) - B(m+u-U, n+v-V)| with B = 0 outside the frame
//                      (img1_ext), and D = 0 for (m, n) outside the frame
//                      (conv2 'same').
//   T(m, n)            ((0 + w_0 D(m-ft, n)) + w_1 D(m-ft+1, n)) + ...   (rows)
//   cost(m, n)         ((0 + w_0 T(m, n-ft)) + w_1 T(m, n-ft+1)) + ...   (columns)
//   argmin             displacements visited in ascending u + v (2U+1); a
//                      displacement replaces the best only when cost < best,
//                      so the FIRST minimum wins ([~,idx] = min(...)).
//   flow               (V - v, U - u) = (vmt, umt).
//
// Several hypotheses per pixel (gqmap_block_match_multi): cost, filter and
// displacement order as above; on top of them a hypothesis count H in
// [1, GQ_BM_HMAX] and a separation sep in [1, 2 GQ_BM_UMAX + 1].
//   rank 0             the argmin above.
//   rank k >= 1        the same first-minimum scan (ascending u + v (2U+1),
//                      replaced only on cost < best) over the ALLOWED
//                      displacements: max(|u - u_j|, |v - v_j|) >= sep for the
//                      pick (u_j, v_j) of every earlier rank j < k (bm_far).
//                      sep = 1: the H smallest, distinct; sep = 2 also forbids
//                      the 8 neighbours of an earlier pick.
//   missing ranks      no allowed displacement at rank k: that rank and all
//                      later ones do not exist (their allowed sets are no
//                      larger); flow = NaN (bm_nan, one bit pattern), cost = +Inf.
//   flow               M x N x 2 x H, rank slowest, slice h as `flow` above;
//                      cost M x N x H.
//
// Sub-pixel refinement (gqmap_block_match_refine): cost, filter, displacement
// order, ranks, sep and missing ranks as above; on top of the pick (u0, v0) of
// rank k with cost c0, a three-point parabola per axis, each axis on its own.
// The row axis uses (u0 -/+ 1, v0), the column axis (u0, v0 -/+ 1).
//   cm, cp             the plain filtered costs of the two neighbours on the
//                      axis, whether or not rank k's separation rule would
//                      have allowed them.
//   refinable axis     both neighbours inside the window (1 <= u0 <= 2U - 1,
//                      1 <= v0 <= 2V - 1), cm >= c0, cp >= c0 and
//                      den = (cm - c0) + (cp - c0) > 0; a NaN cost fails the
//                      comparisons (bm_refine).
//   delta              fmin(fmax((cm - cp) / (den + den), -0.5), 0.5) on a
//                      refinable axis, 0 otherwise.
//   flow               ((double)(V - v0) - delta_v, (double)(U - u0) - delta_u),
//                      layout and sign of `flow` above (plane 0 horizontal).
//   curv               (den_v, den_u) on refinable axes, 0.0 otherwise; M x N x
//                      2 x H, laid out as flow.
//   missing ranks      flow NaN (bm_nan), cost +Inf, curv 0.0.
//   cost               the cost at the integer pick, as gqmap_block_match_multi.
//
// Per-pixel windows (gqmap_block_match_window): cost and filter as above, the
// displacement SIGNED: (du, dv) pairs A(m, n) with B(m + du, n + dv), B = 0
// outside the frame; the index (u, v) above is (du + U, dv + V).  Every bound
// below satisfies |bound| <= GQ_BM_DMAX.
//   win                int32, M x N x 4, column-major planes ulo, uhi, vlo, vhi:
//                      pixel (m, n) considers ulo <= du <= uhi, vlo <= dv <= vhi.
//                      All pixels under its filter footprint are differenced at
//                      that same displacement, as in the cost above.
//   pick               no scan order is implied.  With e = c when c < +Inf and
//                      e = +Inf otherwise (a NaN cost), a displacement of the
//                      box replaces the pick when e < best, or e == best and
//                      (dv, du) is lexicographically smaller (bm_keep_window);
//                      best starts at +Inf with no pick, which every (dv, du)
//                      precedes.  That is the first minimum in ascending
//                      (dv, du), today's u + v (2U+1) order, and on a frame whose
//                      costs are never < +Inf the first displacement of the box
//                      with cost +Inf, as bm_keep_allowed leaves it.  Chunking,
//                      tile width and scan order cannot change a result.
//   empty window       ulo > uhi or vlo > vhi: flow bm_nan(), cost +Inf, curv 0.0.
//   flow               ((double)(-dv0), (double)(-du0)), plane 0 horizontal.
//   subpixel != 0      bm_refine per axis as above; an axis is refinable only if
//                      both neighbours lie inside the pixel's OWN box (ulo < du0
//                      < uhi, likewise v); cm, cp are the plain filtered costs;
//                      flow = ((double)(-dv0) - delta_v, (double)(-du0) -
//                      delta_u), curv and cost as gqmap_block_match_refine at
//                      H = 1 (bm_refined_window).
//   anchor             the box [-U, U] x [-V, V] at every pixel: subpixel = 0 is
//                      gqmap_block_match bit for bit (flow, cost), subpixel = 1
//                      gqmap_block_match_refine at H = 1 (flow, cost, curv).
//
// Coarse to fine (gqmap_block_match_pyramid; U, V, ft, sigma, levels in [1, 6],
// r in [0, 4], k in [0, 2], subpixel):
//   bm_half            ceil(M/2) x ceil(N/2); out(i, j) = ((P(2i, 2j) + P(2i+1,
//                      2j)) + (P(2i, 2j+1) + P(2i+1, 2j+1))) * 0.25, row 2i+1
//                      clamped to M-1 and column 2j+1 to N-1.
//   level l            both frames under bm_half l times; the same ft and sigma.
//   coarsest           c = levels - 1: every pixel has the box [-Uc, Uc] x
//                      [-Vc, Vc], Uc = ceil(U / 2^c), Vc likewise, both <=
//                      GQ_BM_UMAX.
//   going down         fine pixel (m, n) looks at the integer picks of the coarse
//                      pixels (m>>1 + a, n>>1 + b), a, b in [-k, k], clamped to
//                      the coarse grid: ulo = 2 min(du) - r, uhi = 2 max(du) + r,
//                      v alike (bm_window_up).  A coarse pixel without a pick
//                      adds nothing; none with a pick: the empty window.
//   subpixel           level 0 only; coarser levels pass on integer picks.
//   outputs            level 0's flow, cost and curv.  levels = 1 is the anchor
//                      above, hence the existing entry points, bit for bit.
//   reach              Uc 2^c + r (2^c - 1) (bm_reach): the largest |du| the
//                      scheme can return.
//
// Ranked windows (gqmap_block_match_window_multi): cost, filter, signed
// displacement and GQ_BM_DMAX as in "Per-pixel windows"; on top of them H in
// [1, GQ_BM_HMAX] and sep in [1, 2 GQ_BM_UMAX + 1] (bm_bad_multi).
//   win                int32, M x N x 4 x H, rank slowest; slice j is laid out as
//                      `win` above and holds box j of every pixel.
//   pick               rank j applies the rule of bm_keep_window to the
//                      displacements of ITS box j that also satisfy max(|du -
//                      du_i|, |dv - dv_i|) >= sep for the pick (du_i, dv_i) of
//                      every earlier rank i < j that has one (bm_far_key, the
//                      signed sibling of bm_far).
//   missing ranks      box j empty, or nothing in it allowed: flow bm_nan(), cost
//                      +Inf, curv 0.0.  A missing rank excludes nothing, and
//                      later ranks go on: their boxes differ.
//   subpixel != 0      per rank, bm_refine per axis; an axis is refinable only
//                      when both neighbours lie in that rank's own box; cm, cp are
//                      the plain filtered costs, whether or not the separation
//                      would allow them (bm_refined_window, unchanged).
//   outputs            flow and curv M x N x 2 x H, cost M x N x H, rank slowest;
//                      signs and planes as gqmap_block_match_window's.  Scan
//                      order, chunking and tile width appear in no result.
//   identities         H = 1 is gqmap_block_match_window.  Rank 0 is
//                      gqmap_block_match_window on box 0 for any H and sep.  All H
//                      boxes [-U, U] x [-V, V]: subpixel = 0 is
//                      gqmap_block_match_multi, subpixel = 1
//                      gqmap_block_match_refine, at the same H and sep, missing
//                      ranks included (equal boxes make the allowed sets shrink).
//
// Ranked coarse to fine (gqmap_block_match_pyramid_multi): levels, bm_half, Uc,
// Vc, r, k and bm_reach as in "Coarse to fine"; H and sep as above.
//   coarsest           all H boxes are [-Uc, Uc] x [-Vc, Vc].
//   going down         box j of a fine pixel is bm_window_up over the coarse
//                      level's rank-j pick planes; a coarse pixel that misses
//                      rank j adds nothing.
//   every level        runs "Ranked windows" with the same H and sep; only level
//                      0 applies subpixel; the outputs are level 0's.
//   identities         H = 1 is gqmap_block_match_pyramid, and so is rank 0 at
//                      any H and sep: rank 0 depends on rank-0 picks only, level
//                      by level.  levels = 1 is the equal-boxes identity above.
#pragma once
#include <math.h>

#define GQ_BM_UMAX 32  /* U, V in [0, 32] */
#define GQ_BM_FTMAX 4  /* ft in [0, 4]    */
#define GQ_BM_TAPS (2 * GQ_BM_FTMAX + 1)
#define GQ_BM_HMAX 4   /* hypotheses per pixel in [1, 4] */

#ifdef __HIPCC__
#define GQ_BM_HD __host__ __device__ __forceinline__
#else
#define GQ_BM_HD inline
#endif
// the tap loops are unrolled in the kernel (weights in registers); the order is the same
#ifdef __HIP_DEVICE_COMPILE__
#define GQ_BM_UNROLL _Pragma("unroll")
#else
#define GQ_BM_UNROLL
#endif

namespace gq {

struct BmFilter {
    double w[GQ_BM_TAPS];
};

// Host only: the normalised 1-D Gaussian, handed to the kernel as bits.
inline BmFilter bm_filter(int ft, double sigma)
{
    BmFilter f;
    double s = 0.0;
    for (int i = 0; i < GQ_BM_TAPS; ++i) {
        const double k = (double)(i - ft);
        f.w[i] = i <= 2 * ft ? exp(-(k * k) / 2 / sigma / sigma) : 0.0;
        if (i <= 2 * ft) s = s + f.w[i];
    }
    for (int i = 0; i <= 2 * ft; ++i) f.w[i] = f.w[i] / s;
    return f;
}

// Host only: what is wrong with the arguments (nullptr: nothing).
inline const char *bm_bad_args(int M, int N, int U, int V, int ft, double sigma)
{
    if (M < 1 || N < 1) return "empty image";
    if (U < 0 || U > GQ_BM_UMAX || V < 0 || V > GQ_BM_UMAX) return "U, V outside [0,32]";
    if (ft < 0 || ft > GQ_BM_FTMAX) return "ft outside [0,4]";
    if (!(sigma > 0) || !isfinite(sigma)) return "sigma must be finite and > 0";
    return nullptr;
}

// Host only: what is wrong with the hypothesis arguments (nullptr: nothing).
inline const char *bm_bad_multi(int H, int sep)
{
    if (H < 1 || H > GQ_BM_HMAX) return "H outside [1,4]";
    if (sep < 1 || sep > 2 * GQ_BM_UMAX + 1) return "sep outside [1,65]";
    return nullptr;
}

// T of one (row, column): a and b point at tap 0 (frame row m_first = m - ft)
// of the A and the displaced B column, rows contiguous; col_in = the column
// lies inside the frame.  Both arrays must be readable over all 2ft+1 taps.
GQ_BM_HD double bm_rows(const double *a, const double *b, int ft, const BmFilter &f, int m_first, int M,
                        bool col_in)
{
    double acc = 0.0;
GQ_BM_UNROLL
    for (int i = 0; i < GQ_BM_TAPS; ++i) {
        if (i > 2 * ft) break;
        const int m = m_first + i;
        const double d = col_in && m >= 0 && m < M ? fabs(a[i] - b[i]) : 0.0;
        acc = acc + f.w[i] * d;
    }
    return acc;
}

// cost of one pixel: t points at T(m, n - ft), consecutive columns `stride` apart.
GQ_BM_HD double bm_cols(const double *t, int stride, int ft, const BmFilter &f)
{
    double acc = 0.0;
GQ_BM_UNROLL
    for (int j = 0; j < GQ_BM_TAPS; ++j) {
        if (j > 2 * ft) break;
        acc = acc + f.w[j] * t[j * stride];
    }
    return acc;
}

// running first-minimum over the displacement index
GQ_BM_HD void bm_keep(double c, int idx, double &best, int &best_idx)
{
    if (c < best) {
        best = c;
        best_idx = idx;
    }
}

// a pick (u, v) in one int: u, v <= 2 GQ_BM_UMAX fit 8 bits each
GQ_BM_HD int bm_pack(int u, int v) { return u | (v << 8); }

// (u, v) is at least sep away (Chebyshev) from an earlier pick
GQ_BM_HD bool bm_far(int u, int v, int pick, int sep)
{
    int du = u - (pick & 255), dv = v - (pick >> 8);
    du = du < 0 ? -du : du;
    dv = dv < 0 ? -dv : dv;
    return (du > dv ? du : dv) >= sep;
}

// bm_keep over the allowed displacements only.  best_idx starts at -1 = "no
// allowed displacement yet"; the first allowed one takes it whatever its cost,
// as index 0 does at rank 0, so a cost that is never < best (NaN frames)
// still names the first allowed displacement.
GQ_BM_HD void bm_keep_allowed(bool allowed, double c, int idx, double &best, int &best_idx)
{
    if (allowed) {
        if (best_idx < 0) best_idx = idx;
        bm_keep(c, idx, best, best_idx);
    }
}

// the flow of a missing rank: the quiet NaN 0x7ff8000000000000 on host and device
GQ_BM_HD double bm_nan() { return __builtin_nan(""); }

// Sub-pixel refinement.  The four neighbour costs of a pick: row axis (u0 -/+ 1,
// v0), column axis (u0, v0 -/+ 1); NaN until the scan meets the displacement.
struct BmNear {
    double um, up, vm, vp;
};

GQ_BM_HD void bm_near_clear(BmNear &q) { q.um = q.up = q.vm = q.vp = bm_nan(); }

// cost c of displacement (u, v) into q when (u, v) is a neighbour of the packed
// pick; a missing pick is -1, which unpacks to (255, -1) and has no neighbour.
GQ_BM_HD void bm_capture(int u, int v, int pick, double c, BmNear &q)
{
    const int pu = pick & 255, pv = pick >> 8;
    if (v == pv) {
        if (u == pu - 1) q.um = c;
        if (u == pu + 1) q.up = c;
    }
    if (u == pu) {
        if (v == pv - 1) q.vm = c;
        if (v == pv + 1) q.vp = c;
    }
}

// one axis of the parabola fit: offset delta and curvature den, 0 when the axis
// is not refinable.  The comparisons are false on NaN.
GQ_BM_HD void bm_refine(double cm, double c0, double cp, bool in_window, double *delta, double *den)
{
    const double d = (cm - c0) + (cp - c0);
    const bool ok = in_window && cm >= c0 && cp >= c0 && d > 0;
    *delta = ok ? fmin(fmax((cm - cp) / (d + d), -0.5), 0.5) : 0.0;
    *den = ok ? d : 0.0;
}

// flow and curvature of one rank at one pixel from its packed pick (-1: missing)
// and its neighbour costs: out = {flow_h, flow_v, curv_h, curv_v}, plane 0 horizontal
GQ_BM_HD void bm_refined(int pick, double c0, const BmNear &q, int U, int V, double out[4])
{
    const bool found = pick >= 0;
    const int pu = pick & 255, pv = pick >> 8;
    double du, dv, ku, kv;
    bm_refine(q.um, c0, q.up, found && pu >= 1 && pu <= 2 * U - 1, &du, &ku);
    bm_refine(q.vm, c0, q.vp, found && pv >= 1 && pv <= 2 * V - 1, &dv, &kv);
    out[0] = found ? (double)(V - pv) - dv : bm_nan();  // vmt
    out[1] = found ? (double)(U - pu) - du : bm_nan();  // umt
    out[2] = kv;
    out[3] = ku;
}

// ---- per-pixel windows and the coarse-to-fine scheme -------------------------

#define GQ_BM_DMAX 2048                     /* every window bound in [-2048, 2048] */
#define GQ_BM_CHUNK (2 * GQ_BM_UMAX + 1)    /* displacements per axis of one staged B window */
#define GQ_BM_LEVELS 6                      /* levels in [1, 6] */
#define GQ_BM_RMAX 4                        /* r in [0, 4] */
#define GQ_BM_KMAX 2                        /* k in [0, 2] */
#define GQ_BM_NOPICK 0x7fffffff             /* no pick: after every key, and the value of both pick planes */

// a signed displacement in one int, ordered as (dv, du) lexicographically
GQ_BM_HD int bm_key(int du, int dv) { return ((dv + GQ_BM_DMAX) << 13) | (du + GQ_BM_DMAX); }
GQ_BM_HD int bm_key_du(int key) { return (key & 8191) - GQ_BM_DMAX; }
GQ_BM_HD int bm_key_dv(int key) { return (key >> 13) - GQ_BM_DMAX; }

// the box {ulo, uhi, vlo, vhi} holds (du, dv)
GQ_BM_HD bool bm_in_box(const int box[4], int du, int dv)
{
    return du >= box[0] && du <= box[1] && dv >= box[2] && dv <= box[3];
}

// the pick rule of "Per-pixel windows": best starts at +Inf, key at GQ_BM_NOPICK
GQ_BM_HD void bm_keep_window(bool allowed, double c, int du, int dv, double &best, int &key)
{
    const double e = c < INFINITY ? c : INFINITY;
    const int k = bm_key(du, dv);
    if (allowed && (e < best || (e == best && k < key))) {
        best = e;
        key = k;
    }
}

// bm_far for a signed displacement and the key of an earlier rank; a missing rank (GQ_BM_NOPICK) excludes nothing
GQ_BM_HD bool bm_far_key(int du, int dv, int key, int sep)
{
    int au = du - bm_key_du(key), av = dv - bm_key_dv(key);
    au = au < 0 ? -au : au;
    av = av < 0 ? -av : av;
    return key == GQ_BM_NOPICK || (au > av ? au : av) >= sep;
}

// bm_capture for a signed displacement and a key (GQ_BM_NOPICK has no neighbour in reach)
GQ_BM_HD void bm_capture_window(int du, int dv, int key, double c, BmNear &q)
{
    const int pu = bm_key_du(key), pv = bm_key_dv(key);
    if (dv == pv) {
        if (du == pu - 1) q.um = c;
        if (du == pu + 1) q.up = c;
    }
    if (du == pu) {
        if (dv == pv - 1) q.vm = c;
        if (dv == pv + 1) q.vp = c;
    }
}

// (du, dv) is a neighbour that the refinement of the pick `key` in `box` needs
GQ_BM_HD bool bm_near_wanted(const int box[4], int du, int dv, int key)
{
    const int pu = bm_key_du(key), pv = bm_key_dv(key);
    if (key == GQ_BM_NOPICK) return false;
    const bool on_u = dv == pv && (du == pu - 1 || du == pu + 1) && box[0] < pu && pu < box[1];
    const bool on_v = du == pu && (dv == pv - 1 || dv == pv + 1) && box[2] < pv && pv < box[3];
    return on_u || on_v;
}

// bm_refined for a pick in the pixel's own box; subpixel = false leaves the integer flow and curv 0
GQ_BM_HD void bm_refined_window(int key, double c0, const BmNear &q, const int box[4], bool subpixel, double out[4])
{
    const bool found = key != GQ_BM_NOPICK;
    const int pu = bm_key_du(key), pv = bm_key_dv(key);
    double du = 0.0, dv = 0.0, ku = 0.0, kv = 0.0;
    if (subpixel) {
        bm_refine(q.um, c0, q.up, found && box[0] < pu && pu < box[1], &du, &ku);
        bm_refine(q.vm, c0, q.vp, found && box[2] < pv && pv < box[3], &dv, &kv);
        out[0] = found ? (double)(-pv) - dv : bm_nan();
        out[1] = found ? (double)(-pu) - du : bm_nan();
    } else {
        out[0] = found ? (double)(-pv) : bm_nan();
        out[1] = found ? (double)(-pu) : bm_nan();
    }
    out[2] = kv;
    out[3] = ku;
}

// one pixel of the half-resolution frame
GQ_BM_HD double bm_half(const double *P, int M, int N, int i, int j)
{
    const int m0 = 2 * i, n0 = 2 * j, m1 = m0 + 1 < M ? m0 + 1 : M - 1, n1 = n0 + 1 < N ? n0 + 1 : N - 1;
    const double a = P[m0 + (long long)M * n0] + P[m1 + (long long)M * n0];
    const double b = P[m0 + (long long)M * n1] + P[m1 + (long long)M * n1];
    return (a + b) * 0.25;
}

// the box of fine pixel (m, n) from the coarse picks: pick holds the planes du, dv, Mc x Nc each
GQ_BM_HD void bm_window_up(const int *pick, int Mc, int Nc, int m, int n, int r, int k, int box[4])
{
    int ulo = GQ_BM_NOPICK, uhi = -GQ_BM_NOPICK, vlo = GQ_BM_NOPICK, vhi = -GQ_BM_NOPICK;
    for (int b = -k; b <= k; ++b)
        for (int a = -k; a <= k; ++a) {
            int i = (m >> 1) + a, j = (n >> 1) + b;
            i = i < 0 ? 0 : i > Mc - 1 ? Mc - 1 : i;
            j = j < 0 ? 0 : j > Nc - 1 ? Nc - 1 : j;
            const int du = pick[i + (long long)Mc * j], dv = pick[i + (long long)Mc * j + (long long)Mc * Nc];
            if (du == GQ_BM_NOPICK) continue;
            ulo = du < ulo ? du : ulo;
            uhi = du > uhi ? du : uhi;
            vlo = dv < vlo ? dv : vlo;
            vhi = dv > vhi ? dv : vhi;
        }
    const bool any = ulo != GQ_BM_NOPICK;
    box[0] = any ? 2 * ulo - r : 1;
    box[1] = any ? 2 * uhi + r : 0;
    box[2] = any ? 2 * vlo - r : 1;
    box[3] = any ? 2 * vhi + r : 0;
}

GQ_BM_HD int bm_ceil_shift(int x, int c) { return (x + (1 << c) - 1) >> c; }

// the largest displacement the coarse-to-fine scheme can return
GQ_BM_HD int bm_reach(int U, int levels, int r)
{
    const int c = levels - 1;
    return (bm_ceil_shift(U, c) << c) + r * ((1 << c) - 1);
}

// Host only: what is wrong with the arguments of the window entry points (nullptr: nothing)
inline const char *bm_bad_window(int M, int N, int ft, double sigma)
{
    if (M < 1 || N < 1) return "empty image";
    if (ft < 0 || ft > GQ_BM_FTMAX) return "ft outside [0,4]";
    if (!(sigma > 0) || !isfinite(sigma)) return "sigma must be finite and > 0";
    return nullptr;
}

// Host only: a bound of win beyond GQ_BM_DMAX
inline bool bm_bad_bounds(const int *win, int M, int N)
{
    for (long long i = 0; i < 4LL * M * N; ++i)
        if (win[i] < -GQ_BM_DMAX || win[i] > GQ_BM_DMAX) return true;
    return false;
}

// Host only: what is wrong with the arguments of the pyramid entry points (nullptr: nothing)
inline const char *bm_bad_pyramid(int M, int N, int U, int V, int ft, double sigma, int levels, int r, int k)
{
    if (const char *bad = bm_bad_window(M, N, ft, sigma)) return bad;
    if (levels < 1 || levels > GQ_BM_LEVELS) return "levels outside [1,6]";
    if (r < 0 || r > GQ_BM_RMAX) return "r outside [0,4]";
    if (k < 0 || k > GQ_BM_KMAX) return "k outside [0,2]";
    if (U < 0 || V < 0 || U > GQ_BM_DMAX || V > GQ_BM_DMAX) return "U, V outside [0,2048]";
    if (bm_ceil_shift(U, levels - 1) > GQ_BM_UMAX || bm_ceil_shift(V, levels - 1) > GQ_BM_UMAX)
        return "U, V at the coarsest level outside [0,32]";
    return nullptr;
}

}  // namespace gq
