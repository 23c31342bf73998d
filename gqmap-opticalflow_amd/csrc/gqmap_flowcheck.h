// Forward-backward check of two flows and the fill of the rejected pixels:
// the arithmetic, compiled by the kernels (gqmap_flowcheck.hip) and by the
// host models (gqmap_host.cpp).  Both include this one header and are built
// with -ffp-contract=off, so they agree bit for bit.
//
// Specification (fp64, fixed order, no contraction).  Indices are 0-based, m
// the row (fastest in memory), n the column.
//
// Flow convention (block_match_init's and the .flo ground truth's): plane 0 is
// horizontal, plane 1 vertical; pixel (m, n) of the first frame lies at
// (m + f1, n + f0) in the second.  fwd lives on frame 1's grid, bwd on frame
// 2's grid and points back to frame 1.
//
// Consistency (fc_check), per pixel (m, n):
//   u, v               fwd(m, n, 0), fwd(m, n, 1)
//   x, y               (double)n + u, (double)m + v
//   inside             x >= 0 && x <= N-1 && y >= 0 && y <= M-1 (false on NaN);
//                      not inside: err = +Inf, mask = 0, nothing is sampled.
//   j0, j1, fx         j0 = min((int)floor(x), max(N-2, 0)), j1 = min(j0+1, N-1),
//                      fx = x - (double)j0; i0, i1, fy likewise from y and M.
//   b_P                per plane P of bwd
//                      ((P(i0,j0)*(1-fy) + P(i1,j0)*fy)*(1-fx)) +
//                      ((P(i0,j1)*(1-fy) + P(i1,j1)*fy)*fx),
//                      every product and sum rounded on its own (fc_bilinear).
//   ru, rv             u + b0, v + b1
//   e2                 ru*ru + rv*rv
//   mag                (u*u + v*v) + (b0*b0 + b1*b1)
//   thr                a1*mag + a2
//   err, mask          e2, e2 <= thr (false on NaN)
//
// Fill (fc_fill_*): a normalised convolution over the valid pixels, `passes`
// Jacobi passes.  The state of a pixel is one byte: 0 = valid on entry, p =
// filled in pass p (1-based), 255 = not valid (FC_UNFILLED); the state after
// the last pass is the `filled` output.
//   w[i], i = 0..2r    exp(-(i-r)^2 / 2 / sigma / sigma) (host exp), not
//                      normalised.
//   per pass           V = valid ? 1.0 : 0.0, S_c = valid ? flow_c : 0.0 -- a
//                      select, not a product: what is stored at a pixel that is
//                      not valid (NaN, Inf) reaches nothing.  Both 0 outside
//                      the frame.
//   T_X(m, n)          ((0 + w_0 X(m-r, n)) + w_1 X(m-r+1, n)) + ...   (rows)
//   Y_X(m, n)          ((0 + w_0 T_X(m, n-r)) + w_1 T_X(m, n-r+1)) + ... (columns)
//   out                a pixel that is not valid and has Y_V > 0 takes
//                      out_c = Y_{S_c} / Y_V (correctly rounded division) and
//                      the state p; every other pixel keeps flow and state bit
//                      for bit.  A pass with nothing to fill is the identity.
#pragma once
#include <math.h>

#define GQ_FC_RMAX 16  /* r in [0, 16] */
#define GQ_FC_TAPS (2 * GQ_FC_RMAX + 1)
#define GQ_FC_PASSMAX 8 /* passes in [1, 8] */
#define GQ_FC_UNFILLED 255

#ifdef __HIPCC__
#define GQ_FC_HD __host__ __device__ __forceinline__
#else
#define GQ_FC_HD inline
#endif

namespace gq {

struct FcFilter {
    double w[GQ_FC_TAPS];
};

// Host only: the Gaussian taps, handed to the kernel as bits.
inline FcFilter fc_filter(int r, double sigma)
{
    FcFilter f;
    for (int i = 0; i < GQ_FC_TAPS; ++i) {
        const double k = (double)(i - r);
        f.w[i] = i <= 2 * r ? exp(-(k * k) / 2 / sigma / sigma) : 0.0;
    }
    return f;
}

// Host only: what is wrong with the arguments (nullptr: nothing).
inline const char *fc_bad_check(int M, int N, double a1, double a2)
{
    if (M < 1 || N < 1) return "empty field";
    if (!(a1 >= 0) || !isfinite(a1) || !(a2 >= 0) || !isfinite(a2)) return "a1, a2 must be finite and >= 0";
    return nullptr;
}

inline const char *fc_bad_fill(int M, int N, int r, double sigma, int passes)
{
    if (M < 1 || N < 1) return "empty field";
    if (r < 0 || r > GQ_FC_RMAX) return "r outside [0,16]";
    if (!(sigma > 0) || !isfinite(sigma)) return "sigma must be finite and > 0";
    if (passes < 1 || passes > GQ_FC_PASSMAX) return "passes outside [1,8]";
    return nullptr;
}

// one plane of bwd at (i0 + fy, j0 + fx): p points at the plane, rows contiguous
GQ_FC_HD double fc_bilinear(const double *p, int M, int i0, int i1, int j0, int j1, double fy, double fx)
{
    const double gy = 1.0 - fy, gx = 1.0 - fx;
    const double c0 = p[i0 + (long long)M * j0] * gy + p[i1 + (long long)M * j0] * fy;
    const double c1 = p[i0 + (long long)M * j1] * gy + p[i1 + (long long)M * j1] * fy;
    return c0 * gx + c1 * fx;
}

// cell and fraction of a coordinate x in [0, len - 1]
GQ_FC_HD void fc_cell(double x, int len, int *k0, int *k1, double *f)
{
    const int cap = len - 2 > 0 ? len - 2 : 0;
    const int k = (int)floor(x);
    *k0 = k < cap ? k : cap;
    *k1 = *k0 + 1 < len - 1 ? *k0 + 1 : len - 1;
    *f = x - (double)*k0;
}

// err and mask of pixel (m, n); fwd and bwd are M x N x 2
GQ_FC_HD bool fc_check(const double *fwd, const double *bwd, int m, int n, int M, int N, double a1, double a2,
                       double *err)
{
    const long long MN = (long long)M * N, o = m + (long long)M * n;
    const double u = fwd[o], v = fwd[o + MN];
    const double x = (double)n + u, y = (double)m + v;
    const bool inside = x >= 0.0 && x <= (double)(N - 1) && y >= 0.0 && y <= (double)(M - 1);
    if (!inside) {
        *err = INFINITY;
        return false;
    }
    int i0, i1, j0, j1;
    double fx, fy;
    fc_cell(x, N, &j0, &j1, &fx);
    fc_cell(y, M, &i0, &i1, &fy);
    const double b0 = fc_bilinear(bwd, M, i0, i1, j0, j1, fy, fx);
    const double b1 = fc_bilinear(bwd + MN, M, i0, i1, j0, j1, fy, fx);
    const double ru = u + b0, rv = v + b1;
    const double e2 = ru * ru + rv * rv;
    const double mag = (u * u + v * v) + (b0 * b0 + b1 * b1);
    const double thr = a1 * mag + a2;
    *err = e2;
    return e2 <= thr;
}

// T of one (row, column): x points at tap 0 (row m - r) of a column whose rows
// are contiguous and hold 0 outside the frame and at pixels that are not valid.
GQ_FC_HD double fc_rows(const double *x, int r, const FcFilter &f)
{
    double acc = 0.0;
    for (int i = 0; i <= 2 * r; ++i) acc = acc + f.w[i] * x[i];
    return acc;
}

// Y of one pixel: t points at T(m, n - r), consecutive columns `stride` apart.
GQ_FC_HD double fc_cols(const double *t, int stride, int r, const FcFilter &f)
{
    double acc = 0.0;
    for (int j = 0; j <= 2 * r; ++j) acc = acc + f.w[j] * t[j * stride];
    return acc;
}

// a pixel of this state, with this Y_V, is filled in this pass
GQ_FC_HD bool fc_fills(unsigned char state, double yv) { return state == GQ_FC_UNFILLED && yv > 0.0; }

}  // namespace gq
