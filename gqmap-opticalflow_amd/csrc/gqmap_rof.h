// Structure-texture preprocessing (optical_flowSuper.m:7-14, preprocessed =
// true: the generator of middlebury/preprocessed/<name>.mat): ROF
// decomposition by Chambolle's dual projection.  The arithmetic, compiled by
// the kernels (gqmap_rof.hip) and by the host model (gqmap_host.cpp).  Both
// include this one header and are built with -ffp-contract=off; sqrt and
// division are IEEE correctly rounded on both sides, so they agree bit for bit.
//
// Specification (fp64, fixed order, no contraction).  Indices are 0-based, m
// the row (fastest in memory), n the column; im is M x N x C column-major.
//   x          lo, hi = min, max over all M*N*C values;
//              x = ((im - lo) / (hi - lo)) * 2.0 + (-1.0)
//   p1 = p2 = 0 per plane; delta = 1.0 / (4.0 * theta), computed on the host
//   one iteration, per plane, Jacobi (every read is of the previous p):
//     d(m,n)   (p1(m,n) - p1(m,n-1)) + (p2(m,n) - p2(m-1,n)), p outside = +0
//     u(m,n)   x(m,n) + theta*d(m,n)            (product rounded, then the sum)
//     ix(m,n)  u(m,n+1) - u(m,n), +0 in the last column
//     iy(m,n)  u(m+1,n) - u(m,n), +0 in the last row
//     q1 = p1 + delta*ix, q2 = p2 + delta*iy, r = max(1.0, sqrt(q1*q1 + q2*q2))
//     p1 = q1 / r, p2 = q2 / r
//   after n_iter iterations: s = x + theta*d (d of the final p), t = x - alp*s
//   tlo, thi = min, max of t over all planes;
//   texture = ((t - tlo) / (thi - tlo)) * 255.0 + 0.0;  structure = s
// A zero or non-finite range (constant or NaN/Inf input) is an argument error.
#pragma once
#include <math.h>

#define GQ_ROF_CMAX 8         /* planes, C in [1, 8]     */
#define GQ_ROF_ITMAX 10000    /* n_iter in [0, 10000]    */

#ifdef __HIPCC__
#define GQ_ROF_HD __host__ __device__ __forceinline__
#else
#define GQ_ROF_HD inline
#endif

namespace gq {

// Host only: what is wrong with the arguments (nullptr: nothing).
inline const char *rof_bad_args(int M, int N, int C, double theta, int n_iter, double alp)
{
    if (M < 1 || N < 1) return "empty image";
    if (C < 1 || C > GQ_ROF_CMAX) return "C outside [1,8]";
    if (!(theta > 0) || !isfinite(theta)) return "theta must be finite and > 0";
    if (n_iter < 0 || n_iter > GQ_ROF_ITMAX) return "n_iter outside [0,10000]";
    if (!isfinite(alp)) return "alp must be finite";
    return nullptr;
}

// Host only: a range a rescale cannot divide by (bad = a non-finite value was seen).
inline bool rof_bad_range(double lo, double hi, bool bad)
{
    const double w = hi - lo;
    return bad || !isfinite(lo) || !isfinite(hi) || !(w > 0) || !isfinite(w);
}

inline double rof_delta(double theta) { return 1.0 / (4.0 * theta); }

GQ_ROF_HD double rof_scale_in(double v, double lo, double hi) { return ((v - lo) / (hi - lo)) * 2.0 + (-1.0); }

// d: pw = p1(m, n-1), pn = p2(m-1, n), +0 where outside the frame
GQ_ROF_HD double rof_div(double p1, double pw, double p2, double pn) { return (p1 - pw) + (p2 - pn); }

GQ_ROF_HD double rof_u(double x, double theta, double d) { return x + theta * d; }

// the dual step; ix, iy are already +0 in the last column / row
GQ_ROF_HD void rof_step(double &p1, double &p2, double ix, double iy, double delta)
{
    const double q1 = p1 + delta * ix, q2 = p2 + delta * iy;
    const double r = fmax(1.0, sqrt(q1 * q1 + q2 * q2));
    p1 = q1 / r;
    p2 = q2 / r;
}

GQ_ROF_HD double rof_t(double x, double alp, double s) { return x - alp * s; }

GQ_ROF_HD double rof_scale_out(double t, double tlo, double thi) { return ((t - tlo) / (thi - tlo)) * 255.0 + 0.0; }

}  // namespace gq
