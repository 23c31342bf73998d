// Weighted median filter of a flow, guided by an image and a confidence map:
// the arithmetic, compiled by the kernel (gqmap_wmedian.hip) and by the host
// model (gqmap_host.cpp).  Both include this one header and are built with
// -ffp-contract=off, so they agree bit for bit.
//
// Specification (fp64, fixed order, no contraction).  Indices are 0-based, m
// the row (fastest in memory), n the column.  flow is M x N x 2 (plane 0
// horizontal), guide G and the optional confidence C are M x N; without C the
// confidence is 1 everywhere.  r in [0, 8], sigma_s and sigma_c finite and > 0,
// passes in [1, 8].
//
// The window of the output pixel (m, n) is every (i, j) of the frame with
// |i - m| <= r and |j - n| <= r.
//
// Weight of the entry (i, j), every operation rounded on its own:
//   s[k], k = 0..2r    exp(-(k-r)^2 / 2 / sigma_s / sigma_s) (host exp; handed
//                      to the kernel as bits)
//   d                  (G(i,j) - G(m,n)) / sigma_c
//   w                  (s[i-m+r] * s[j-n+r]) * (1.0 / (1.0 + d*d))
//                      with C: w = w * C(i,j)
// The range weight is rational: it needs only correctly rounded +, *, /, so
// host and device agree with no table and no assumption on the image's range.
//
// Fixed point (wm_wq):
//   wq                 w >= 2^-16 ? (uint32)((w < 1.0 ? w : 1.0) * 65536.0) : 0
// A NaN weight fails the comparison and gives 0: a NaN in G (at the entry or at
// the centre) or in C.  All sums of wq are exact integers below 2^25 (289
// entries of at most 2^16), so no result depends on an order of summation.
//
// Selection, per plane c:
//   live               wq > 0 and flow_c(i,j) is not NaN; +-Inf are values.
//   key                the monotone 64-bit key of the double's bits (wm_key):
//                      sign bit set: all bits flipped, else the sign bit
//                      flipped.  -0 sorts before +0; equal keys are equal bits.
//   W                  the sum of the live wq
//   out                W = 0: the input, bit for bit.  Otherwise the bits of
//                      the live entry with the smallest key k such that
//                      2 * sum_{live, key <= k} wq >= W: the lower weighted
//                      median.
//
// Consequences: r = 0 is the identity.  A NaN centre is filled whenever
// anything live is in reach.  A pixel with C = 0 never contributes, even after
// it has been replaced (C stays fixed): to inpaint, mark pixels NaN instead.
//
// Passes are Jacobi: pass p reads the whole output of pass p - 1; G and C stay
// fixed.
#pragma once
#include <math.h>
#include <stdint.h>

#define GQ_WM_RMAX 8 /* r in [0, 8] */
#define GQ_WM_TAPS (2 * GQ_WM_RMAX + 1)
#define GQ_WM_PASSMAX 8 /* passes in [1, 8] */

#ifdef __HIPCC__
#define GQ_WM_HD __host__ __device__ __forceinline__
#else
#define GQ_WM_HD inline
#endif

namespace gq {

struct WmFilter {
    double s[GQ_WM_TAPS];
};

// Host only: the spatial taps, handed to the kernel as bits.
inline WmFilter wm_filter(int r, double sigma_s)
{
    WmFilter f;
    for (int i = 0; i < GQ_WM_TAPS; ++i) {
        const double k = (double)(i - r);
        f.s[i] = i <= 2 * r ? exp(-(k * k) / 2 / sigma_s / sigma_s) : 0.0;
    }
    return f;
}

// Host only: what is wrong with the arguments (nullptr: nothing).
inline const char *wm_bad(int M, int N, int r, double sigma_s, double sigma_c, int passes)
{
    if (M < 1 || N < 1) return "empty field";
    if (r < 0 || r > GQ_WM_RMAX) return "r outside [0,8]";
    if (!(sigma_s > 0) || !isfinite(sigma_s)) return "sigma_s must be finite and > 0";
    if (!(sigma_c > 0) || !isfinite(sigma_c)) return "sigma_c must be finite and > 0";
    if (passes < 1 || passes > GQ_WM_PASSMAX) return "passes outside [1,8]";
    return nullptr;
}

// the order-preserving key of a double's bits, and back
GQ_WM_HD uint64_t wm_key(uint64_t bits) { return bits >> 63 ? ~bits : bits ^ 0x8000000000000000ull; }
GQ_WM_HD uint64_t wm_unkey(uint64_t key) { return key >> 63 ? key ^ 0x8000000000000000ull : ~key; }

// the key belongs to a NaN: above +Inf's or below -Inf's
GQ_WM_HD bool wm_key_nan(uint64_t key) { return key > 0xfff0000000000000ull || key < 0x000fffffffffffffull; }

// wq of one entry: ss = s[i-m+r] * s[j-n+r], g = G(i,j), gc = G(m,n), c = C(i,j)
// (1.0 without a confidence map: w * 1.0 is w, bit for bit)
GQ_WM_HD uint32_t wm_wq(double ss, double g, double gc, double sigma_c, double c)
{
    const double d = (g - gc) / sigma_c;
    double w = ss * (1.0 / (1.0 + d * d));
    w = w * c;
    return w >= 0x1p-16 ? (uint32_t)((w < 1.0 ? w : 1.0) * 65536.0) : 0u;
}

}  // namespace gq
