// Weighted flow denoising: the arithmetic of one iteration, compiled by the
// kernels (gqmap_legacy.hip) and by the host model (gqmap_host.cpp).  Both
// include this one header and are built with -ffp-contract=off, so they agree
// bit for bit.  The engine of legacy/gqmap_cpu.m (gqmap_cpu_run) is the special
// case var == NULL, mu0 == NULL, scatter = reference.
//
// Specification (fp64, fixed order, no contraction).  Indices are 0-based, m the
// row (fastest in memory), n the column, l the layer (plane 0 horizontal).
//
// Inputs, all M x N x 2, column-major: flow (the observation), var (or NULL),
// mu0 (or NULL), sigma0 (or NULL).  State: mu, sigma (M x N x 2), rou
// (M x N x 2 x 2: edge j, layer l).  Scratch: dnode (M x N x 2 x 2), dedge
// (M x N x 2 x 5 x 2: edge j, term q, layer l), both zero before iteration 1.
//
// Start.  mu = mu0, which must be finite everywhere; mu0 == NULL: mu = flow,
// and then flow must be finite.  sigma = sigma0, or U(0,1) + 2 from the library
// RNG (seed, stream 3, index = the entry's linear index).  rou = 0.
//
// Observation (dn_observed).  Entry (m, n, l) is observed iff flow is finite,
// var is finite and var > 0; with var == NULL every finite flow entry is
// observed, at the scalar o->var.
//
// Per iteration it = 1, 2, ...:
//   Nodes m < M-1, n < N-1 own a node rule per layer and two edges, j = 0 to
//   (m+1, n) and j = 1 to (m, n+1).  The last row and the last column have no
//   node rule and own no edge (the reference's loop bounds).
//   Node rule (dn_node), K Gauss-Hermite points X, W:
//     x_k    = (sqrt(2) * sigma) * X[k] + mu
//     dval_k = W[k] * (f - x_k) / var      observed
//            = +0.0                         unobserved -- a select: a NaN, an
//              Inf or any payload stored in flow or var there reaches nothing
//     dnode(0) = (sum_k dval_k) / sqrt(pi)
//     dnode(1) = (sum_k dval_k * X[k]) * sqrt(2 / pi)
//   so an unobserved node's dnode is exactly +0: it is moved by its edges alone
//   (inpainting).
//   Edge rule (dn_edge), K x K points, p = rou, (o1, u1) the owner's sigma and
//   mu, (o2, u2) the second endpoint's:
//     q = sqrt(1 + p), r = sqrt(1 - p), s = (q + r) / 2, t = (q - r) / 2,
//     ds = (1/q - 1/r) / 4, dt = (1/q + 1/r) / 4
//     per column c (XI = X[c]) and row rr (XJ = X[rr]):
//       ZI = s*XI + t*XJ, ZJ = t*XI + s*XJ
//       diff = ((sqrt(2)*o2)*ZJ + u2) - ((sqrt(2)*o1)*ZI + u1); |diff| > dta: 0
//       df1 = (W[c]*W[rr]) * diff / gama, df2 = -df1
//       c1 += df1, co1 += df1*ZI, co2 += df2*ZJ,
//       cp += o1*df1*(ds*XI + dt*XJ) + o2*df2*(dt*XI + ds*XJ)
//     column sums first, then their sum over c (s1, so1, so2, sp); s2 = 0 - s1
//     dedge(q = 0..4) = 1/pi*s1, 1/pi*s2, 1/pi*sqrt(2)*so1, 1/pi*sqrt(2)*so2,
//                       1/pi*sqrt(2)*sp
//   Sum (dn_gather), every node and layer:
//     a = dnode(0) + (dedge(m,n,0,0) + dedge(m,n,1,0))
//     b = dnode(1) + (dedge(m,n,0,2) + dedge(m,n,1,2))
//     scatter = reference (0), legacy/gqmap_cpu.m:58-59 as written:
//       nu = dedge(m+1,n,0,1), nl = dedge(m,n+1,1,1) (0.0 past the frame),
//       su, sl likewise from q = 3
//     scatter = adjoint (1): the edges whose second endpoint the node is,
//       nu = dedge(m-1,n,0,1) when m >= 1, nl = dedge(m,n-1,1,1) when n >= 1,
//       su, sl from q = 3; otherwise 0.0
//     a = a + (nu + nl), b = b + (su + sl)
//   The reference's shift hands an edge's second-endpoint gradient to the node
//   two places before that endpoint; the adjoint scatter hands it to the
//   endpoint.  Under it a node of the last row (column) has no node rule and no
//   edge of its own: it hangs on the one edge that ends in it, (m-1, n, j=0) or
//   (m, n-1, j=1), and the corner node (M-1, N-1) on none -- it never moves.
//   Step (dn_apply): step = step0 / (1 + it / step_decay);
//     mu = mu + a*step; sigma = |sigma + b*step|;
//     rou(j) = fmax(fmin(rou(j) + dedge(m,n,j,4)*step, corr), -corr)
//   Trace: the maxima over all nodes and layers of |a|, |b| and |dedge(.,4)|,
//   taken on the bit patterns of |x| (dn_abits: exact in any order, a NaN
//   above +Inf).  Stop (dn_stop) after iteration it when it + 1 > its, or
//   it + 1 > min_its and max|a| < tor.
#pragma once
#include <math.h>
#include <stddef.h>

#ifdef __HIPCC__
#define GQ_DN_HD __host__ __device__ __forceinline__
#else
#define GQ_DN_HD inline
#endif

// full unroll for a constant K (the compilers of the kernels and of the library's host side)
#ifdef __clang__
#define GQ_DN_PRAGMA(x) _Pragma(#x)
#define GQ_DN_UNROLL(n) GQ_DN_PRAGMA(unroll n)
#else
#define GQ_DN_UNROLL(n)
#endif

// How the node rule takes its variance: the scalar var, the scalar var == 1
// (x / 1 == x exactly, the division is left out), or a field with the
// observation select.
#define GQ_DN_VAR_SCALAR 0
#define GQ_DN_VAR_ONE 1
#define GQ_DN_VAR_FIELD 2

namespace gq {

GQ_DN_HD size_t dn_i3(int M, int N, int m, int n, int l) { return m + (size_t)M * (n + (size_t)N * l); }
GQ_DN_HD size_t dn_i4(int M, int N, int m, int n, int a, int b)
{
    return m + (size_t)M * (n + (size_t)N * (a + 2 * (size_t)b));
}
GQ_DN_HD size_t dn_i5(int M, int N, int m, int n, int j, int q, int l)
{
    return m + (size_t)M * (n + (size_t)N * (j + 2 * (q + 5 * (size_t)l)));
}

// false on NaN and on +-Inf
GQ_DN_HD bool dn_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

// has_var: a variance field is given (v its entry); otherwise every finite f is observed
GQ_DN_HD bool dn_observed(double f, bool has_var, double v)
{
    return dn_finite(f) && (!has_var || (dn_finite(v) && v > 0));
}

// The rules read their constants from a Rule: any struct with K, gama, dta and
// the arrays X, W (Gauss-Hermite nodes and weights) and WW (W[c] * W[r] at
// r + K*c) -- the kernels' parameter block, DnRule on the host.
struct DnRule {
    int K;
    double gama, dta;
    double X[16], W[16], WW[16 * 16];
};

// The two rules are written once, as macros, and wrapped as functions below.
// The kernels expand the macros in their own body, on their parameter block:
// called as functions they bind the block to a reference, the compiler then
// copies all of it to registers up front, merges ZI(c, r) with ZJ(r, c) across
// the unrolled loops and keeps those values live -- 247 VGPRs and 2 waves per
// SIMD where the expanded form takes 132 and 3, and 4.30 ms against 3.92 ms
// for 50 iterations at 388 x 584 (same bits either way).
//
// Node rule (legacy/gqmap_cpu.m:20-26).  KT: K as a constant (0: R.K at run
// time).  so1 = sqrt(2) * sigma.  VM = GQ_DN_VAR_FIELD: var is the entry's
// variance (the scalar without a field) and obs its verdict.  out: 2 doubles.
#define GQ_DN_NODE_RULE(R, KT, VM, so1, u1, f, var, obs, out)                                                         \
    do {                                                                                                              \
        const int K_ = (KT) ? (KT) : (R).K;                                                                           \
        [[maybe_unused]] constexpr int UNR_ = (KT) ? (KT) : 1;                                                        \
        const double PI_ = 3.14159265358979323846;                                                                    \
        double du_ = 0, dsum_ = 0;                                                                                    \
        GQ_DN_UNROLL(UNR_)                                                                                            \
        for (int k_ = 0; k_ < K_; ++k_) {                                                                             \
            const double x_ = (so1) * (R).X[k_] + (u1);                                                               \
            double dval_;                                                                                             \
            if ((VM) == GQ_DN_VAR_ONE) dval_ = (R).W[k_] * ((f) - x_);                                                \
            else if ((VM) == GQ_DN_VAR_SCALAR) dval_ = (R).W[k_] * ((f) - x_) / (var);                                \
            else dval_ = (obs) ? (R).W[k_] * ((f) - x_) / (var) : 0.0;                                                \
            du_ += dval_;                                                                                             \
            dsum_ += dval_ * (R).X[k_];                                                                               \
        }                                                                                                             \
        (out)[0] = du_ / sqrt(PI_);                                                                                   \
        (out)[1] = dsum_ * sqrt(2.0 / PI_);                                                                           \
    } while (0)

// Edge rule (:28-54).  Every expression keeps the reference's operand order;
// what is hoisted is a whole subexpression of it, computed once with the same
// operands: s*XI, t*XI, ds*XI, dt*XI per column c and t*XJ, s*XJ, dt*XJ, ds*XJ
// per row r (when K is a constant: held in registers), sq2*o1 and sq2*o2, WIWJ
// from the host table WW (W[c] * W[r] at r + K*c).
// c2 (the sum of df2 = -df1) is 0 - c1 exactly: both start at +0, IEEE
// addition is symmetric under negation, and an exact-zero sum is +0 in both
// chains -- so column and total sums of df2 are not formed (s2 = 0 - s1).
// GAMA1: gama == 1, where x / 1 == x exactly; DTA_INF: dta == inf, where
// fabs(diff) > dta is false for every diff (NaN included).  out: 5 doubles.
#define GQ_DN_EDGE_RULE(R, KT, GAMA1, DTA_INF, p, o1, u1, o2, u2, out)                                                \
    do {                                                                                                              \
        const int K_ = (KT) ? (KT) : (R).K;                                                                           \
        [[maybe_unused]] constexpr int UNR_ = (KT) ? (KT) : 1;                                                        \
        const double sq2_ = sqrt(2.0), PI_ = 3.14159265358979323846;                                                  \
        const double so1_ = sq2_ * (o1), so2_ = sq2_ * (o2);                                                          \
        const double q_ = sqrt(1 + (p)), r_ = sqrt(1 - (p));                                                          \
        const double s_ = (q_ + r_) / 2, tt_ = (q_ - r_) / 2;                                                         \
        const double ds_ = (1 / q_ - 1 / r_) / 4, dt_ = (1 / q_ + 1 / r_) / 4;                                        \
        double txj_[UNR_], sxj_[UNR_], dtxj_[UNR_], dsxj_[UNR_];                                                      \
        if (KT) {                                                                                                     \
            GQ_DN_UNROLL(UNR_)                                                                                        \
            for (int rr_ = 0; rr_ < UNR_; ++rr_) {                                                                    \
                txj_[rr_] = tt_ * (R).X[rr_];                                                                         \
                sxj_[rr_] = s_ * (R).X[rr_];                                                                          \
                dtxj_[rr_] = dt_ * (R).X[rr_];                                                                        \
                dsxj_[rr_] = ds_ * (R).X[rr_];                                                                        \
            }                                                                                                         \
        }                                                                                                             \
        double s1_ = 0, so1s_ = 0, so2s_ = 0, sp_ = 0;                                                                \
        GQ_DN_UNROLL(UNR_)                                                                                            \
        for (int c_ = 0; c_ < K_; ++c_) { /* sum(sum(A)): column sums first */                                        \
            const double xi_ = (R).X[c_];                                                                             \
            const double sxi_ = s_ * xi_, txi_ = tt_ * xi_, dsxi_ = ds_ * xi_, dtxi_ = dt_ * xi_;                     \
            double c1_ = 0, co1_ = 0, co2_ = 0, cp_ = 0;                                                              \
            GQ_DN_UNROLL(UNR_)                                                                                        \
            for (int rr_ = 0; rr_ < K_; ++rr_) {                                                                      \
                const double xj_ = (R).X[rr_];                                                                        \
                const double tx_ = (KT) ? txj_[rr_] : tt_ * xj_, sx_ = (KT) ? sxj_[rr_] : s_ * xj_;                   \
                const double dtx_ = (KT) ? dtxj_[rr_] : dt_ * xj_, dsx_ = (KT) ? dsxj_[rr_] : ds_ * xj_;              \
                const double ZI_ = sxi_ + tx_, ZJ_ = txi_ + sx_;                                                      \
                const double x1_ = so1_ * ZI_ + (u1), x2_ = so2_ * ZJ_ + (u2);                                        \
                double diff_ = x2_ - x1_;                                                                             \
                if (!(DTA_INF) && fabs(diff_) > (R).dta) diff_ = 0; /* (:44) */                                       \
                const double ww_ = (R).WW[rr_ + K_ * c_];                                                             \
                const double df1_ = (GAMA1) ? ww_ * diff_ : ww_ * diff_ / (R).gama, df2_ = -df1_;                     \
                c1_ += df1_;                                                                                          \
                co1_ += df1_ * ZI_;                                                                                   \
                co2_ += df2_ * ZJ_;                                                                                   \
                cp_ += (o1) * df1_ * (dsxi_ + dtx_) + (o2) * df2_ * (dtxi_ + dsx_);                                   \
            }                                                                                                         \
            s1_ += c1_; so1s_ += co1_; so2s_ += co2_; sp_ += cp_;                                                     \
        }                                                                                                             \
        const double s2_ = 0.0 - s1_;                                                                                 \
        (out)[0] = 1 / PI_ * s1_;                                                                                     \
        (out)[1] = 1 / PI_ * s2_;                                                                                     \
        (out)[2] = 1 / PI_ * sq2_ * so1s_;                                                                            \
        (out)[3] = 1 / PI_ * sq2_ * so2s_;                                                                            \
        (out)[4] = 1 / PI_ * sq2_ * sp_;                                                                              \
    } while (0)

template <int KT, int VM, class Rule>
GQ_DN_HD void dn_node(const Rule &R, double so1, double u1, double f, double var, bool obs, double out[2])
{
    GQ_DN_NODE_RULE(R, KT, VM, so1, u1, f, var, obs, out);
}

template <int KT, bool GAMA1, bool DTA_INF, class Rule>
GQ_DN_HD void dn_edge(const Rule &R, double p, double o1, double u1, double o2, double u2, double out[5])
{
    GQ_DN_EDGE_RULE(R, KT, GAMA1, DTA_INF, p, o1, u1, o2, u2, out);
}

// Sum (:58-59): dmu and dsigma of node (m, n), layer l.  ADJ: the adjoint
// scatter, otherwise the reference's own shift.
template <bool ADJ>
GQ_DN_HD void dn_gather(const double *dnode, const double *de, int M, int N, int m, int n, int l, double &a, double &b)
{
    a = dnode[dn_i4(M, N, m, n, 0, l)] + (de[dn_i5(M, N, m, n, 0, 0, l)] + de[dn_i5(M, N, m, n, 1, 0, l)]);
    b = dnode[dn_i4(M, N, m, n, 1, l)] + (de[dn_i5(M, N, m, n, 0, 2, l)] + de[dn_i5(M, N, m, n, 1, 2, l)]);
    double nu, nl, su, sl;
    if (ADJ) {
        nu = m >= 1 ? de[dn_i5(M, N, m - 1, n, 0, 1, l)] : 0.0;
        nl = n >= 1 ? de[dn_i5(M, N, m, n - 1, 1, 1, l)] : 0.0;
        su = m >= 1 ? de[dn_i5(M, N, m - 1, n, 0, 3, l)] : 0.0;
        sl = n >= 1 ? de[dn_i5(M, N, m, n - 1, 1, 3, l)] : 0.0;
    } else {
        nu = m + 1 < M ? de[dn_i5(M, N, m + 1, n, 0, 1, l)] : 0.0;
        nl = n + 1 < N ? de[dn_i5(M, N, m, n + 1, 1, 1, l)] : 0.0;
        su = m + 1 < M ? de[dn_i5(M, N, m + 1, n, 0, 3, l)] : 0.0;
        sl = n + 1 < N ? de[dn_i5(M, N, m, n + 1, 1, 3, l)] : 0.0;
    }
    a = a + (nu + nl);
    b = b + (su + sl);
}

GQ_DN_HD double dn_step(double step0, int it, double step_decay) { return step0 / (1 + it / step_decay); }  // (:62)

// Step and clamps (:63-65) of node (m, n), layer l; returns max_j |dedge(m,n,j,4,l)|.
GQ_DN_HD double dn_apply(double *mu, double *sigma, double *rou, const double *de, int M, int N, int m, int n, int l,
                         double a, double b, double step, double corr)
{
    double mp = 0;
    const size_t q = dn_i3(M, N, m, n, l);
    mu[q] = mu[q] + a * step;              // (:63)
    sigma[q] = fabs(sigma[q] + b * step);  // (:64)
    for (int j = 0; j < 2; ++j) {          // (:65)
        const double d = de[dn_i5(M, N, m, n, j, 4, l)];
        mp = fmax(mp, fabs(d));
        const size_t r = dn_i4(M, N, m, n, j, l);
        rou[r] = fmax(fmin(rou[r] + d * step, corr), -corr);
    }
    return mp;
}

// |v| as its bit pattern: for |v| >= 0 (and NaN above +inf) the unsigned
// order of the bits is the order of the values, so max is exact in any order
GQ_DN_HD unsigned long long dn_abits(double v)
{
    const double a = fabs(v);
    unsigned long long u;
    __builtin_memcpy(&u, &a, sizeof u);
    return u;
}
GQ_DN_HD double dn_from_bits(unsigned long long u)
{
    double v;
    __builtin_memcpy(&v, &u, sizeof v);
    return v;
}

// the stop rule (:70) after iteration it, mx = its max|dmu|
GQ_DN_HD bool dn_stop(int it, int its, int min_its, double mx, double tor)
{
    return it + 1 > its || (it + 1 > min_its && mx < tor);
}

}  // namespace gq
