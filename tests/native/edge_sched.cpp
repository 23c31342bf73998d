// edge_sched.cpp -- host check of edge_sums_range_sched (TEST INFRASTRUCTURE,
// built and run by tests/test_edge_sched.py).
//
// edge_sums_range_sched is edge_sums_range with a pair's table rows read a
// pair ahead and its two roots taken side by side (gqmap_math.h).  Here every
// form of it (SCHED = 1, 2, 3) runs against edge_sums in one piece on the same
// operands, gqmap_math.h compiled as the CPU model compiles it: the whole
// range from zero, with and without the centre point (without: against
// edge_sums_range), and the halo chain's four slices carried through memory
// for the equal cut and the kernel's (GQ_FLOW_HALO_EPI = 0 and 8).  The table
// is allocated at exactly K^2 rows behind a guard row of signalling values, so
// a read past the last row shows in the sums.  Operand sets: random ones, half
// of them with the correlation at or next to its clamps, and sets that make d
// exactly 0 (C = 0: the centre's d is 0 and a pair's fp = fm; C = -p_k for a
// pair k: its dp is 0, the root sqrt(eps)).  The six sums must be identical
// bits.
// One line per case on stdout:
//   <type> K=<K> pairs=<n> centre=<0|1> empty_slices=<n> empty_kernel=<n> one_pair_kernel=<n> sets=<n> zero_d=<n> mismatches=<n>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

namespace gq {
using std::floor;
using std::fma;
using std::fmax;
using std::fmin;
}  // namespace gq
#define GQ_HD inline
#define GQ_SQRT(x) std::sqrt(x)
#define GQ_UNROLL2
#define GQ_PAIR_UNROLL
#define GQ_PAIR_UNROLL_K(n)
#define GQ_NODE_UNROLL
#define GQ_UNROLL_FULL
#include "../../gqmap-opticalflow_amd/csrc/gqmap_math.h"

using namespace gq;

namespace {

struct Rng {  // splitmix64
    uint64_t s;
    uint64_t next()
    {
        uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
};

// a K x K product rule laid out as gqmap_create lays out its table (symmetric
// nodes, Gaussian weights), K^2 rows and one guard row of NaNs behind them
template <typename R>
std::vector<R> table(int K)
{
    std::vector<double> X(K), W(K);
    std::vector<R> tab((size_t)NTAB * (K * K + 1), std::numeric_limits<R>::quiet_NaN());
    const double xmax = 0.5 * std::sqrt(2.0 * K + 1.0) + 0.6 * (K - 2) / 3.0;
    double wsum = 0;
    for (int i = 0; i < K; ++i) {
        X[i] = -xmax + 2 * xmax * i / (K - 1);
        if (2 * i + 1 == K) X[i] = 0.0;
        W[i] = std::exp(-X[i] * X[i]);
        wsum += W[i];
    }
    for (int i = 0; i < K; ++i) W[i] /= wsum;
    for (int cc = 0; cc < K; ++cc)
        for (int r = 0; r < K; ++r) {
            const int k = r + K * cc;
            const double xi = X[cc], xj = X[r], ww = W[cc] * W[r];
            tab[tab_at(T_XI, k)] = R(xi);
            tab[tab_at(T_XJ, k)] = R(xj);
            tab[tab_at(T_W, k)] = R(ww);
            tab[tab_at(T_WXI, k)] = R(ww * xi);
            tab[tab_at(T_WXJ, k)] = R(ww * xj);
            tab[tab_at(T_WA, k)] = R(ww * (xi * xi + xj * xj));
            tab[tab_at(T_WM, k)] = R(ww * (xi * xi - xj * xj));
            tab[tab_at(T_WX, k)] = R(ww * (xi * xj));
        }
    return tab;
}

template <typename R>
bool same_bits(const Sums<R> &a, const Sums<R> &b)
{
    const R x[6] = {a.s0, a.sxi, a.sxj, a.sa, a.sm, a.sx}, y[6] = {b.s0, b.sxi, b.sxj, b.sa, b.sm, b.sx};
    return memcmp(x, y, sizeof x) == 0;
}

constexpr int SETS = 400;
constexpr int KERNEL_EPI = 8;  // GQ_FLOW_HALO_EPI's default (gqmap_tuning.h)
constexpr double CORR = 0.99;  // the engine's clamp of a correlation (corr_tor = 0.01)

// the four slices of one cut, each continuing the sums the one before left in memory
template <int SCHED, typename R>
Sums<R> chained(const R *tp, int K2, int epi, R eps, const EdgeCoef<R> &c)
{
    const int np = K2 >> 1;
    volatile R pass[6] = {0, 0, 0, 0, 0, 0};
    for (int w = 0; w < 4; ++w) {
        Sums<R> S;
        S.s0 = pass[0]; S.sxi = pass[1]; S.sxj = pass[2]; S.sa = pass[3]; S.sm = pass[4]; S.sx = pass[5];
        edge_sums_range_sched<SCHED>(tp, chain_cut(np, w, epi), chain_cut(np, w + 1, epi), K2, w == 3, eps, c, S);
        pass[0] = S.s0; pass[1] = S.sxi; pass[2] = S.sxj; pass[3] = S.sa; pass[4] = S.sm; pass[5] = S.sx;
    }
    Sums<R> got;
    got.s0 = pass[0]; got.sxi = pass[1]; got.sxj = pass[2]; got.sa = pass[3]; got.sm = pass[4]; got.sx = pass[5];
    return got;
}

template <int SCHED, typename R>
int check(const R *tp, int K2, R eps, const EdgeCoef<R> &c, const Sums<R> &ref, const Sums<R> &ref_nc)
{
    const int np = K2 >> 1;
    int bad = 0;
    Sums<R> one;  // the whole range from zero, centre on: edge_sums itself
    edge_sums_range_sched<SCHED>(tp, 0, np, K2, true, eps, c, one);
    bad += !same_bits(ref, one);
    Sums<R> nc;  // centre off
    edge_sums_range_sched<SCHED>(tp, 0, np, K2, false, eps, c, nc);
    bad += !same_bits(ref_nc, nc);
    for (int epi : {0, KERNEL_EPI}) bad += !same_bits(ref, chained<SCHED>(tp, K2, epi, eps, c));
    return bad;
}

template <typename R>
int run_K(const char *type, int K)
{
    const std::vector<R> tab = table<R>(K);
    const R *tp = tab.data();
    const int K2 = K * K, np = K2 >> 1;
    const R eps = R(1e-6);
    Rng g{991u + (uint64_t)K};
    int bad = 0, zero_d = 0, empty = 0, empty_k = 0, one_k = 0;
    for (int w = 0; w < 4; ++w) {
        empty += (np * w) / 4 == (np * (w + 1)) / 4;
        empty_k += chain_cut(np, w, KERNEL_EPI) == chain_cut(np, w + 1, KERNEL_EPI);
        one_k += chain_cut(np, w + 1, KERNEL_EPI) - chain_cut(np, w, KERNEL_EPI) == 1;
    }
    for (int s = 0; s < SETS; ++s) {
        const R u1 = R((g.uni() - 0.5) * 16), u2 = R((g.uni() - 0.5) * 16);
        const bool small = g.uni() < 0.3;
        const R o1 = R(small ? 0.05 + 0.3 * g.uni() : 0.5 + 5.5 * g.uni());
        const R o2 = R(small ? 0.05 + 0.3 * g.uni() : 0.5 + 5.5 * g.uni());
        R p = R((g.uni() - 0.5) * 1.96);
        const int edge = s % 8;
        if (edge == 0) p = R(CORR);
        if (edge == 1) p = R(-CORR);
        if (edge == 2 || edge == 3) p = R((edge == 2 ? 1 : -1) * (CORR - 1e-4 * g.uni()));
        EdgeCoef<R> c = edge_coef(u1, u2, o1, o2, p);
        // d exactly 0: equal means (C = 0: the centre point, and fp = fm in
        // every pair), and means u1 = -p_k, u2 = 0 for one pair k (C = -p_k:
        // that pair's dp = C + p_k)
        if (s % 16 == 5) {
            c = edge_coef(u1, u1, o1, o2, p);
            bad += c.C != R(0);
            ++zero_d;
        }
        if (s % 16 == 13) {
            const int kz = (s / 16) % np;
            const R pk = fma(c.A, tp[tab_at(T_XI, kz)], c.B * tp[tab_at(T_XJ, kz)]);
            c = edge_coef(-pk, R(0), o1, o2, p);
            bad += c.C + pk != R(0);
            ++zero_d;
        }
        const Sums<R> ref = edge_sums(tp, 0, K2, 1, eps, c);
        Sums<R> ref_nc;
        edge_sums_range(tp, 0, np, K2, false, eps, c, ref_nc);
        bad += !(ref.s0 > R(0));  // (a guard row read would make it NaN)
        bad += check<1>(tp, K2, eps, c, ref, ref_nc);
        bad += check<2>(tp, K2, eps, c, ref, ref_nc);
        bad += check<3>(tp, K2, eps, c, ref, ref_nc);
    }
    printf("%s K=%d pairs=%d centre=%d empty_slices=%d empty_kernel=%d one_pair_kernel=%d sets=%d zero_d=%d mismatches=%d\n",
           type, K, np, K2 & 1, empty, empty_k, one_k, SETS, zero_d, bad);
    return bad;
}

template <typename R>
int run_type(const char *type)
{
    int bad = 0;
    for (int K = 2; K <= 16; ++K) bad += run_K<R>(type, K);
    return bad;
}

}  // namespace

int main()
{
    const int bad = run_type<double>("double") + run_type<float>("float");
    return bad ? 1 : 0;
}
