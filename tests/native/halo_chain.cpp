// halo_chain.cpp -- host check of edge_sums_range (TEST INFRASTRUCTURE, built
// and run by tests/test_halo_chain.py).
//
// The dataflow item's halo chain cuts an edge's pair range [0, K^2/2) into four
// consecutive slices, [chain_cut(w), chain_cut(w + 1)) for w = 0..3, each
// continuing the six sums the one before left, the last one taking the centre
// point.  Two cuts: four equal slices, [np w / 4, np (w + 1) / 4), and the
// kernel's (a last slice shorter by KERNEL_EPI pairs' worth of epilogue).
// Here that carried form runs against edge_sums in one piece on the same
// operands (gqmap_math.h compiled as the CPU model compiles it): the six sums
// must agree bit for bit.  One line per case on stdout:
//   <type> K=<K> pairs=<n> centre=<0|1> empty_slices=<n> empty_kernel=<n> sets=<n> near_corr=<n> mismatches=<n>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
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

// a K x K product rule laid out as gqmap_create lays out its table: symmetric
// nodes, Gaussian weights
std::vector<double> table(int K)
{
    std::vector<double> X(K), W(K), tab(NTAB * TAB_STRIDE, 0.0);
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
            tab[tab_at(T_XI, k)] = xi;
            tab[tab_at(T_XJ, k)] = xj;
            tab[tab_at(T_W, k)] = ww;
            tab[tab_at(T_WXI, k)] = ww * xi;
            tab[tab_at(T_WXJ, k)] = ww * xj;
            tab[tab_at(T_WA, k)] = ww * (xi * xi + xj * xj);
            tab[tab_at(T_WM, k)] = ww * (xi * xi - xj * xj);
            tab[tab_at(T_WX, k)] = ww * (xi * xj);
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

template <typename R>
int run_K(const char *type, int K)
{
    const auto tabd = table(K);
    const std::vector<R> tab(tabd.begin(), tabd.end());
    const R *tp = tab.data();
    const int K2 = K * K, np = K2 >> 1;
    const R eps = R(1e-6);
    Rng g{777u + (uint64_t)K};
    int bad = 0, near = 0, empty = 0, empty_k = 0;
    for (int w = 0; w < 4; ++w) {
        empty += (np * w) / 4 == (np * (w + 1)) / 4;
        empty_k += chain_cut(np, w, KERNEL_EPI) == chain_cut(np, w + 1, KERNEL_EPI);
        bad += chain_cut(np, w, 0) != (np * w) / 4 || chain_cut(np, w, KERNEL_EPI) > chain_cut(np, w + 1, KERNEL_EPI);
    }
    bad += chain_cut(np, 0, KERNEL_EPI) != 0 || chain_cut(np, 4, KERNEL_EPI) != np || chain_cut(np, 4, 0) != np;
    for (int s = 0; s < SETS; ++s) {
        const R u1 = R((g.uni() - 0.5) * 16), u2 = R((g.uni() - 0.5) * 16);
        const bool small = g.uni() < 0.3;
        const R o1 = R(small ? 0.05 + 0.3 * g.uni() : 0.5 + 5.5 * g.uni());
        const R o2 = R(small ? 0.05 + 0.3 * g.uni() : 0.5 + 5.5 * g.uni());
        // a quarter of the sets at or next to the clamps +-corr
        R p = R((g.uni() - 0.5) * 1.96);
        const int edge = s % 8;
        if (edge == 0) p = R(CORR);
        if (edge == 1) p = R(-CORR);
        if (edge == 2 || edge == 3) p = R((edge == 2 ? 1 : -1) * (CORR - 1e-4 * g.uni()));
        near += edge < 4;
        const EdgeCoef<R> c = edge_coef(u1, u2, o1, o2, p);
        const Sums<R> ref = edge_sums(tp, 0, K2, 1, eps, c);
        // the chain: wave w continues from the sums wave w - 1 passed on
        // (through memory, as the kernel passes them through LDS)
        for (int epi : {0, KERNEL_EPI}) {
            volatile R pass[6] = {0, 0, 0, 0, 0, 0};
            for (int w = 0; w < 4; ++w) {
                Sums<R> S;
                S.s0 = pass[0]; S.sxi = pass[1]; S.sxj = pass[2]; S.sa = pass[3]; S.sm = pass[4]; S.sx = pass[5];
                edge_sums_range(tp, chain_cut(np, w, epi), chain_cut(np, w + 1, epi), K2, w == 3, eps, c, S);
                pass[0] = S.s0; pass[1] = S.sxi; pass[2] = S.sxj; pass[3] = S.sa; pass[4] = S.sm; pass[5] = S.sx;
            }
            Sums<R> got;
            got.s0 = pass[0]; got.sxi = pass[1]; got.sxj = pass[2]; got.sa = pass[3]; got.sm = pass[4]; got.sx = pass[5];
            bad += !same_bits(ref, got);
        }
        bad += !(ref.s0 > R(0));
        // the whole range in one call is edge_sums itself
        Sums<R> one;
        edge_sums_range(tp, 0, np, K2, true, eps, c, one);
        bad += !same_bits(ref, one);
    }
    printf("%s K=%d pairs=%d centre=%d empty_slices=%d empty_kernel=%d sets=%d near_corr=%d mismatches=%d\n", type, K, np,
           K2 & 1, empty, empty_k, SETS, near, bad);
    return bad;
}

template <typename R>
int run_type(const char *type)
{
    int bad = 0;
    for (int K : {2, 3, 4, 9, 11, 16}) bad += run_K<R>(type, K);
    return bad;
}

}  // namespace

int main()
{
    const int bad = run_type<double>("double") + run_type<float>("float");
    return bad ? 1 : 0;
}
