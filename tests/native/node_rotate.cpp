// node_rotate.cpp -- host check of node_sums' loop forms (TEST INFRASTRUCTURE,
// built and run by tests/test_node_rotate.py).
//
// node_sums<0, true, false> (the straight loop) against the pipelined form
// and every rotated form of it (gqmap_math.h, ROT) on the same inputs: the six
// sums must agree bit for bit.  One line per case on stdout:
//   <type> K=<K> k0=<k0> dk=<dk> samples=<n> form=<name> nodes=<n> clamped=<n> mismatches=<n>
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

constexpr int MO = 24, NO = 24, M2 = MO + 2;

// the padded frame as the engine builds it (getVV): the frame inside a border
// of 3 a - 3 b + c extrapolations, then the zero tail of vv_elems
std::vector<double> padded_frame(const std::vector<double> &V)
{
    const int N2 = NO + 2, M2N2 = M2 * N2;
    std::vector<double> VV(vv_elems(MO, NO), 0.0);
    for (int n = 0; n < NO; ++n)
        for (int m = 0; m < MO; ++m) VV[(m + 1) + (size_t)M2 * (n + 1)] = V[m + (size_t)MO * n];
    for (int i = 0; i < N2; ++i) {
        const int ix = M2 * i, iy = ix + M2 - 1;
        VV[ix] = (3.0 * VV[ix + 1] - 3.0 * VV[ix + 2]) + VV[ix + 3];
        VV[iy] = (3.0 * VV[iy - 1] - 3.0 * VV[iy - 2]) + VV[iy - 3];
    }
    for (int i = 0; i < M2; ++i) {
        VV[i] = (3.0 * VV[M2 + i] - 3.0 * VV[M2 * 2 + i]) + VV[M2 * 3 + i];
        VV[M2N2 - M2 + i] = (3.0 * VV[M2N2 - M2 * 2 + i] - 3.0 * VV[M2N2 - M2 * 3 + i]) + VV[M2N2 - M2 * 4 + i];
    }
    return VV;
}

// a K x K product rule laid out as gqmap_create lays out its table: symmetric
// nodes over the Gauss-Hermite range of that K, Gaussian weights
std::vector<double> table(int K)
{
    std::vector<double> X(K), W(K), tab(NTAB * TAB_STRIDE, 0.0);
    const double xmax = K == 2 ? 0.7071067811865476 : K == 3 ? 1.224744871391589 : 3.190993201781528;
    double wsum = 0;
    for (int i = 0; i < K; ++i) {
        X[i] = K == 1 ? 0.0 : -xmax + 2 * xmax * i / (K - 1);
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
struct Inputs {
    std::vector<R> VV, I1;
    struct Node {
        int m, n;
        R u1, u2, o1, o2, p;
    };
    std::vector<Node> nodes;
};

template <typename R>
Inputs<R> make_inputs()
{
    Rng g{12345};
    std::vector<double> I2(MO * NO), I1(MO * NO);
    for (auto &v : I2) v = (double)(int)(g.uni() * 256);
    for (auto &v : I1) v = (double)(int)(g.uni() * 256);
    const auto VV = padded_frame(I2);
    Inputs<R> in;
    in.VV.assign(VV.begin(), VV.end());
    in.I1.assign(I1.begin(), I1.end());
    // every fourth node; means up to 8 px and sigmas up to 6 px, so near the
    // border the samples fall on both sides of the clamps and in the middle
    // (small sigma) on neither
    for (int n = 0; n < NO; n += 2)
        for (int m = (n / 2) % 2; m < MO; m += 2) {
            typename Inputs<R>::Node nd;
            nd.m = m; nd.n = n;
            nd.u1 = R((g.uni() - 0.5) * 16);
            nd.u2 = R((g.uni() - 0.5) * 16);
            const bool small = g.uni() < 0.3;
            nd.o1 = R(small ? 0.05 + 0.3 * g.uni() : 0.5 + 5.5 * g.uni());
            nd.o2 = R(small ? 0.05 + 0.3 * g.uni() : 0.5 + 5.5 * g.uni());
            nd.p = R((g.uni() - 0.5) * 1.8);
            in.nodes.push_back(nd);
        }
    return in;
}

template <typename R>
bool same_bits(const Sums<R> &a, const Sums<R> &b)
{
    const R x[6] = {a.s0, a.sxi, a.sxj, a.sa, a.sm, a.sx}, y[6] = {b.s0, b.sxi, b.sxj, b.sa, b.sm, b.sx};
    return memcmp(x, y, sizeof x) == 0;
}

template <typename R, bool PF, int ROT>
int compare(const char *type, const char *form, const Inputs<R> &in, const std::vector<R> &tab, int K, int k0, int dk)
{
    const int K2 = K * K;
    const R eps = R(1e-3), xmax = R(K == 2 ? 0.7071067811865476 : K == 3 ? 1.224744871391589 : 3.190993201781528);
    const R *tp = tab.data(), *I1 = in.I1.data();
    const auto fv = frame_view(in.VV.data(), M2);
    int bad = 0, clamped = 0;
    for (const auto &nd : in.nodes) {
        const NodeCoef<R> c = node_coef(nd.o1, nd.o2, nd.p);
        clamped += !node_unclamped(c, nd.u1, nd.u2, nd.m, nd.n, MO, NO, xmax);
        const Sums<R> ref = node_sums<0, true, false>(tp, k0, K2, dk, fv, I1, MO, NO, eps, c, nd.u1, nd.u2, nd.m, nd.n);
        const Sums<R> got = node_sums<0, true, PF, ROT>(tp, k0, K2, dk, fv, I1, MO, NO, eps, c, nd.u1, nd.u2, nd.m, nd.n);
        bad += !same_bits(ref, got);
        if (k0 >= K2) bad += !same_bits(got, Sums<R>{});  // no sample: the sums stay zero
    }
    const int samples = k0 < K2 ? (K2 - 1 - k0) / dk + 1 : 0;
    printf("%s K=%d k0=%d dk=%d samples=%d form=%s nodes=%d clamped=%d mismatches=%d\n", type, K, k0, dk, samples,
           form, (int)in.nodes.size(), clamped, bad);
    return bad;
}

template <typename R>
int run_type(const char *type)
{
    const Inputs<R> in = make_inputs<R>();
    int bad = 0;
    for (int K : {2, 3, 9}) {
        const auto tabd = table(K);
        const std::vector<R> tab(tabd.begin(), tabd.end());
        const int K2 = K * K;
        // (k0, dk) of the lanes-per-node splits, then a lane with exactly one
        // sample and a lane with none
        const int pairs[5][2] = {{0, 1}, {1, 2}, {3, 4}, {K2 - 1, 16}, {K2, 16}};
        for (const auto &pr : pairs) {
            const int k0 = pr[0], dk = pr[1];
            bad += compare<R, true, 0>(type, "pf", in, tab, K, k0, dk);
            bad += compare<R, true, NODE_UNROLL(4)>(type, "pf4", in, tab, K, k0, dk);
            bad += compare<R, true, NODE_ROT>(type, "rot", in, tab, K, k0, dk);
            bad += compare<R, true, NODE_ROT | NODE_ROT_STAGE>(type, "staged", in, tab, K, k0, dk);
            bad += compare<R, true, NODE_ROT | NODE_ROT_STAGE | NODE_UNROLL(2)>(type, "staged2", in, tab, K, k0, dk);
        }
    }
    return bad;
}

}  // namespace

int main()
{
    const int bad = run_type<double>("double") + run_type<float>("float");
    return bad ? 1 : 0;
}
