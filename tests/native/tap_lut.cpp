// tap_lut.cpp -- host check of the offset store's arithmetic (TEST
// INFRASTRUCTURE, built and run by tests/test_tap_lut.py).
//
// The fp64 mixture item of the dataflow launch reads integer frames through an
// offset store (gqmap_math.h vvo2_t): a tap is the entry of a table of doubles
// at the 16-bit byte offset the store holds, where the binary16 pair store
// converts binary16 -> float -> double.  Here, with gqmap_math.h compiled as
// the CPU model compiles it:
//   node   node_sums on the offset store (node_sums_lut: the table reads, the
//          trips written out 1 and 4 per pass) against node_sums' pipelined
//          loop on a float store of the same frame, clamped and clamp-free,
//          K = 2..16: the six sums bit for bit;
//   table  every integer of [-510, 765] through taplut_offset / taplut_entry
//          against the conversion chain (a software binary16 round trip, then
//          float, then double), for tables starting at -510, at the value and
//          in between; the offsets' form (multiples of 8 below 8 TAPLUT_N).
// One line per case on stdout:
//   node K=<K> sets=<n> clamped_samples=<n> free_sets=<n> mismatches=<n>
//   table values=<n> mismatches=<n>
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
    int below(int n) { return (int)(next() % (uint64_t)n); }
};

// a K x K product rule laid out as gqmap_create lays out its table
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

bool same_bits(const Sums<double> &a, const Sums<double> &b)
{
    const double x[6] = {a.s0, a.sxi, a.sxj, a.sa, a.sm, a.sx}, y[6] = {b.s0, b.sxi, b.sxj, b.sa, b.sm, b.sx};
    return memcmp(x, y, sizeof x) == 0;
}

// double -> binary16 (round to nearest even) -> float: the pair store's first
// conversion and its widening, in integer arithmetic
float through_binary16(double v)
{
    if (v == 0.0) return 0.0f;
    int e;
    const double m = std::frexp(std::fabs(v), &e);  // |v| = m 2^e, m in [0.5, 1)
    // 11 significant bits (normal numbers: |v| >= 2^-14, all that occur here)
    const double scaled = std::ldexp(m, 11);
    double q = std::floor(scaled);
    const double rem = scaled - q;
    if (rem > 0.5 || (rem == 0.5 && std::fmod(q, 2.0) == 1.0)) q += 1.0;
    const double r = std::ldexp(q, e - 11);
    return (float)(v < 0 ? -r : r);
}

constexpr int MO = 24, NO = 20;

struct Frame {
    std::vector<float> vf;     // today's store on the host: float, exact
    std::vector<vvo2_t> vo;    // the offset store, as gqmap_set_images lays it out
    std::vector<double> lut;   // the table the kernel fills
    std::vector<double> I1;
};

Frame frame(Rng &g)
{
    const size_t M2 = MO + 2, N2 = NO + 2, ne = vv_elems(MO, NO);
    std::vector<int> vv(M2 * N2);
    for (int &v : vv) v = -510 + g.below(TAPLUT_N);
    vv[g.below((int)vv.size())] = -510;  // both ends of the table
    vv[g.below((int)vv.size() - 1) + 1] = 765;
    int vmin = 0, vmax = 0;  // (0: the zero column and the tail)
    for (int v : vv) {
        vmin = v < vmin ? v : vmin;
        vmax = v > vmax ? v : vmax;
    }
    Frame F;
    F.vf.assign(ne, 0.0f);
    const uint16_t zero = taplut_offset(0, vmin);
    F.vo.assign(ne, vvo2_t{zero, zero});
    for (size_t cc = 0; cc < N2; ++cc)
        for (size_t r = 0; r < M2; ++r) {
            F.vf[r + M2 * cc] = (float)vv[r + M2 * cc];
            F.vo[r + M2 * cc].lo = taplut_offset(vv[r + M2 * cc], vmin);
            if (cc + 1 < N2) F.vo[r + M2 * cc].hi = taplut_offset(vv[r + M2 * (cc + 1)], vmin);
        }
    F.lut.resize(vmax - vmin + 1);
    for (int i = 0; i < (int)F.lut.size(); ++i) F.lut[i] = taplut_entry(i, vmin);
    F.I1.resize((size_t)MO * NO);
    for (double &v : F.I1) v = (double)g.below(256);
    return F;
}

int run_K(int K)
{
    const auto tab = table(K);
    const double *tp = tab.data();
    const int K2 = K * K;
    const double eps = 1e-6;
    double xmax = 0;
    for (int k = 0; k < K2; ++k) xmax = std::fmax(xmax, std::fabs(tab[tab_at(T_XI, k)]));
    Rng g{4242u + (uint64_t)K};
    int bad = 0, sets = 0, free_sets = 0;
    long clamped = 0;
    for (int f = 0; f < 6; ++f) {
        const Frame F = frame(g);
        const auto fv = frame_view(F.vf.data(), MO + 2);
        const auto lv = frame_view_lut(F.vo.data(), MO + 2, F.lut.data());
        for (int s = 0; s < 40; ++s, ++sets) {
            const bool small = s % 4 == 0;  // a quarter of the sets: small sigma at an inner node (clamp-free)
            const int m = small ? 8 + g.below(MO - 16) : g.below(MO), n = small ? 8 + g.below(NO - 16) : g.below(NO);
            const double o1 = small ? 0.05 + 0.5 * g.uni() : 0.5 + 22.5 * g.uni();
            const double o2 = small ? 0.05 + 0.5 * g.uni() : 0.5 + 22.5 * g.uni();
            const double p = (g.uni() - 0.5) * 1.96;
            const double u1 = (g.uni() - 0.5) * (small ? 2 : 12), u2 = (g.uni() - 0.5) * (small ? 2 : 12);
            const NodeCoef<double> c = node_coef(o1, o2, p);
            for (int k = 0; k < K2; ++k) {  // (for the record: samples the clamps act on)
                const double X = fma(c.ax, tp[tab_at(T_XI, k)], fma(c.bx, tp[tab_at(T_XJ, k)], u1 + double(n + 1)));
                const double Y = fma(c.ay, tp[tab_at(T_XI, k)], fma(c.by, tp[tab_at(T_XJ, k)], u2 + double(m + 1)));
                clamped += X < 1 || X > NO || Y < 1 || Y > MO;
            }
            const Sums<double> ref = node_sums<0, true, true, NODE_UNROLL(4)>(tp, 0, K2, 1, fv, F.I1.data(), MO, NO, eps, c,
                                                                              u1, u2, m, n);
            const Sums<double> g1 = node_sums<0, true, true, 0>(tp, 0, K2, 1, lv, F.I1.data(), MO, NO, eps, c, u1, u2, m, n);
            const Sums<double> g4 = node_sums<0, true, true, NODE_UNROLL(4)>(tp, 0, K2, 1, lv, F.I1.data(), MO, NO, eps, c,
                                                                             u1, u2, m, n);
            bad += !same_bits(ref, g1) + !same_bits(ref, g4) + !(ref.s0 > 0);
            if (node_unclamped(c, u1, u2, m, n, MO, NO, xmax)) {
                ++free_sets;
                const Sums<double> rf = node_sums<0, false, true, NODE_UNROLL(4)>(tp, 0, K2, 1, fv, F.I1.data(), MO, NO, eps,
                                                                                 c, u1, u2, m, n);
                const Sums<double> gf = node_sums<0, false, true, NODE_UNROLL(4)>(tp, 0, K2, 1, lv, F.I1.data(), MO, NO, eps,
                                                                                 c, u1, u2, m, n);
                bad += !same_bits(rf, gf) + !same_bits(rf, ref);
            }
        }
    }
    printf("node K=%d sets=%d clamped_samples=%ld free_sets=%d mismatches=%d\n", K, sets, clamped, free_sets, bad);
    return bad;
}

int run_table()
{
    int bad = 0, n = 0;
    for (int v = -510; v <= 765; ++v, ++n) {
        const double chain = (double)through_binary16((double)v);
        bad += chain != (double)v;  // (the pair store's own condition: the frame's values are exact in binary16)
        const int top = v < 0 ? v : 0;  // a table starts at or below the value and at or below 0
        for (int vmin : {-510, top, (top - 510) / 2}) {
            if (v - vmin >= TAPLUT_N) continue;
            const uint16_t o = taplut_offset(v, vmin);
            bad += o % 8 != 0 || o / 8 >= TAPLUT_N || (int)o != (v - vmin) * 8;
            const double e = taplut_entry(o / 8, vmin);
            bad += memcmp(&e, &chain, sizeof e) != 0;
        }
    }
    bad += n != TAPLUT_N;
    // binary16 itself: the round trip rounds (2049 is not a binary16 value; 2048 and 2050 are)
    bad += through_binary16(2049.0) != 2048.0f || through_binary16(2051.0) != 2052.0f || through_binary16(-0.5) != -0.5f;
    printf("table values=%d mismatches=%d\n", n, bad);
    return bad;
}

}  // namespace

int main()
{
    int bad = run_table();
    for (int K = 2; K <= 16; ++K) bad += run_K(K);
    return bad ? 1 : 0;
}
