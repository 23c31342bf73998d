// item_trim.cpp -- host check of the trimmed dataflow item's address forms
// (TEST INFRASTRUCTURE, built and run by tests/test_item_trim.py).
//
// The fp64 mixture item on the offset store reads its taps through a view
// with biased bases (gqmap_math.h TapViewLutBiased) and addresses its edge
// operands by 32-bit element offsets (edge_elem32, edge_plane_elem32, where
// edge_addr32_ok holds).  Here, with gqmap_math.h compiled as the CPU model
// compiles it:
//   bias   every cell (iy, ix) of [1, Mo] x [1, No]: the biased index on the
//          two biased bases addresses the elements cell_elem and + 2 M2 name,
//          inside the buffer, and view_taps16 returns load_taps16's taps;
//   addr   node (m, n) and plane 0..8: the 32-bit element offset against the
//          64-bit index m + M n + loff + MNL plane;
//   ok     edge_addr32_ok at a size;
//   node   node_sums_lut through the biased view against the present view,
//          clamped and clamp-free, 1 and 4 trips per pass: the six sums bit
//          for bit.
// One line per case on stdout:
//   bias Mo=<Mo> No=<No> cells=<n> last_byte_slack=<n> mismatches=<n>
//   addr M=<M> N=<N> L=<L> checks=<n> mismatches=<n>
//   ok M=<M> N=<N> L=<L> bytes=<b> ok=<0|1>
//   node K=<K> sets=<n> clamped_samples=<n> free_sets=<n> mismatches=<n>
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

// Every cell of an Mo x No frame: the addresses and the taps of the biased view.
int run_bias(int Mo, int No)
{
    const int M2 = Mo + 2;
    const size_t ne = vv_elems(Mo, No);
    std::vector<vvo2_t> vo(ne);
    for (size_t i = 0; i < ne; ++i) vo[i] = vvo2_t{(uint16_t)(i * 2654435761u >> 7), (uint16_t)(i * 40503u + 1)};  // (every element its own word)
    const double *nolut = nullptr;
    const auto pv = frame_view_lut(vo.data(), M2, nolut);
    const auto bv = frame_view_lut_biased(vo.data(), M2, nolut);
    const uintptr_t base = (uintptr_t)vo.data(), end = base + ne * sizeof(vvo2_t);
    long bad = 0, cells = 0;
    uintptr_t top = 0;
    for (int ix = 1; ix <= No; ++ix)
        for (int iy = 1; iy <= Mo; ++iy, ++cells) {
            const uint32_t o = pv.cell(iy, ix), ob = bv.cell(iy, ix);
            const uintptr_t a0 = bv.b0 + (uintptr_t)ob * 4, a2 = bv.b2 + (uintptr_t)ob * 4;
            bad += a0 != base + (uintptr_t)o * 4;
            bad += a2 != base + ((uintptr_t)o + 2u * (uint32_t)M2) * 4;
            bad += a0 < base || a2 + 16 > end;  // four rows of a column pair from either base
            top = a2 + 16 > top ? a2 + 16 : top;
            const auto T = load_taps16(pv.p, o, pv.ld);
            const auto B = view_taps16(bv, ob);
            bad += memcmp(T.v, B.v, sizeof T.v) != 0;
            bad += memcmp(B.v, &vo[o], 16) != 0 || memcmp(B.v + 4, &vo[o + 2 * M2], 16) != 0;
        }
    bad += bv.cell(1, 1) != tap_bias_elems(M2) || bv.b0 + 4 * (uintptr_t)tap_bias_elems(M2) != base;
    // cell (Mo, No): its last element is (Mo + 2)(No + 2), the first of the zero
    // column (its high half, column No + 3, is the last tap)
    bad += top != base + ((size_t)(Mo + 2) * (No + 2) + 1) * 4;
    printf("bias Mo=%d No=%d cells=%ld last_byte_slack=%ld mismatches=%ld\n", Mo, No, cells, (long)(end - top), bad);
    return bad != 0;
}

// 32-bit element offsets against the 64-bit index: every node when `all`,
// else the corners, the edges' ends and a stride through the grid.
int run_addr(int M, int N, int L, bool all)
{
    const int64_t MN = (int64_t)M * N, MNL = MN * L;
    long bad = 0, checks = 0;
    auto node = [&](int m, int n, int l) {
        const int64_t loff = MN * l, h = m + (int64_t)M * n + loff;
        const uint32_t h32 = edge_elem32(m, n, M, (uint32_t)loff);
        bad += (int64_t)h32 != h;
        for (int plane = 0; plane < EDGE_ADDR_PLANES; ++plane, ++checks) {
            const int64_t want = h + MNL * plane;
            const uint32_t got = edge_plane_elem32(h32, (uint32_t)plane, (uint32_t)MNL);
            bad += (int64_t)got != want;
            bad += (uint64_t)want * 8 != (uint64_t)(uint32_t)(got * 8u);  // the byte offset of a double, in 32 bits
        }
    };
    for (int l = 0; l < L; ++l) {
        if (all) {
            for (int n = 0; n < N; ++n)
                for (int m = 0; m < M; ++m) node(m, n, l);
        } else {
            for (int n : {0, 1, N / 2, N - 2, N - 1})
                for (int m : {0, 1, M / 2, M - 2, M - 1}) node(m, n, l);
            for (int64_t i = 0; i < MN; i += 4099) node((int)(i % M), (int)(i / M), l);
        }
    }
    printf("addr M=%d N=%d L=%d checks=%ld mismatches=%ld\n", M, N, L, checks, bad);
    return bad != 0;
}

void run_ok(int64_t M, int64_t N, int64_t L, int64_t bytes)
{
    printf("ok M=%lld N=%lld L=%lld bytes=%lld ok=%d\n", (long long)M, (long long)N, (long long)L, (long long)bytes,
           (int)edge_addr32_ok(M, N, L, bytes));
}

constexpr int MO = 24, NO = 20;

struct Frame {
    std::vector<vvo2_t> vo;   // the offset store, as gqmap_set_images lays it out
    std::vector<double> lut;  // the table the kernel fills
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
    const uint16_t zero = taplut_offset(0, vmin);
    F.vo.assign(ne, vvo2_t{zero, zero});
    for (size_t cc = 0; cc < N2; ++cc)
        for (size_t r = 0; r < M2; ++r) {
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
    Rng g{777u + (uint64_t)K};
    int bad = 0, sets = 0, free_sets = 0;
    long clamped = 0;
    for (int f = 0; f < 6; ++f) {
        const Frame F = frame(g);
        const auto lv = frame_view_lut(F.vo.data(), MO + 2, F.lut.data());
        const auto bv = frame_view_lut_biased(F.vo.data(), MO + 2, F.lut.data());
        for (int s = 0; s < 40; ++s, ++sets) {
            const bool small = s % 4 == 0;  // a quarter of the sets: small sigma at an inner node (clamp-free)
            // (the others: every eighth at a corner node, whose samples clamp to both ends of an axis)
            const bool corner = !small && s % 8 == 1;
            const int m = small ? 8 + g.below(MO - 16) : corner ? (g.below(2) ? MO - 1 : 0) : g.below(MO);
            const int n = small ? 8 + g.below(NO - 16) : corner ? (g.below(2) ? NO - 1 : 0) : g.below(NO);
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
            const Sums<double> r1 = node_sums<0, true, true, 0>(tp, 0, K2, 1, lv, F.I1.data(), MO, NO, eps, c, u1, u2, m, n);
            const Sums<double> r4 = node_sums<0, true, true, NODE_UNROLL(4)>(tp, 0, K2, 1, lv, F.I1.data(), MO, NO, eps, c,
                                                                             u1, u2, m, n);
            const Sums<double> g1 = node_sums<0, true, true, 0>(tp, 0, K2, 1, bv, F.I1.data(), MO, NO, eps, c, u1, u2, m, n);
            const Sums<double> g4 = node_sums<0, true, true, NODE_UNROLL(4)>(tp, 0, K2, 1, bv, F.I1.data(), MO, NO, eps, c,
                                                                             u1, u2, m, n);
            bad += !same_bits(r1, g1) + !same_bits(r4, g4) + !same_bits(r1, r4) + !(r1.s0 > 0);
            if (node_unclamped(c, u1, u2, m, n, MO, NO, xmax)) {
                ++free_sets;
                const Sums<double> f1 = node_sums<0, false, true, 0>(tp, 0, K2, 1, bv, F.I1.data(), MO, NO, eps, c, u1, u2, m, n);
                const Sums<double> f4 = node_sums<0, false, true, NODE_UNROLL(4)>(tp, 0, K2, 1, bv, F.I1.data(), MO, NO, eps,
                                                                                 c, u1, u2, m, n);
                const Sums<double> rf = node_sums<0, false, true, NODE_UNROLL(4)>(tp, 0, K2, 1, lv, F.I1.data(), MO, NO, eps,
                                                                                 c, u1, u2, m, n);
                bad += !same_bits(rf, f1) + !same_bits(rf, f4) + !same_bits(rf, r1);
            }
        }
    }
    printf("node K=%d sets=%d clamped_samples=%ld free_sets=%d mismatches=%d\n", K, sets, clamped, free_sets, bad);
    return bad;
}

}  // namespace

int main()
{
    int bad = run_bias(40, 56) + run_bias(388, 584);
    // C2's node grid (a node per pixel), every node; the largest grid the
    // 32-bit form takes (M N = 2^24 - 1 = 4095 x 4097), every node; L > 1
    bad += run_addr(388, 584, 1, true);
    bad += run_addr(4095, 4097, 1, true);
    bad += run_addr(1023, 1025, 3, false);
    run_ok(388, 584, 1, 8);
    run_ok(4095, 4097, 1, 8);   // M N L = 2^24 - 1
    run_ok(4096, 4096, 1, 8);   // 2^24: just above
    run_ok(4095, 4098, 1, 8);
    run_ok(1023, 1025, 4, 8);   // M N L L = 2^24 - 16
    run_ok(1024, 1024, 4, 8);   // M N L L = 2^24
    run_ok(16777215, 1, 1, 8);
    run_ok(16777216, 1, 1, 8);  // M itself past 24 bits
    for (int K : {2, 9, 16}) bad += run_K(K);
    return bad ? 1 : 0;
}
