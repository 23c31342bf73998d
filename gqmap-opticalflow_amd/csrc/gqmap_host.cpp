// gqmap_host.cpp -- host-side helpers of libgqmap.so (no device code).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>

#include "gqmap_blockmatch.h"
#include "gqmap_denoise.h"
#include "gqmap_flowcheck.h"
#include "gqmap_internal.h"
#include "gqmap_rof.h"
#include "gqmap_wmedian.h"

namespace gq {

static thread_local std::string g_err;

void set_error(const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
}

void clear_error() { g_err.clear(); }

// getVV (gqmap_gpu_mixture.m:191-208): copy I2 into the interior of an
// (M+2)x(N+2) array, then extrapolate the first/last row of every column and
// afterwards the first/last column of every row with 3*f1 - 3*f2 + f3 -- the
// boundary rule of MATLAB interp2(...,'cubic').  Column-major throughout.
void build_padded(const double *I2, int M, int N, double *VV)
{
    const int M2 = M + 2, N2 = N + 2;
    std::fill(VV, VV + (size_t)M2 * N2, 0.0);
    for (int n = 0; n < N; ++n)
        std::memcpy(VV + (size_t)M2 * (n + 1) + 1, I2 + (size_t)M * n, sizeof(double) * M);
    for (int col = 0; col < N2; ++col) {
        double *c = VV + (size_t)M2 * col;
        c[0] = (3.0 * c[1] - 3.0 * c[2]) + c[3];
        c[M2 - 1] = (3.0 * c[M2 - 2] - 3.0 * c[M2 - 3]) + c[M2 - 4];
    }
    double *first = VV, *last = VV + (size_t)M2 * (N2 - 1);
    for (int r = 0; r < M2; ++r) {
        first[r] = (3.0 * first[r + M2] - 3.0 * first[r + 2 * M2]) + first[r + 3 * M2];
        last[r] = (3.0 * last[r - M2] - 3.0 * last[r - 2 * M2]) + last[r - 3 * M2];
    }
}

// imresize 'bicubic' kernel (Keys, a = -0.5) in its unscaled form
static double keys_cubic(double x)
{
    const double ax = std::fabs(x), ax2 = ax * ax, ax3 = ax2 * ax;
    return ax <= 1.0 ? 1.5 * ax3 - 2.5 * ax2 + 1.0
         : ax <= 2.0 ? -0.5 * ax3 + 2.5 * ax2 - 4.0 * ax + 2.0
                     : 0.0;
}

int resize_len(int len, double scale) { return (int)std::ceil(scale * (double)len); }

// MATLAB imresize contributions(): output sample x (1-based) sits at
// u = x/scale + (1 - 1/scale)/2 in input coordinates; taps left..left+P-1
// with left = floor(u - width/2); a reduction widens the kernel to 4/scale
// and scales it by `scale` (antialiasing); rows are normalised to sum 1;
// out-of-range taps mirror symmetrically; tap columns that are zero for
// every output are dropped (so scale 1 is an exact copy).
int resize_contrib(int in_len, int out_len, double scale, int antialias, std::vector<double> &w,
                   std::vector<int> &idx)
{
    const bool aa = antialias && scale < 1.0;
    const double width = aa ? 4.0 / scale : 4.0;
    const int P = (int)std::ceil(width) + 2;
    std::vector<double> wf((size_t)out_len * P);
    std::vector<int> jf((size_t)out_len * P);
    const long period = 2L * in_len;
    for (int i = 0; i < out_len; ++i) {
        const double u = (double)(i + 1) / scale + 0.5 * (1.0 - 1.0 / scale);
        const double left = std::floor(u - width / 2.0);
        double *wr = &wf[(size_t)i * P];
        double sum = 0.0;
        for (int k = 0; k < P; ++k) {
            const double d = u - (left + (double)k);
            wr[k] = aa ? scale * keys_cubic(scale * d) : keys_cubic(d);
            sum += wr[k];
        }
        for (int k = 0; k < P; ++k) {
            wr[k] /= sum;
            long j = ((long)left + k - 1) % period;
            if (j < 0) j += period;
            jf[(size_t)i * P + k] = (int)(j < in_len ? j : period - 1 - j);
        }
    }
    std::vector<int> keep;
    for (int k = 0; k < P; ++k)
        for (int i = 0; i < out_len; ++i)
            if (wf[(size_t)i * P + k] != 0.0) { keep.push_back(k); break; }
    const int Pk = (int)keep.size();
    w.assign((size_t)out_len * Pk, 0.0);
    idx.assign((size_t)out_len * Pk, 0);
    for (int i = 0; i < out_len; ++i)
        for (int k = 0; k < Pk; ++k) {
            w[(size_t)i * Pk + k] = wf[(size_t)i * P + keep[k]];
            idx[(size_t)i * Pk + k] = jf[(size_t)i * P + keep[k]];
        }
    return Pk;
}

// Gauss-Hermite nodes/weights for int exp(-x^2) f(x): Newton iteration on the
// orthonormal Hermite recurrence with asymptotic starting guesses.  The
// reference (GaussHermite_2.m) takes the eigen-decomposition of the Jacobi
// matrix instead; both give the same rule (tests compare with numpy.hermgauss).
int gauss_hermite(int n, double *x, double *w)
{
    if (n < 1 || n > GQMAP_KMAX) return 1;
    const double pim4 = 0.7511255444649425;  // pi^(-1/4)
    const int half = (n + 1) / 2;
    double z = 0, pp = 1;
    double xd[GQMAP_KMAX], wd[GQMAP_KMAX];  // descending
    for (int i = 0; i < half; ++i) {
        if (i == 0) z = std::sqrt(2.0 * n + 1) - 1.85575 * std::pow(2.0 * n + 1, -1.0 / 6.0);
        else if (i == 1) z -= 1.14 * std::pow((double)n, 0.426) / z;
        else if (i == 2) z = 1.86 * z - 0.86 * xd[0];
        else if (i == 3) z = 1.91 * z - 0.91 * xd[1];
        else z = 2.0 * z - xd[i - 2];
        int iter = 0;
        for (; iter < 200; ++iter) {
            double p1 = pim4, p2 = 0.0;
            for (int j = 1; j <= n; ++j) {
                const double p3 = p2;
                p2 = p1;
                p1 = z * std::sqrt(2.0 / j) * p2 - std::sqrt((j - 1.0) / j) * p3;
            }
            pp = std::sqrt(2.0 * n) * p2;
            const double z1 = z;
            z = z1 - p1 / pp;
            if (std::fabs(z - z1) <= 1e-15 * std::max(1.0, std::fabs(z))) break;
        }
        if (iter == 200) return 2;
        xd[i] = z;
        xd[n - 1 - i] = -z;
        wd[i] = wd[n - 1 - i] = 2.0 / (pp * pp);
    }
    if (n % 2 == 1) xd[half - 1] = 0.0;  // exact symmetric middle node
    for (int i = 0; i < n; ++i) {
        x[i] = xd[n - 1 - i];
        w[i] = wd[n - 1 - i];
    }
    return 0;
}

}  // namespace gq

extern "C" {

const char *gqmap_last_error(void) { return gq::g_err.c_str(); }

gqmap_status gqmap_gauss_hermite(int K, double *x, double *w)
{
    gq::clear_error();
    GQ_CHECK(x && w, GQMAP_ERR_INVALID_ARG, "null argument");
    GQ_CHECK(K >= 1 && K <= GQMAP_KMAX, GQMAP_ERR_INVALID_ARG, "K=%d outside [1,%d]", K, GQMAP_KMAX);
    GQ_CHECK(gq::gauss_hermite(K, x, w) == 0, GQMAP_ERR_INVALID_ARG, "Gauss-Hermite did not converge");
    return GQMAP_OK;
}

void gqmap_rand_uniform(uint64_t seed, uint32_t stream, uint64_t first, size_t n, double *out)
{
    const uint64_t base = gq::stream_base(seed, stream);
    for (size_t i = 0; i < n; ++i) out[i] = gq::u01(base, first + i);
}

int gqmap_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Middlebury .flo I/O and AEPE, host-side library calls
// ---------------------------------------------------------------------------
extern "C" {

// readFlowFile.m:33-84: "PIEH" tag (float 202021.25), int32 width, int32
// height, then rows of interleaved (u, v) float32; flow is M x N x 2 doubles
// (column-major).  flow == NULL: only the size is returned.
gqmap_status gqmap_read_flo(const char *path, int *M, int *N, double *flow)
{
    gq::clear_error();
    GQ_CHECK(path && M && N, GQMAP_ERR_INVALID_ARG, "gqmap_read_flo: null argument");
    const size_t len = std::strlen(path);
    GQ_CHECK(len > 4 && std::strcmp(path + len - 4, ".flo") == 0, GQMAP_ERR_INVALID_ARG,
             "readFlowFile: filename %s should have extension '.flo'", path);
    FILE *f = std::fopen(path, "rb");
    GQ_CHECK(f, GQMAP_ERR_INVALID_ARG, "readFlowFile: could not open %s", path);
    float tag = 0;
    int32_t wh[2] = {0, 0};
    const bool hdr = std::fread(&tag, 4, 1, f) == 1 && std::fread(wh, 4, 2, f) == 2;
    if (!hdr || tag != 202021.25f || wh[0] < 1 || wh[0] > 99999 || wh[1] < 1 || wh[1] > 99999) {
        std::fclose(f);
        gq::set_error("readFlowFile(%s): wrong tag or illegal size", path);
        return GQMAP_ERR_INVALID_ARG;
    }
    const int W = wh[0], H = wh[1];
    *M = H;
    *N = W;
    if (!flow) {
        std::fclose(f);
        return GQMAP_OK;
    }
    std::vector<float> row((size_t)2 * W);
    for (int m = 0; m < H; ++m) {
        if (std::fread(row.data(), sizeof(float), row.size(), f) != row.size()) {
            std::fclose(f);
            gq::set_error("readFlowFile(%s): truncated data", path);
            return GQMAP_ERR_INVALID_ARG;
        }
        for (int n = 0; n < W; ++n) {
            flow[m + (size_t)H * n] = row[2 * (size_t)n];
            flow[m + (size_t)H * n + (size_t)H * W] = row[2 * (size_t)n + 1];
        }
    }
    std::fclose(f);
    return GQMAP_OK;
}

// legacy/writeFlowFile.m:33-76
gqmap_status gqmap_write_flo(const char *path, const double *flow, int M, int N)
{
    gq::clear_error();
    GQ_CHECK(path && flow && M > 0 && N > 0, GQMAP_ERR_INVALID_ARG, "gqmap_write_flo: bad argument");
    const size_t len = std::strlen(path);
    GQ_CHECK(len > 4 && std::strcmp(path + len - 4, ".flo") == 0, GQMAP_ERR_INVALID_ARG,
             "writeFlowFile: filename %s should have extension '.flo'", path);
    FILE *f = std::fopen(path, "wb");
    GQ_CHECK(f, GQMAP_ERR_INVALID_ARG, "writeFlowFile: could not open %s", path);
    const int32_t wh[2] = {N, M};
    bool ok = std::fwrite("PIEH", 1, 4, f) == 4 && std::fwrite(wh, 4, 2, f) == 2;
    std::vector<float> row((size_t)2 * N);
    for (int m = 0; m < M && ok; ++m) {
        for (int n = 0; n < N; ++n) {
            row[2 * (size_t)n] = (float)flow[m + (size_t)M * n];
            row[2 * (size_t)n + 1] = (float)flow[m + (size_t)M * n + (size_t)M * N];
        }
        ok = std::fwrite(row.data(), sizeof(float), row.size(), f) == row.size();
    }
    ok = (std::fclose(f) == 0) && ok;
    GQ_CHECK(ok, GQMAP_ERR_INVALID_ARG, "writeFlowFile: write to %s failed", path);
    return GQMAP_OK;
}

// gqmap_gpu_mixture.m:63-64: flow(unknown) = 0, then
// mean(mean(sqrt(sum((tflow - flow).^2, 3)))) over rows/cols crop..end-crop
// (column means first).  unknown may be NULL.
gqmap_status gqmap_aepe(const double *tflow, const double *flow, const uint8_t *unknown, int M, int N, int crop,
                        double *out)
{
    gq::clear_error();
    GQ_CHECK(tflow && flow && out, GQMAP_ERR_INVALID_ARG, "gqmap_aepe: null argument");
    GQ_CHECK(crop >= 0 && M > 2 * crop && N > 2 * crop, GQMAP_ERR_INVALID_ARG, "gqmap_aepe: crop %d of %dx%d",
             crop, M, N);
    const size_t MN = (size_t)M * N;
    double total = 0;
    for (int n = crop; n < N - crop; ++n) {
        double col = 0;
        for (int m = crop; m < M - crop; ++m) {
            const size_t q = m + (size_t)M * n;
            const bool unk = unknown && unknown[q];
            const double du = tflow[q] - (unk ? 0.0 : flow[q]);
            const double dv = tflow[q + MN] - (unk ? 0.0 : flow[q + MN]);
            col += std::sqrt(du * du + dv * dv);
        }
        total += col / (M - 2 * crop);
    }
    *out = total / (N - 2 * crop);
    return GQMAP_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Block-matching initialiser, host model (legacy/optical_flow_temp.m:13-32):
// the arithmetic of gqmap_blockmatch.h over zero-padded copies of the frames,
// one displacement at a time.  Bit for bit what gqmap_block_match computes.
// ---------------------------------------------------------------------------
// H = 0: the single-hypothesis result (flow M x N x 2); H >= 1: H ranks by the
// greedy rule of gqmap_blockmatch.h, one pass over the displacements per rank,
// as the kernel does.  refine (H >= 1): the sub-pixel flow and the curvature
// (curv may be null) by H + 1 passes, pass r >= 1 also keeping the neighbour
// costs of rank r - 1's pick, again as the kernel does.  who names the caller
// in errors.
static gqmap_status bm_host(const char *who, const double *A, const double *B, int M, int N, int U, int V, int ft,
                            double sigma, int H, int sep, bool refine, double *flow, double *cost, double *curv)
{
    gq::clear_error();
    GQ_CHECK(A && B && flow, GQMAP_ERR_INVALID_ARG, "%s: null argument", who);
    const char *bad = gq::bm_bad_args(M, N, U, V, ft, sigma);
    GQ_CHECK(!bad, GQMAP_ERR_INVALID_ARG, "%s: %s (M=%d N=%d U=%d V=%d ft=%d sigma=%g)", who, bad, M, N, U, V, ft,
             sigma);
    const gq::BmFilter f = gq::bm_filter(ft, sigma);
    // Ap(r, c) = A(r - ft, c - ft), Bp(r, c) = B(r - ft - U, c - ft - V), zero outside
    const size_t AH = (size_t)M + 2 * ft, AW = (size_t)N + 2 * ft, BH = AH + 2 * U, BW = AW + 2 * V;
    const size_t MN = (size_t)M * N;
    const int ranks = H == 0 ? 1 : H;
    std::vector<double> Ap(AH * AW, 0.0), Bp(BH * BW, 0.0), T((size_t)M * AW), best(MN);
    std::vector<int> bidx(MN), pick(MN * GQ_BM_HMAX), last(refine ? MN : 0, -1);
    std::vector<gq::BmNear> nbr(refine ? MN : 0);
    std::vector<double> c0(refine ? MN : 0);
    for (int n = 0; n < N; ++n) {
        std::memcpy(&Ap[ft + AH * (n + ft)], A + (size_t)M * n, sizeof(double) * M);
        std::memcpy(&Bp[ft + U + BH * (n + ft + V)], B + (size_t)M * n, sizeof(double) * M);
    }
    const int nu = 2 * U + 1;
    for (int r = 0; r < ranks + (refine ? 1 : 0); ++r) {
        std::fill(best.begin(), best.end(), INFINITY);
        std::fill(bidx.begin(), bidx.end(), -1);
        for (gq::BmNear &q : nbr) gq::bm_near_clear(q);
        for (int v = 0; v <= 2 * V; ++v)
            for (int u = 0; u <= 2 * U; ++u) {
                for (size_t c = 0; c < AW; ++c) {
                    const bool col_in = c >= (size_t)ft && c < (size_t)ft + N;
                    for (int m = 0; m < M; ++m)
                        T[m + (size_t)M * c] =
                            gq::bm_rows(&Ap[m + AH * c], &Bp[m + u + BH * (c + v)], ft, f, m - ft, M, col_in);
                }
                for (int n = 0; n < N; ++n)
                    for (int m = 0; m < M; ++m) {
                        const size_t o = m + (size_t)M * n;
                        const double c = gq::bm_cols(&T[o], M, ft, f);
                        if (r < ranks) {
                            bool allowed = true;
                            for (int j = 0; j < r; ++j) allowed = allowed && gq::bm_far(u, v, pick[o + MN * j], sep);
                            gq::bm_keep_allowed(allowed, c, u + v * nu, best[o], bidx[o]);
                        }
                        if (refine && r >= 1) gq::bm_capture(u, v, last[o], c, nbr[o]);
                    }
            }
        for (size_t o = 0; o < MN; ++o) {
            const bool found = bidx[o] >= 0;
            if (refine) {
                if (r >= 1) {  // rank r - 1, its neighbour costs now known
                    double out[4];
                    gq::bm_refined(last[o], c0[o], nbr[o], U, V, out);
                    flow[o + 2 * MN * (r - 1)] = out[0];
                    flow[o + 2 * MN * (r - 1) + MN] = out[1];
                    if (cost) cost[o + MN * (r - 1)] = c0[o];
                    if (curv) {
                        curv[o + 2 * MN * (r - 1)] = out[2];
                        curv[o + 2 * MN * (r - 1) + MN] = out[3];
                    }
                }
            } else {  // rank r
                flow[o + 2 * MN * r] = found ? (double)(V - bidx[o] / nu) : gq::bm_nan();       // vmt
                flow[o + 2 * MN * r + MN] = found ? (double)(U - bidx[o] % nu) : gq::bm_nan();  // umt
                if (cost) cost[o + MN * r] = best[o];
            }
            // this scan's pick, for the scans after it
            const int p = found ? gq::bm_pack(bidx[o] % nu, bidx[o] / nu) : -1;
            if (refine) {
                last[o] = p;
                c0[o] = best[o];
            }
            // a missing rank adds no exclusion: the allowed set stays empty for the later ranks
            if (r < ranks) pick[o + MN * r] = found ? p : pick[o + MN * (r > 0 ? r - 1 : 0)];
        }
    }
    return GQMAP_OK;
}

extern "C" {

gqmap_status gqmap_block_match_host(const double *A, const double *B, int M, int N, int U, int V, int ft,
                                    double sigma, double *flow, double *cost)
{
    return bm_host("gqmap_block_match_host", A, B, M, N, U, V, ft, sigma, 0, 1, false, flow, cost, nullptr);
}

gqmap_status gqmap_block_match_multi_host(const double *A, const double *B, int M, int N, int U, int V, int ft,
                                          double sigma, int H, int sep, double *flow, double *cost)
{
    gq::clear_error();
    const char *bad = gq::bm_bad_multi(H, sep);
    GQ_CHECK(!bad, GQMAP_ERR_INVALID_ARG, "gqmap_block_match_multi_host: %s (H=%d sep=%d)", bad, H, sep);
    return bm_host("gqmap_block_match_multi_host", A, B, M, N, U, V, ft, sigma, H, sep, false, flow, cost, nullptr);
}

gqmap_status gqmap_block_match_refine_host(const double *A, const double *B, int M, int N, int U, int V, int ft,
                                           double sigma, int H, int sep, double *flow, double *cost, double *curv)
{
    gq::clear_error();
    const char *bad = gq::bm_bad_multi(H, sep);
    GQ_CHECK(!bad, GQMAP_ERR_INVALID_ARG, "gqmap_block_match_refine_host: %s (H=%d sep=%d)", bad, H, sep);
    return bm_host("gqmap_block_match_refine_host", A, B, M, N, U, V, ft, sigma, H, sep, true, flow, cost, curv);
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Per-pixel windows and the coarse-to-fine scheme, plain and ranked, host
// models ("Per-pixel windows", "Coarse to fine", "Ranked windows" and "Ranked
// coarse to fine" of gqmap_blockmatch.h).  Tile by tile, as the kernel: a
// displacement is evaluated over a 32 x 32 tile when one of the tile's pixels
// has it in its box, so the work follows the windows and not their union over
// the frame.  The pick rule knows no scan order, so the tiling shows in no
// result.  The plain entry points are the ranked ones at H = 1: no earlier
// rank excludes anything and every rank offset is zero.
// ---------------------------------------------------------------------------
namespace {

// one level of "Ranked windows": win (M x N x 4 x H) or, when null, the box cbox at every pixel and rank.  flow, curv
// (M x N x 2 x H), cost (M x N x H) and pick (per rank the planes du, dv; GQ_BM_NOPICK without a pick) may each be
// null.  The rank loop is inside the tile: the A tile is staged once, only the keys survive a rank.
void bm_ranked_level(const double *A, const double *B, int M, int N, const int *win, const int cbox[4], int ft,
                     const gq::BmFilter &f, int H, int sep, bool subpixel, double *flow, double *cost, double *curv,
                     int *pick)
{
    constexpr int TM = 32, TN = 32;
    const int AH = TM + 2 * ft, AW = TN + 2 * ft;
    const size_t MN = (size_t)M * N;
    std::vector<double> As((size_t)AH * AW), bcol(AH), T((size_t)TM * AW), best(TM * TN);
    std::vector<int> box(4 * TM * TN), key(TM * TN), prev(GQ_BM_HMAX * TM * TN);
    std::vector<gq::BmNear> nbr(TM * TN);
    for (int n0 = 0; n0 < N; n0 += TN)
        for (int m0 = 0; m0 < M; m0 += TM) {
            const int th = std::min(TM, M - m0), tw = std::min(TN, N - n0);
            for (int c = 0; c < AW; ++c)
                for (int i = 0; i < AH; ++i) {
                    const int gm = m0 - ft + i, gn = n0 - ft + c;
                    As[i + (size_t)AH * c] = gm >= 0 && gm < M && gn >= 0 && gn < N ? A[gm + (size_t)M * gn] : 0.0;
                }
            for (int rank = 0; rank < H; ++rank) {
                // (du, dv) is allowed at pixel o: far from the pick of every earlier rank that has one
                const auto allowed = [&](int o, int du, int dv) {
                    for (int i = 0; i < rank; ++i)
                        if (!gq::bm_far_key(du, dv, prev[i + GQ_BM_HMAX * o], sep)) return false;
                    return true;
                };
                int un[4] = {GQ_BM_NOPICK, -GQ_BM_NOPICK, GQ_BM_NOPICK, -GQ_BM_NOPICK};
                for (int j = 0; j < tw; ++j)
                    for (int i = 0; i < th; ++i) {
                        int *b = &box[4 * (i + TM * j)];
                        for (int q = 0; q < 4; ++q)
                            b[q] = win ? win[(m0 + i) + (size_t)M * (n0 + j) + MN * q + 4 * MN * rank] : cbox[q];
                        best[i + TM * j] = INFINITY;
                        key[i + TM * j] = GQ_BM_NOPICK;
                        gq::bm_near_clear(nbr[i + TM * j]);
                        if (b[0] > b[1] || b[2] > b[3]) continue;
                        un[0] = std::min(un[0], b[0]);
                        un[1] = std::max(un[1], b[1]);
                        un[2] = std::min(un[2], b[2]);
                        un[3] = std::max(un[3], b[3]);
                    }
                for (int pass = 0; pass < (subpixel ? 2 : 1); ++pass)
                    for (int dv = un[2]; dv <= un[3]; ++dv)
                        for (int du = un[0]; du <= un[1]; ++du) {
                            bool any = false;
                            for (int j = 0; j < tw && !any; ++j)
                                for (int i = 0; i < th && !any; ++i) {
                                    const int o = i + TM * j;
                                    any = pass == 0 ? gq::bm_in_box(&box[4 * o], du, dv) && allowed(o, du, dv)
                                                    : gq::bm_near_wanted(&box[4 * o], du, dv, key[o]);
                                }
                            if (!any) continue;
                            for (int c = 0; c < tw + 2 * ft; ++c) {
                                const int gn = n0 - ft + c;
                                for (int i = 0; i < AH; ++i) {
                                    const int bm = m0 - ft + i + du, bn = gn + dv;
                                    bcol[i] = bm >= 0 && bm < M && bn >= 0 && bn < N ? B[bm + (size_t)M * bn] : 0.0;
                                }
                                for (int i = 0; i < th; ++i)
                                    T[i + (size_t)TM * c] = gq::bm_rows(&As[i + (size_t)AH * c], &bcol[i], ft, f,
                                                                        m0 + i - ft, M, gn >= 0 && gn < N);
                            }
                            for (int j = 0; j < tw; ++j)
                                for (int i = 0; i < th; ++i) {
                                    const int o = i + TM * j;
                                    const double c = gq::bm_cols(&T[i + (size_t)TM * j], TM, ft, f);
                                    if (pass == 0)
                                        gq::bm_keep_window(gq::bm_in_box(&box[4 * o], du, dv) && allowed(o, du, dv), c,
                                                           du, dv, best[o], key[o]);
                                    else
                                        gq::bm_capture_window(du, dv, key[o], c, nbr[o]);
                                }
                        }
                for (int j = 0; j < tw; ++j)
                    for (int i = 0; i < th; ++i) {
                        const int o = i + TM * j;
                        const size_t g = (m0 + i) + (size_t)M * (n0 + j);
                        double out[4];
                        gq::bm_refined_window(key[o], best[o], nbr[o], &box[4 * o], subpixel, out);
                        if (flow) {
                            flow[g + 2 * MN * rank] = out[0];
                            flow[g + 2 * MN * rank + MN] = out[1];
                        }
                        if (cost) cost[g + MN * rank] = best[o];
                        if (curv) {
                            curv[g + 2 * MN * rank] = out[2];
                            curv[g + 2 * MN * rank + MN] = out[3];
                        }
                        if (pick) {
                            const bool found = key[o] != GQ_BM_NOPICK;
                            pick[g + 2 * MN * rank] = found ? gq::bm_key_du(key[o]) : GQ_BM_NOPICK;
                            pick[g + 2 * MN * rank + MN] = found ? gq::bm_key_dv(key[o]) : GQ_BM_NOPICK;
                        }
                        prev[rank + GQ_BM_HMAX * o] = key[o];
                    }
            }
        }
}

// "Coarse to fine" and "Ranked coarse to fine": the frames halved up to level levels - 1, the boxes of a level from
// the H pick-plane pairs of the level above, level 0's outputs returned
void bm_pyramid_levels(const double *A, const double *B, int M, int N, int U, int V, int ft, double sigma, int levels,
                       int r, int k, int H, int sep, bool subpixel, double *flow, double *cost, double *curv)
{
    const gq::BmFilter f = gq::bm_filter(ft, sigma);
    const int c = levels - 1;
    std::vector<std::vector<double>> As(levels), Bs(levels);
    std::vector<int> Ms(levels, M), Ns(levels, N);
    for (int l = 1; l < levels; ++l) {
        const int Mp = Ms[l - 1], Np = Ns[l - 1];
        Ms[l] = (Mp + 1) / 2, Ns[l] = (Np + 1) / 2;
        As[l].resize((size_t)Ms[l] * Ns[l]);
        Bs[l].resize((size_t)Ms[l] * Ns[l]);
        for (int j = 0; j < Ns[l]; ++j)
            for (int i = 0; i < Ms[l]; ++i) {
                As[l][i + (size_t)Ms[l] * j] = gq::bm_half(l == 1 ? A : As[l - 1].data(), Mp, Np, i, j);
                Bs[l][i + (size_t)Ms[l] * j] = gq::bm_half(l == 1 ? B : Bs[l - 1].data(), Mp, Np, i, j);
            }
    }
    const int Uc = gq::bm_ceil_shift(U, c), Vc = gq::bm_ceil_shift(V, c);
    const int cbox[4] = {-Uc, Uc, -Vc, Vc};
    std::vector<int> pick, win;  // H pick-plane pairs of the level above, H boxes of this one
    for (int l = c; l >= 0; --l) {
        const double *a = l == 0 ? A : As[l].data(), *b = l == 0 ? B : Bs[l].data();
        const size_t mn = (size_t)Ms[l] * Ns[l];
        if (l < c) {
            const size_t mnc = (size_t)Ms[l + 1] * Ns[l + 1];
            win.resize(4 * mn * H);
            for (int j = 0; j < H; ++j)
                for (int n = 0; n < Ns[l]; ++n)
                    for (int m = 0; m < Ms[l]; ++m) {
                        int box[4];
                        gq::bm_window_up(pick.data() + 2 * mnc * j, Ms[l + 1], Ns[l + 1], m, n, r, k, box);
                        for (int q = 0; q < 4; ++q) win[m + (size_t)Ms[l] * n + mn * q + 4 * mn * j] = box[q];
                    }
        }
        std::vector<int> next(l > 0 ? 2 * mn * H : 0);
        bm_ranked_level(a, b, Ms[l], Ns[l], l < c ? win.data() : nullptr, cbox, ft, f, H, sep, l == 0 && subpixel,
                        l == 0 ? flow : nullptr, l == 0 ? cost : nullptr, l == 0 ? curv : nullptr,
                        l > 0 ? next.data() : nullptr);
        pick.swap(next);
    }
}

}  // namespace

extern "C" {

gqmap_status gqmap_block_match_window_multi_host(const double *A, const double *B, const int *win, int M, int N,
                                                 int ft, double sigma, int H, int sep, int subpixel, double *flow,
                                                 double *cost, double *curv)
{
    gq::clear_error();
    GQ_CHECK(A && B && win && flow, GQMAP_ERR_INVALID_ARG, "gqmap_block_match_window_multi_host: null argument");
    const char *bad = gq::bm_bad_window(M, N, ft, sigma);
    GQ_CHECK(!bad, GQMAP_ERR_INVALID_ARG, "gqmap_block_match_window_multi_host: %s (M=%d N=%d ft=%d sigma=%g)", bad, M,
             N, ft, sigma);
    bad = gq::bm_bad_multi(H, sep);
    GQ_CHECK(!bad, GQMAP_ERR_INVALID_ARG, "gqmap_block_match_window_multi_host: %s (H=%d sep=%d)", bad, H, sep);
    for (int j = 0; j < H; ++j)
        GQ_CHECK(!gq::bm_bad_bounds(win + 4 * (size_t)M * N * j, M, N), GQMAP_ERR_INVALID_ARG,
                 "gqmap_block_match_window_multi_host: a window bound of rank %d outside [-%d,%d]", j, GQ_BM_DMAX,
                 GQ_BM_DMAX);
    bm_ranked_level(A, B, M, N, win, nullptr, ft, gq::bm_filter(ft, sigma), H, sep, subpixel != 0, flow, cost, curv,
                    nullptr);
    return GQMAP_OK;
}

gqmap_status gqmap_block_match_pyramid_multi_host(const double *A, const double *B, int M, int N, int U, int V, int ft,
                                                  double sigma, int levels, int r, int k, int H, int sep, int subpixel,
                                                  double *flow, double *cost, double *curv)
{
    gq::clear_error();
    GQ_CHECK(A && B && flow, GQMAP_ERR_INVALID_ARG, "gqmap_block_match_pyramid_multi_host: null argument");
    const char *bad = gq::bm_bad_pyramid(M, N, U, V, ft, sigma, levels, r, k);
    GQ_CHECK(!bad, GQMAP_ERR_INVALID_ARG,
             "gqmap_block_match_pyramid_multi_host: %s (M=%d N=%d U=%d V=%d ft=%d sigma=%g levels=%d r=%d k=%d)", bad, M,
             N, U, V, ft, sigma, levels, r, k);
    bad = gq::bm_bad_multi(H, sep);
    GQ_CHECK(!bad, GQMAP_ERR_INVALID_ARG, "gqmap_block_match_pyramid_multi_host: %s (H=%d sep=%d)", bad, H, sep);
    bm_pyramid_levels(A, B, M, N, U, V, ft, sigma, levels, r, k, H, sep, subpixel != 0, flow, cost, curv);
    return GQMAP_OK;
}

int gqmap_block_match_reach(int U, int levels, int r)
{
    if (U < 0 || levels < 1 || levels > GQ_BM_LEVELS || r < 0) return -1;
    return gq::bm_reach(U, levels, r);
}

gqmap_status gqmap_block_match_window_host(const double *A, const double *B, const int *win, int M, int N, int ft,
                                           double sigma, int subpixel, double *flow, double *cost, double *curv)
{
    gq::clear_error();
    GQ_CHECK(A && B && win && flow, GQMAP_ERR_INVALID_ARG, "gqmap_block_match_window_host: null argument");
    const char *bad = gq::bm_bad_window(M, N, ft, sigma);
    GQ_CHECK(!bad, GQMAP_ERR_INVALID_ARG, "gqmap_block_match_window_host: %s (M=%d N=%d ft=%d sigma=%g)", bad, M, N, ft,
             sigma);
    GQ_CHECK(!gq::bm_bad_bounds(win, M, N), GQMAP_ERR_INVALID_ARG,
             "gqmap_block_match_window_host: a window bound outside [-%d,%d]", GQ_BM_DMAX, GQ_BM_DMAX);
    bm_ranked_level(A, B, M, N, win, nullptr, ft, gq::bm_filter(ft, sigma), 1, 0, subpixel != 0, flow, cost, curv,
                    nullptr);
    return GQMAP_OK;
}

gqmap_status gqmap_block_match_pyramid_host(const double *A, const double *B, int M, int N, int U, int V, int ft,
                                            double sigma, int levels, int r, int k, int subpixel, double *flow,
                                            double *cost, double *curv)
{
    gq::clear_error();
    GQ_CHECK(A && B && flow, GQMAP_ERR_INVALID_ARG, "gqmap_block_match_pyramid_host: null argument");
    const char *bad = gq::bm_bad_pyramid(M, N, U, V, ft, sigma, levels, r, k);
    GQ_CHECK(!bad, GQMAP_ERR_INVALID_ARG,
             "gqmap_block_match_pyramid_host: %s (M=%d N=%d U=%d V=%d ft=%d sigma=%g levels=%d r=%d k=%d)", bad, M, N, U,
             V, ft, sigma, levels, r, k);
    bm_pyramid_levels(A, B, M, N, U, V, ft, sigma, levels, r, k, 1, 0, subpixel != 0, flow, cost, curv);
    return GQMAP_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Structure-texture preprocessing, host model (optical_flowSuper.m:7-14 with
// preprocessed = true): the arithmetic of gqmap_rof.h, one plain Jacobi sweep
// per iteration over ping-pong copies of p.  Bit for bit what
// gqmap_structure_texture computes.
// ---------------------------------------------------------------------------
extern "C" {

gqmap_status gqmap_structure_texture_host(const double *im, int M, int N, int C, double theta, int n_iter,
                                          double alp, double *texture, double *structure)
{
    gq::clear_error();
    GQ_CHECK(im && texture, GQMAP_ERR_INVALID_ARG, "gqmap_structure_texture_host: null argument");
    const char *bad = gq::rof_bad_args(M, N, C, theta, n_iter, alp);
    GQ_CHECK(!bad, GQMAP_ERR_INVALID_ARG, "gqmap_structure_texture_host: %s (M=%d N=%d C=%d theta=%g n_iter=%d alp=%g)",
             bad, M, N, C, theta, n_iter, alp);
    const size_t MN = (size_t)M * N, n_all = MN * C;
    double lo = INFINITY, hi = -INFINITY;
    bool nonfinite = false;
    for (size_t i = 0; i < n_all; ++i) {
        nonfinite = nonfinite || !std::isfinite(im[i]);
        lo = std::fmin(lo, im[i]);
        hi = std::fmax(hi, im[i]);
    }
    GQ_CHECK(!gq::rof_bad_range(lo, hi, nonfinite), GQMAP_ERR_INVALID_ARG,
             "gqmap_structure_texture_host: input range [%g, %g] is zero or not finite", lo, hi);
    const double delta = gq::rof_delta(theta);
    std::vector<double> x(n_all), u(MN), p1(n_all, 0.0), p2(n_all, 0.0), t(n_all), s(n_all);
    for (size_t i = 0; i < n_all; ++i) x[i] = gq::rof_scale_in(im[i], lo, hi);
    // u (or s) of one plane from its p
    auto sweep_u = [&](const double *xc, const double *a1, const double *a2, double *out) {
        for (int n = 0; n < N; ++n)
            for (int m = 0; m < M; ++m) {
                const size_t o = m + (size_t)M * n;
                const double d = gq::rof_div(a1[o], n > 0 ? a1[o - M] : 0.0, a2[o], m > 0 ? a2[o - 1] : 0.0);
                out[o] = gq::rof_u(xc[o], theta, d);
            }
    };
    for (int c = 0; c < C; ++c) {
        const double *xc = &x[MN * c];
        double *a1 = &p1[MN * c], *a2 = &p2[MN * c];
        for (int it = 0; it < n_iter; ++it) {
            sweep_u(xc, a1, a2, u.data());
            // p of a pixel is read by u only, and u is complete: update in place
            for (int n = 0; n < N; ++n)
                for (int m = 0; m < M; ++m) {
                    const size_t o = m + (size_t)M * n;
                    const double ix = n < N - 1 ? u[o + M] - u[o] : 0.0;
                    const double iy = m < M - 1 ? u[o + 1] - u[o] : 0.0;
                    gq::rof_step(a1[o], a2[o], ix, iy, delta);
                }
        }
        sweep_u(xc, a1, a2, &s[MN * c]);
    }
    double tlo = INFINITY, thi = -INFINITY;
    nonfinite = false;
    for (size_t i = 0; i < n_all; ++i) {
        t[i] = gq::rof_t(x[i], alp, s[i]);
        nonfinite = nonfinite || !std::isfinite(t[i]);
        tlo = std::fmin(tlo, t[i]);
        thi = std::fmax(thi, t[i]);
    }
    GQ_CHECK(!gq::rof_bad_range(tlo, thi, nonfinite), GQMAP_ERR_INVALID_ARG,
             "gqmap_structure_texture_host: texture range [%g, %g] is zero or not finite", tlo, thi);
    for (size_t i = 0; i < n_all; ++i) texture[i] = gq::rof_scale_out(t[i], tlo, thi);
    if (structure) std::memcpy(structure, s.data(), sizeof(double) * n_all);
    return GQMAP_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Forward-backward check and fill, host models: the arithmetic of
// gqmap_flowcheck.h, pixel by pixel, the fill over zero-padded copies of V, S_0
// and S_1, one plain Jacobi pass at a time.  Bit for bit what
// gqmap_flow_consistency and gqmap_flow_fill compute.
// ---------------------------------------------------------------------------
extern "C" {

gqmap_status gqmap_flow_consistency_host(const double *fwd, const double *bwd, int M, int N, double a1, double a2,
                                         double *err, unsigned char *mask)
{
    gq::clear_error();
    GQ_CHECK(fwd && bwd && (err || mask), GQMAP_ERR_INVALID_ARG, "gqmap_flow_consistency_host: null argument");
    const char *bad = gq::fc_bad_check(M, N, a1, a2);
    GQ_CHECK(!bad, GQMAP_ERR_INVALID_ARG, "gqmap_flow_consistency_host: %s (M=%d N=%d a1=%g a2=%g)", bad, M, N, a1,
             a2);
    for (int n = 0; n < N; ++n)
        for (int m = 0; m < M; ++m) {
            double e;
            const bool ok = gq::fc_check(fwd, bwd, m, n, M, N, a1, a2, &e);
            const size_t o = m + (size_t)M * n;
            if (err) err[o] = e;
            if (mask) mask[o] = ok ? 1 : 0;
        }
    return GQMAP_OK;
}

gqmap_status gqmap_flow_fill_host(const double *flow, const unsigned char *mask, int M, int N, int r, double sigma,
                                  int passes, double *out, unsigned char *filled)
{
    gq::clear_error();
    GQ_CHECK(flow && mask && out, GQMAP_ERR_INVALID_ARG, "gqmap_flow_fill_host: null argument");
    const char *bad = gq::fc_bad_fill(M, N, r, sigma, passes);
    GQ_CHECK(!bad, GQMAP_ERR_INVALID_ARG, "gqmap_flow_fill_host: %s (M=%d N=%d r=%d sigma=%g passes=%d)", bad, M, N,
             r, sigma, passes);
    const gq::FcFilter f = gq::fc_filter(r, sigma);
    const size_t MN = (size_t)M * N, PH = (size_t)M + 2 * r, PW = (size_t)N + 2 * r;
    std::vector<unsigned char> state(MN), next(MN);
    std::vector<double> cur(flow, flow + 2 * MN), X(3 * PH * PW), T(3 * (size_t)M * PW), Y(3 * MN);
    for (size_t i = 0; i < MN; ++i) state[i] = mask[i] ? 0 : GQ_FC_UNFILLED;
    for (int p = 1; p <= passes; ++p) {
        // X_q(row, col) = X_q of pixel (row - r, col - r), zero outside the frame
        std::fill(X.begin(), X.end(), 0.0);
        for (int n = 0; n < N; ++n)
            for (int m = 0; m < M; ++m) {
                const size_t o = m + (size_t)M * n, c = m + r + PH * (n + r);
                const bool valid = state[o] != GQ_FC_UNFILLED;
                X[c] = valid ? 1.0 : 0.0;
                X[c + PH * PW] = valid ? cur[o] : 0.0;
                X[c + 2 * PH * PW] = valid ? cur[o + MN] : 0.0;
            }
        for (int q = 0; q < 3; ++q) {
            const double *Xq = &X[q * PH * PW];
            double *Tq = &T[q * (size_t)M * PW];
            for (size_t c = 0; c < PW; ++c)
                for (int m = 0; m < M; ++m) Tq[m + (size_t)M * c] = gq::fc_rows(&Xq[m + PH * c], r, f);
            for (int n = 0; n < N; ++n)
                for (int m = 0; m < M; ++m) Y[q * MN + m + (size_t)M * n] = gq::fc_cols(&Tq[m + (size_t)M * n], M, r, f);
        }
        for (size_t o = 0; o < MN; ++o) {
            const bool fill = gq::fc_fills(state[o], Y[o]);
            if (fill) {
                cur[o] = Y[MN + o] / Y[o];
                cur[o + MN] = Y[2 * MN + o] / Y[o];
            }
            next[o] = fill ? (unsigned char)p : state[o];
        }
        state.swap(next);
    }
    std::memcpy(out, cur.data(), sizeof(double) * 2 * MN);
    if (filled) std::memcpy(filled, state.data(), MN);
    return GQMAP_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Weighted flow denoising, host model: the arithmetic of gqmap_denoise.h, the
// two phases of an iteration (rules, then sum and step) each split over columns
// among the threads.  A column's results depend on no other column of the same
// phase and the maxima are taken on bit patterns, so the thread count shows in
// no result.  Bit for bit what gqmap_flow_denoise computes.
// ---------------------------------------------------------------------------
namespace {

int dn_threads()
{
    const char *e = std::getenv("GQMAP_HOST_THREADS");
    int n = e ? std::atoi(e) : (int)std::min(16u, std::thread::hardware_concurrency());
    return std::max(1, std::min(n, 256));
}

// fn(tid, n0, n1) over a static split of the columns [0, ncols) among nthreads
template <class F>
void dn_columns(int nthreads, int ncols, F fn)
{
    nthreads = std::max(1, std::min(nthreads, ncols));
    std::vector<std::thread> pool;
    for (int t = 1; t < nthreads; ++t)
        pool.emplace_back(fn, t, (int)((int64_t)ncols * t / nthreads), (int)((int64_t)ncols * (t + 1) / nthreads));
    fn(0, 0, (int)((int64_t)ncols / nthreads));
    for (std::thread &th : pool) th.join();
}

template <int KT>
int dn_host_run(const gqmap_cpu_options *o, const gq::DnRule &R, const double *flow, const double *var, int M, int N, bool adjoint, double *mu, double *sigma, double *rou, double *trace)
{
    const size_t MN = (size_t)M * N;
    std::vector<double> dnode(4 * MN, 0.0), dedge(20 * MN, 0.0);
    const int T = dn_threads();
    std::vector<unsigned long long> mx(3 * (size_t)T);
    int done = 0;
    for (int it = 1;; ++it) {
        dn_columns(T, N - 1, [&](int, int n0, int n1) {
            for (int n = n0; n < n1; ++n)
                for (int l = 0; l < 2; ++l)
                    for (int m = 0; m < M - 1; ++m) {
                        const size_t q = gq::dn_i3(M, N, m, n, l);
                        const double o1 = sigma[q], u1 = mu[q], f = flow[q], v = var ? var[q] : o->var;
                        double dn[2];
                        gq::dn_node<KT, GQ_DN_VAR_FIELD>(R, std::sqrt(2.0) * o1, u1, f, v,
                                                         gq::dn_observed(f, var != nullptr, v), dn);
                        dnode[gq::dn_i4(M, N, m, n, 0, l)] = dn[0];
                        dnode[gq::dn_i4(M, N, m, n, 1, l)] = dn[1];
                        for (int j = 0; j < 2; ++j) {
                            const size_t q2 = gq::dn_i3(M, N, m + (j == 0), n + (j == 1), l);
                            double de[5];
                            gq::dn_edge<KT, false, false>(R, rou[gq::dn_i4(M, N, m, n, j, l)], o1, u1, sigma[q2], mu[q2], de);
                            for (int k = 0; k < 5; ++k) dedge[gq::dn_i5(M, N, m, n, j, k, l)] = de[k];
                        }
                    }
        });
        std::fill(mx.begin(), mx.end(), 0ull);
        const double step = gq::dn_step(o->step0, it, o->step_decay);
        dn_columns(T, N, [&](int tid, int n0, int n1) {
            unsigned long long *r = &mx[3 * (size_t)tid];
            for (int n = n0; n < n1; ++n)
                for (int l = 0; l < 2; ++l)
                    for (int m = 0; m < M; ++m) {
                        double a, b;
                        if (adjoint) gq::dn_gather<true>(dnode.data(), dedge.data(), M, N, m, n, l, a, b);
                        else gq::dn_gather<false>(dnode.data(), dedge.data(), M, N, m, n, l, a, b);
                        const double mp = gq::dn_apply(mu, sigma, rou, dedge.data(), M, N, m, n, l, a, b, step, o->corr_tor);
                        r[0] = std::max(r[0], gq::dn_abits(a));
                        r[1] = std::max(r[1], gq::dn_abits(b));
                        r[2] = std::max(r[2], gq::dn_abits(mp));
                    }
        });
        unsigned long long top[3] = {0, 0, 0};
        for (int t = 0; t < T; ++t)
            for (int k = 0; k < 3; ++k) top[k] = std::max(top[k], mx[3 * (size_t)t + k]);
        if (trace)
            for (int k = 0; k < 3; ++k) trace[3 * (size_t)(it - 1) + k] = gq::dn_from_bits(top[k]);
        done = it;
        if (gq::dn_stop(it, o->its, o->min_its, gq::dn_from_bits(top[0]), o->tor)) break;
    }
    return done;
}

}  // namespace

extern "C" {

gqmap_status gqmap_flow_denoise_host(const gqmap_cpu_options *o, const double *flow, const double *var,
                                     const double *mu0, int M, int N, const double *sigma0, uint64_t seed,
                                     int scatter, double *mu, double *sigma, double *rou, double *trace,
                                     int *its_done)
{
    gq::clear_error();
    const char *fn = "gqmap_flow_denoise_host";
    GQ_CHECK(o && flow && mu && sigma && rou, GQMAP_ERR_INVALID_ARG, "%s: null argument", fn);
    GQ_CHECK(M >= 2 && N >= 2, GQMAP_ERR_INVALID_ARG, "%s: flow %dx%d too small", fn, M, N);
    GQ_CHECK(o->K >= 1 && o->K <= GQMAP_KMAX, GQMAP_ERR_INVALID_ARG, "K=%d outside [1,%d]", o->K, GQMAP_KMAX);
    GQ_CHECK(o->its >= 1, GQMAP_ERR_INVALID_ARG, "its=%d", o->its);
    GQ_CHECK(scatter == GQMAP_SCATTER_REFERENCE || scatter == GQMAP_SCATTER_ADJOINT, GQMAP_ERR_INVALID_ARG,
             "%s: scatter=%d (0: reference, 1: adjoint)", fn, scatter);
    const size_t MN = (size_t)M * N;
    const double *start = mu0 ? mu0 : flow;
    for (size_t i = 0; i < 2 * MN; ++i)
        GQ_CHECK(gq::dn_finite(start[i]), GQMAP_ERR_INVALID_ARG, "%s: %s", fn,
                 mu0 ? "mu0 must be finite everywhere" : "without mu0 the flow is the start and must be finite everywhere");
    static_assert(GQMAP_KMAX == 16, "DnRule's arrays");
    gq::DnRule R{};
    R.K = o->K; R.gama = o->gama; R.dta = o->dta;
    if (gq::gauss_hermite(o->K, R.X, R.W) != 0) {
        gq::set_error("Gauss-Hermite did not converge for K=%d", o->K);
        return GQMAP_ERR_INVALID_ARG;
    }
    for (int c = 0; c < o->K; ++c)
        for (int r = 0; r < o->K; ++r) R.WW[r + o->K * c] = R.W[c] * R.W[r];  // WIWJ (:5-6)
    std::memmove(mu, start, sizeof(double) * 2 * MN);
    if (sigma0) {
        std::memmove(sigma, sigma0, sizeof(double) * 2 * MN);
    } else {
        const uint64_t base = gq::stream_base(seed, 3);
        for (size_t i = 0; i < 2 * MN; ++i) sigma[i] = gq::u01(base, (uint64_t)i) + 2;
    }
    std::fill(rou, rou + 4 * MN, 0.0);
    const bool adjoint = scatter == GQMAP_SCATTER_ADJOINT;
    const int done = o->K == 9 ? dn_host_run<9>(o, R, flow, var, M, N, adjoint, mu, sigma, rou, trace)
                               : dn_host_run<0>(o, R, flow, var, M, N, adjoint, mu, sigma, rou, trace);
    if (its_done) *its_done = done;
    return GQMAP_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Weighted median filter, host model: the arithmetic of gqmap_wmedian.h, pixel
// by pixel.  The window's live entries are sorted by key and the integer
// weights summed from the smallest key up; the columns are split among the
// threads, and a pixel's result depends on the pass's input alone, so the
// thread count shows in no result.  Bit for bit what gqmap_flow_wmedian
// computes.
// ---------------------------------------------------------------------------
extern "C" {

gqmap_status gqmap_flow_wmedian_host(const double *flow, const double *guide, const double *conf, int M, int N, int r,
                                     double sigma_s, double sigma_c, int passes, double *out)
{
    gq::clear_error();
    GQ_CHECK(flow && guide && out, GQMAP_ERR_INVALID_ARG, "gqmap_flow_wmedian_host: null argument");
    const char *bad = gq::wm_bad(M, N, r, sigma_s, sigma_c, passes);
    GQ_CHECK(!bad, GQMAP_ERR_INVALID_ARG,
             "gqmap_flow_wmedian_host: %s (M=%d N=%d r=%d sigma_s=%g sigma_c=%g passes=%d)", bad, M, N, r, sigma_s,
             sigma_c, passes);
    const gq::WmFilter f = gq::wm_filter(r, sigma_s);
    const size_t MN = (size_t)M * N;
    std::vector<uint64_t> cur(2 * MN), nxt(2 * MN);
    std::memcpy(cur.data(), flow, sizeof(double) * 2 * MN);
    for (int p = 1; p <= passes; ++p) {
        dn_columns(dn_threads(), N, [&](int, int n0, int n1) {
            std::vector<uint32_t> wq;
            std::vector<std::pair<uint64_t, uint32_t>> live;
            for (int n = n0; n < n1; ++n)
                for (int m = 0; m < M; ++m) {
                    const int i0 = std::max(m - r, 0), i1 = std::min(m + r, M - 1);
                    const int j0 = std::max(n - r, 0), j1 = std::min(n + r, N - 1);
                    const size_t o = m + (size_t)M * n;
                    wq.clear();
                    for (int j = j0; j <= j1; ++j)
                        for (int i = i0; i <= i1; ++i) {
                            const size_t q = i + (size_t)M * j;
                            wq.push_back(gq::wm_wq(f.s[i - m + r] * f.s[j - n + r], guide[q], guide[o], sigma_c,
                                                   conf ? conf[q] : 1.0));
                        }
                    for (int c = 0; c < 2; ++c) {
                        const uint64_t *plane = &cur[c * MN];
                        live.clear();
                        uint32_t total = 0, e = 0;
                        for (int j = j0; j <= j1; ++j)
                            for (int i = i0; i <= i1; ++i, ++e) {
                                const uint64_t key = gq::wm_key(plane[i + (size_t)M * j]);
                                if (wq[e] > 0 && !gq::wm_key_nan(key)) {
                                    live.emplace_back(key, wq[e]);
                                    total += wq[e];
                                }
                            }
                        uint64_t bits = plane[o];
                        if (total > 0) {
                            std::sort(live.begin(), live.end());
                            uint32_t cum = 0;
                            for (const auto &kv : live) {
                                cum += kv.second;
                                if (2 * cum >= total) {
                                    bits = gq::wm_unkey(kv.first);
                                    break;
                                }
                            }
                        }
                        nxt[c * MN + o] = bits;
                    }
                }
        });
        cur.swap(nxt);
    }
    std::memcpy(out, cur.data(), sizeof(double) * 2 * MN);
    return GQMAP_OK;
}

}  // extern "C"
