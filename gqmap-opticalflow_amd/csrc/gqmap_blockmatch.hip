// Block-matching initialiser on the device (legacy/optical_flow_temp.m:13-32 +
// legacy/Gaussian_filter.m): Gaussian-filtered SAD over a (2U+1) x (2V+1)
// window, argmin displacement per pixel.  The arithmetic is gqmap_blockmatch.h
// (shared with the host model gqmap_block_match_host); this file is the tiling.
//
// One workgroup of 256 lanes owns a 32 x TN output tile (rows x columns, TN =
// 8, 16 or 32).  It stages the A tile (halo ft) and the B window (halo ft+U
// rows, ft+V columns) in LDS once, zero outside the frame, then scans the
// displacements: row pass of the abs-difference into an LDS tile T (32 x
// (TN+2ft), double-buffered so one barrier per displacement is enough), column
// pass out of T, running (min, index) in registers.  The cost volume never
// exists in device memory.  Lanes run along m (the fastest index): global
// loads, the final stores and every LDS access are unit-stride over a wave half.
//
// One kernel template, three modes (gqmap_blockmatch.h has their rules):
//   single  1 scan; stores the argmin's flow and cost.
//   multi   H scans ("Several hypotheses").  Every lane builds T at every
//           displacement; only its own keep is gated by the distance to its
//           earlier picks, which stay in registers packed (u, v), one per rank
//           and output column.  Scan r stores rank r's flow and cost.
//   refine  H + 1 scans ("Sub-pixel refinement").  The neighbour costs of a
//           pick are known only once its scan has ended and the cost volume
//           does not exist, so they are computed again: scan r < H selects
//           rank r as multi does; scan r >= 1 also keeps the cost of every
//           displacement one step on an axis from rank r - 1's pick
//           (bm_capture: four integer compares per output column and
//           displacement, 4 NPT doubles in registers) and stores rank r - 1's
//           flow, cost and curvature.  The last scan selects nothing.
// The mode is a template parameter, not an argument: the refine kernel at TN =
// 32 fills the 128 VGPRs that still give bm_choose_cols its four workgroups per
// CU, and the single kernel must not carry the ranked kernels' registers.
#include <hip/hip_runtime.h>

#include <cmath>

#include "gqmap_internal.h"
#include "gqmap_blockmatch.h"

namespace gq {

constexpr int BM_TM = 32;        // tile rows = lanes along m
constexpr int BM_GROUPS = 8;     // column groups of a 256-lane workgroup
constexpr int BM_THREADS = BM_TM * BM_GROUPS;

enum BmMode { BM_SINGLE, BM_MULTI, BM_REFINE };

// LDS doubles of one workgroup: A tile, B window, two T tiles
static size_t bm_lds_doubles(int TN, int U, int V, int ft)
{
    const size_t AH = BM_TM + 2 * ft, AW = TN + 2 * ft;
    return AH * AW + (AH + 2 * U) * (AW + 2 * V) + 2 * (size_t)BM_TM * AW;
}

// NPT = output columns per lane: TN = 8 * NPT.  The single mode ignores H, sep
// and curv; multi ignores curv.  cost may be null, and so may curv.
template <int NPT, int MODE>
__global__ __launch_bounds__(BM_THREADS) void k_block_match(const double *__restrict__ A,
                                                            const double *__restrict__ B, int M, int N, int U,
                                                            int V, int ft, BmFilter f, int tiles_m, int H, int sep,
                                                            double *__restrict__ flow, double *__restrict__ cost,
                                                            double *__restrict__ curv)
{
    extern __shared__ double bm_lds[];
    constexpr int TN = BM_GROUPS * NPT;
    constexpr bool RANKED = MODE != BM_SINGLE, REFINE = MODE == BM_REFINE;
    constexpr int MAX_SCANS = !RANKED ? 1 : REFINE ? GQ_BM_HMAX + 1 : GQ_BM_HMAX;
    const int AH = BM_TM + 2 * ft, AW = TN + 2 * ft, BH = AH + 2 * U, BW = AW + 2 * V;
    double *As = bm_lds, *Bs = As + AH * AW, *Ts = Bs + BH * BW;
    const int tid = threadIdx.x;
    const int m0 = (int)(blockIdx.x % tiles_m) * BM_TM, n0 = (int)(blockIdx.x / tiles_m) * TN;

    for (int t = tid; t < AH * AW; t += BM_THREADS) {
        const int gm = m0 - ft + t % AH, gn = n0 - ft + t / AH;
        As[t] = gm >= 0 && gm < M && gn >= 0 && gn < N ? A[gm + (int64_t)M * gn] : 0.0;
    }
    for (int t = tid; t < BH * BW; t += BM_THREADS) {
        const int gm = m0 - ft - U + t % BH, gn = n0 - ft - V + t / BH;
        Bs[t] = gm >= 0 && gm < M && gn >= 0 && gn < N ? B[gm + (int64_t)M * gn] : 0.0;
    }
    __syncthreads();

    const int lm = tid % BM_TM, cg = tid / BM_TM;
    const int nu = 2 * U + 1, nd = nu * (2 * V + 1);
    const int scans = !RANKED ? 1 : REFINE ? H + 1 : H;
    const int64_t MN = (int64_t)M * N;
    const int gm = m0 + lm;
    // ranked modes: the earlier picks.  refine: rank r - 1's pick (-1 when that rank is missing), its cost, and
    // its neighbour costs, filled during scan r
    [[maybe_unused]] int pick[NPT][GQ_BM_HMAX - 1], last[NPT];
    [[maybe_unused]] double c0[NPT];
    [[maybe_unused]] BmNear nbr[NPT];
    // T's buffer parity runs on a counter over the displacements of ALL scans, not on idx: a scan has an odd
    // number of displacements, so idx & 1 would put the last T of a scan and the first of the next into one
    // buffer, with no barrier between a slow wave's column pass and a fast wave's row pass.  With the running
    // counter consecutive displacements alternate throughout and the one barrier per displacement covers the scan
    // boundary like any other step.  (In the single mode the counter is idx.)
    unsigned done = 0;
    // unrolled over the compile-time bound, so no index into pick is dynamic; the break is block-uniform and every
    // lane reaches every barrier
#pragma unroll
    for (int r = 0; r < MAX_SCANS; ++r) {
        if (r >= scans) break;
        double best[NPT];
        int bidx[NPT];
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
            best[k] = INFINITY;
            bidx[k] = RANKED ? -1 : 0;
            if constexpr (REFINE) bm_near_clear(nbr[k]);
        }
        int u = 0, v = 0;
        for (int idx = 0; idx < nd; ++idx, ++done) {
            double *T = Ts + (done & 1u) * (BM_TM * AW);
            for (int c = cg; c < AW; c += BM_GROUPS) {
                const int gn = n0 - ft + c;
                T[lm + BM_TM * c] = bm_rows(As + lm + AH * c, Bs + (lm + u) + BH * (c + v), ft, f, m0 + lm - ft, M,
                                            gn >= 0 && gn < N);
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < NPT; ++k) {
                if constexpr (MODE == BM_SINGLE) {
                    bm_keep(bm_cols(T + lm + BM_TM * (cg + BM_GROUPS * k), BM_TM, ft, f), idx, best[k], bidx[k]);
                } else if constexpr (MODE == BM_MULTI) {
                    // the exclusion test before the column pass: integer work on registers, which the compiler
                    // then places ahead of the barrier.  refine below has the other order.  Each is the order
                    // its mode was timed with; one order for both was slower in one of them.
                    bool allowed = true;
#pragma unroll
                    for (int j = 0; j < GQ_BM_HMAX - 1; ++j)
                        if (j < r) allowed = allowed && bm_far(u, v, pick[k][j], sep);
                    bm_keep_allowed(allowed, bm_cols(T + lm + BM_TM * (cg + BM_GROUPS * k), BM_TM, ft, f), idx, best[k],
                                    bidx[k]);
                } else {
                    const double c = bm_cols(T + lm + BM_TM * (cg + BM_GROUPS * k), BM_TM, ft, f);
                    if (r < H) {
                        bool allowed = true;
#pragma unroll
                        for (int j = 0; j < GQ_BM_HMAX - 1; ++j)
                            if (j < r) allowed = allowed && bm_far(u, v, pick[k][j], sep);
                        bm_keep_allowed(allowed, c, idx, best[k], bidx[k]);
                    }
                    if (r >= 1) bm_capture(u, v, last[k], c, nbr[k]);
                }
            }
            if (++u == nu) {
                u = 0;
                ++v;
            }
        }
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
            const int gn = n0 + cg + BM_GROUPS * k;
            const bool inside = gm < M && gn < N, found = !RANKED || bidx[k] >= 0;
            const int64_t o = gm + (int64_t)M * gn;
            if constexpr (REFINE) {
                if (r >= 1 && inside) {  // rank r - 1, its neighbour costs now known
                    double out[4];
                    bm_refined(last[k], c0[k], nbr[k], U, V, out);
                    flow[o + 2 * MN * (r - 1)] = out[0];
                    flow[o + 2 * MN * (r - 1) + MN] = out[1];
                    if (cost) cost[o + MN * (r - 1)] = c0[k];
                    if (curv) {
                        curv[o + 2 * MN * (r - 1)] = out[2];
                        curv[o + 2 * MN * (r - 1) + MN] = out[3];
                    }
                }
            } else if (inside) {  // rank r
                flow[o + 2 * MN * r] = found ? (double)(V - bidx[k] / nu) : bm_nan();       // vmt
                flow[o + 2 * MN * r + MN] = found ? (double)(U - bidx[k] % nu) : bm_nan();  // umt
                if (cost) cost[o + MN * r] = best[k];
            }
            if constexpr (RANKED) {  // this scan's pick, for the scans after it
                const int p = found ? bm_pack(bidx[k] % nu, bidx[k] / nu) : -1;
                if constexpr (REFINE) {
                    last[k] = p;
                    c0[k] = best[k];
                }
                // a missing rank adds no exclusion: the allowed set stays empty for the later ranks
                if (r < GQ_BM_HMAX - 1) pick[k][r < GQ_BM_HMAX - 1 ? r : 0] = found ? p : pick[k][r > 0 ? r - 1 : 0];
            }
        }
    }
}

// Tile width from the workgroups a CU holds at once.  The displacement loop
// is a chain of LDS round trips with a barrier each, so what hides its latency
// is resident waves: per CU min(LDS limit, 8 workgroups = the 32-wave cap, the
// grid's workgroups per CU).  A wider tile repeats less of the row pass in its
// column halo, so the widest width that keeps 4 workgroups (4 waves per SIMD)
// resident wins; when none does, the width with the most, ties to the wider.
static int bm_choose_cols(int M, int N, int U, int V, int ft, int cus)
{
    const double lds_cu = 160.0 * 1024, tiles_m = (M + BM_TM - 1) / BM_TM;
    int cols = 8;
    double most = -1;
    for (int tn = 32; tn >= 8; tn /= 2) {
        const double by_lds = std::floor(lds_cu / (bm_lds_doubles(tn, U, V, ft) * sizeof(double)));
        const double by_grid = tiles_m * ((N + tn - 1) / tn) / (cus > 0 ? cus : 1);
        const double res = std::fmin(std::fmin(by_lds, 8.0), by_grid);
        if (res >= 4) return tn;
        if (res > most) {
            most = res;
            cols = tn;
        }
    }
    return cols;
}

// tile columns forced by gqmap_debug_block_match_cols (0: chosen from the grid)
static int g_bm_cols = 0;
int bm_forced_cols() { return g_bm_cols; }  // gqmap_blockmatch_window.hip follows the same debug switch

// H = 0: the single mode (gqmap_block_match); H >= 1: multi, or with refine the refine mode (dcurv may be null)
template <int NPT>
static hipError_t bm_launch(const double *dA, const double *dB, int M, int N, int U, int V, int ft,
                            const BmFilter &f, int H, int sep, bool refine, double *dflow, double *dcost,
                            double *dcurv, hipStream_t s)
{
    constexpr int TN = BM_GROUPS * NPT;
    const auto kernel = H == 0   ? &k_block_match<NPT, BM_SINGLE>
                        : refine ? &k_block_match<NPT, BM_REFINE>
                                 : &k_block_match<NPT, BM_MULTI>;
    const size_t bytes = bm_lds_doubles(TN, U, V, ft) * sizeof(double);
    // above 64 KB (up to 117 KB at U = V = 32, ft = 4, TN = 32) the dynamic LDS limit must be raised
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return e;
    const int tiles_m = (M + BM_TM - 1) / BM_TM, tiles_n = (N + TN - 1) / TN;
    const dim3 grid((unsigned)((int64_t)tiles_m * tiles_n)), block(BM_THREADS);
    kernel<<<grid, block, bytes, s>>>(dA, dB, M, N, U, V, ft, f, tiles_m, H, sep, dflow, dcost, dcurv);
    return hipGetLastError();
}

}  // namespace gq

using namespace gq;

namespace {
// gqmap_block_match (H = 0), gqmap_block_match_multi (H >= 1) and gqmap_block_match_refine (H >= 1, refine; curv
// may be null) behind one body; who names the caller in errors
static gqmap_status bm_device(const char *who, const double *A, const double *B, int M, int N, int U, int V, int ft,
                              double sigma, int H, int sep, bool refine, double *flow, double *cost, double *curv,
                              double *elapsed_ms, int device)
{
    clear_error();
    GQ_CHECK(A && B && flow, GQMAP_ERR_INVALID_ARG, "%s: null argument", who);
    const char *bad = bm_bad_args(M, N, U, V, ft, sigma);
    GQ_CHECK(!bad, GQMAP_ERR_INVALID_ARG, "%s: %s (M=%d N=%d U=%d V=%d ft=%d sigma=%g)", who, bad, M,
             N, U, V, ft, sigma);
    GQ_CHECK((int64_t)((M + BM_TM - 1) / BM_TM) * ((N + 7) / 8) <= 0x7fffffff, GQMAP_ERR_INVALID_ARG,
             "%s: %dx%d has too many tiles", who, M, N);
    GQ_CHECK(gqmap_device_count() > device && device >= 0, GQMAP_ERR_NO_DEVICE, "no HIP device %d", device);
    DeviceGuard dg(device);
    const BmFilter f = bm_filter(ft, sigma);
    int cus = 0;
    GQ_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    int cols = g_bm_cols;
    if (cols == 0) cols = bm_choose_cols(M, N, U, V, ft, cus);

    const size_t bytes = sizeof(double) * (size_t)M * N, ranks = H == 0 ? 1 : (size_t)H;
    DevBuf dA, dB, dflow, dcost, dcurv;
    Events ev;
    GQ_HIP(hipMalloc(&dA.p, bytes));
    GQ_HIP(hipMalloc(&dB.p, bytes));
    GQ_HIP(hipMalloc(&dflow.p, 2 * ranks * bytes));
    if (cost) GQ_HIP(hipMalloc(&dcost.p, ranks * bytes));
    if (refine && curv) GQ_HIP(hipMalloc(&dcurv.p, 2 * ranks * bytes));
    GQ_HIP(hipMemcpy(dA.p, A, bytes, hipMemcpyHostToDevice));
    GQ_HIP(hipMemcpy(dB.p, B, bytes, hipMemcpyHostToDevice));
    if (elapsed_ms) {
        GQ_HIP(hipEventCreate(&ev.a));
        GQ_HIP(hipEventCreate(&ev.b));
        GQ_HIP(hipEventRecord(ev.a, 0));
    }
    const double *a = (const double *)dA.p, *b = (const double *)dB.p;
    double *df = (double *)dflow.p, *dc = (double *)dcost.p, *dk = (double *)dcurv.p;
    GQ_HIP(cols == 32   ? bm_launch<4>(a, b, M, N, U, V, ft, f, H, sep, refine, df, dc, dk, 0)
           : cols == 16 ? bm_launch<2>(a, b, M, N, U, V, ft, f, H, sep, refine, df, dc, dk, 0)
                        : bm_launch<1>(a, b, M, N, U, V, ft, f, H, sep, refine, df, dc, dk, 0));
    if (elapsed_ms) {
        float ms = 0;
        GQ_HIP(hipEventRecord(ev.b, 0));
        GQ_HIP(hipEventSynchronize(ev.b));
        GQ_HIP(hipEventElapsedTime(&ms, ev.a, ev.b));
        *elapsed_ms = ms;
    }
    GQ_HIP(hipMemcpy(flow, dflow.p, 2 * ranks * bytes, hipMemcpyDeviceToHost));
    if (cost) GQ_HIP(hipMemcpy(cost, dcost.p, ranks * bytes, hipMemcpyDeviceToHost));
    if (dcurv.p) GQ_HIP(hipMemcpy(curv, dcurv.p, 2 * ranks * bytes, hipMemcpyDeviceToHost));
    return GQMAP_OK;
}
}  // namespace

extern "C" {

// Not in the public header (tests): force the tile width to 8, 16 or 32
// columns; 0 restores the choice from the grid.  Never changes a result.
int gqmap_debug_block_match_cols(int cols)
{
    if (cols != 0 && cols != 8 && cols != 16 && cols != 32) return -1;
    g_bm_cols = cols;
    return 0;
}

gqmap_status gqmap_block_match(const double *A, const double *B, int M, int N, int U, int V, int ft,
                               double sigma, double *flow, double *cost, double *elapsed_ms, int device)
{
    return bm_device("gqmap_block_match", A, B, M, N, U, V, ft, sigma, 0, 1, false, flow, cost, nullptr, elapsed_ms,
                     device);
}

gqmap_status gqmap_block_match_multi(const double *A, const double *B, int M, int N, int U, int V, int ft,
                                     double sigma, int H, int sep, double *flow, double *cost, double *elapsed_ms,
                                     int device)
{
    clear_error();
    const char *bad = bm_bad_multi(H, sep);
    GQ_CHECK(!bad, GQMAP_ERR_INVALID_ARG, "gqmap_block_match_multi: %s (H=%d sep=%d)", bad, H, sep);
    return bm_device("gqmap_block_match_multi", A, B, M, N, U, V, ft, sigma, H, sep, false, flow, cost, nullptr,
                     elapsed_ms, device);
}

gqmap_status gqmap_block_match_refine(const double *A, const double *B, int M, int N, int U, int V, int ft,
                                      double sigma, int H, int sep, double *flow, double *cost, double *curv,
                                      double *elapsed_ms, int device)
{
    clear_error();
    const char *bad = bm_bad_multi(H, sep);
    GQ_CHECK(!bad, GQMAP_ERR_INVALID_ARG, "gqmap_block_match_refine: %s (H=%d sep=%d)", bad, H, sep);
    return bm_device("gqmap_block_match_refine", A, B, M, N, U, V, ft, sigma, H, sep, true, flow, cost, curv,
                     elapsed_ms, device);
}

}  // extern "C"
