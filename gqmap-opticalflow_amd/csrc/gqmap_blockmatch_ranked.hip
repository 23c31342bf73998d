// Ranked hypotheses over per-pixel windows, and through the coarse-to-fine
// matcher ("Ranked windows" and "Ranked coarse to fine" of gqmap_blockmatch.h,
// shared with the host models in gqmap_host.cpp).  This file is the tiling.
//
// k_block_match_ranked keeps the tile form of k_block_match_window
// (gqmap_blockmatch_window.hip): 256 lanes own 32 x TN outputs, lanes along m,
// the A tile and a chunked B window in LDS, T double-buffered, one barrier per
// displacement with the vote riding on it.  The rank loop is outermost:
//   A tile      staged once for all ranks.
//   per rank    the lane loads that rank's boxes of its NPT outputs (4 NPT ints,
//               not 4 NPT H), the workgroup reduces the union box again (un is
//               reset behind a barrier), walks it in chunks, runs the refine walk
//               over the neighbours of this rank's picks and stores this rank's
//               flow, cost, curv and pick planes.
//   exclusion   only the keys of the earlier ranks survive a rank: three ints
//               per output, shifted down after every rank (no indexed register
//               array).  The keep is gated by the lane's own box and by
//               bm_far_key against those keys; a lane wants a displacement only
//               when it is in its box AND allowed, so skipping follows the
//               allowed set.
// The two helper kernels of the pyramid (k_bm_half, k_bm_window_up) are the
// window file's, launched through bmw_half_launch / bmw_window_up_launch once
// per level and once per rank.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "gqmap_internal.h"
#include "gqmap_blockmatch.h"

namespace gq {

int bm_forced_cols();  // gqmap_blockmatch.hip: the tile width of gqmap_debug_block_match_cols
// gqmap_blockmatch_window.hip: the tile's LDS, the tile width rule, the debug switches and the helper kernels
size_t bmw_lds_doubles(int TN, int CU, int CV, int ft);
int bmw_choose_cols(int M, int N, int CU, int CV, int ft, int cus);
void bmw_forced_chunk(int *cu, int *cv);
bool bmw_stats_on();
double *bmw_stats_last(int level);
hipError_t bmw_half_launch(const double *dP, int M, int N, double *dout, int Mh, int Nh, hipStream_t s);
hipError_t bmw_window_up_launch(const int *dpick, int Mc, int Nc, int M, int N, int r, int k, int *dwin, hipStream_t s);

constexpr int BMR_TM = 32;     // tile rows = lanes along m, as BMW_TM
constexpr int BMR_GROUPS = 8;  // column groups of a 256-lane workgroup
constexpr int BMR_THREADS = BMR_TM * BMR_GROUPS;
constexpr int BMR_CHUNK_DEFAULT = 17;  // chunk extent when the windows' extent is not known to the host

// win (M x N x 4 x H) or, when null, the box cbox at every pixel and rank.  flow, curv (M x N x 2 x H), cost (M x N x H)
// and pick (per rank the planes du, dv) may each be null; stats as k_block_match_window's, summed over the ranks.
template <int NPT, bool REFINE>
__global__ __launch_bounds__(BMR_THREADS) void k_block_match_ranked(
    const double *__restrict__ A, const double *__restrict__ B, const int *__restrict__ win, int4 cbox, int M, int N,
    int ft, BmFilter f, int tiles_m, int CU, int CV, int H, int sep, double *__restrict__ flow,
    double *__restrict__ cost, double *__restrict__ curv, int *__restrict__ pick,
    unsigned long long *__restrict__ stats)
{
    extern __shared__ double bmr_lds[];
    __shared__ int un[4], vote[3];
    constexpr int TN = BMR_GROUPS * NPT;
    const int AH = BMR_TM + 2 * ft, AW = TN + 2 * ft, BH = AH + CU - 1, BW = AW + CV - 1;
    double *As = bmr_lds, *Bs = As + AH * AW, *Ts = Bs + BH * BW;
    const int tid = threadIdx.x;
    const int m0 = (int)(blockIdx.x % tiles_m) * BMR_TM, n0 = (int)(blockIdx.x / tiles_m) * TN;
    const int lm = tid % BMR_TM, cg = tid / BMR_TM;
    const int gm = m0 + lm;
    const int64_t MN = (int64_t)M * N;

    for (int t = tid; t < AH * AW; t += BMR_THREADS) {
        const int am = m0 - ft + t % AH, an = n0 - ft + t / AH;
        As[t] = am >= 0 && am < M && an >= 0 && an < N ? A[am + (int64_t)M * an] : 0.0;
    }
    if (tid == 0) vote[0] = vote[1] = vote[2] = 0;
    // the keys of the three ranks before this one, the latest first; GQ_BM_NOPICK excludes nothing
    int prev[NPT][3];
#pragma unroll
    for (int k = 0; k < NPT; ++k) prev[k][0] = prev[k][1] = prev[k][2] = GQ_BM_NOPICK;
    // T's buffer parity runs on a counter over the displacements evaluated, through all ranks; every barrier below is
    // reached by every lane, the branches around them are block-uniform
    unsigned done = 0;
    unsigned long long scanned = 0, area = 0;
    // the workgroup's OR of a flag in ONE barrier, three slots in rotation: see k_block_match_window
    int slot = 0;
    const auto any_lane = [&](bool flag) {
        if (flag) vote[slot] = 1;
        __syncthreads();
        const bool any = vote[slot] != 0;
        if (tid == 0) vote[slot == 0 ? 2 : slot - 1] = 0;
        slot = slot == 2 ? 0 : slot + 1;
        return any;
    };
    for (int j = 0; j < H; ++j) {
        // box j of this lane's output pixels; a pixel outside the frame has the empty box
        const int *wj = win ? win + 4 * MN * j : nullptr;
        int box[NPT][4];
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
            const int gn = n0 + cg + BMR_GROUPS * k;
            const bool inside = gm < M && gn < N;
            const int64_t o = gm + (int64_t)M * gn;
            box[k][0] = !inside ? 1 : wj ? wj[o] : cbox.x;
            box[k][1] = !inside ? 0 : wj ? wj[o + MN] : cbox.y;
            box[k][2] = !inside ? 1 : wj ? wj[o + 2 * MN] : cbox.z;
            box[k][3] = !inside ? 0 : wj ? wj[o + 3 * MN] : cbox.w;
        }
        // rank 0: the A tile and the vote slots are written; later ranks: every lane has read the union box of the
        // rank before and is past its last column pass, so un, Bs and T are free
        __syncthreads();
        if (tid == 0) {
            un[0] = un[2] = GQ_BM_NOPICK;
            un[1] = un[3] = -GQ_BM_NOPICK;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NPT; ++k)
            if (box[k][0] <= box[k][1] && box[k][2] <= box[k][3]) {
                atomicMin(&un[0], box[k][0]);
                atomicMax(&un[1], box[k][1]);
                atomicMin(&un[2], box[k][2]);
                atomicMax(&un[3], box[k][3]);
                area += (unsigned long long)(box[k][1] - box[k][0] + 1) * (unsigned)(box[k][3] - box[k][2] + 1);
            }
        __syncthreads();
        const int Ulo = un[0], Uhi = un[1], Vlo = un[2], Vhi = un[3];  // Ulo > Uhi: no pixel of the tile has a box j

        double best[NPT];
        int key[NPT];
        [[maybe_unused]] BmNear nbr[NPT];
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
            best[k] = INFINITY;
            key[k] = GQ_BM_NOPICK;
            if constexpr (REFINE) bm_near_clear(nbr[k]);
        }
#pragma unroll
        for (int pass = 0; pass < (REFINE ? 2 : 1); ++pass) {
            // bit k: output pixel k of this lane wants the cost of (du, dv) in this walk: in its box and allowed, or a
            // neighbour of its pick on a refinable axis
            const auto wants = [&](int du, int dv) {
                unsigned mask = 0;
#pragma unroll
                for (int k = 0; k < NPT; ++k) {
                    const bool w = pass == 0 ? bm_in_box(box[k], du, dv) && bm_far_key(du, dv, prev[k][0], sep) &&
                                                   bm_far_key(du, dv, prev[k][1], sep) &&
                                                   bm_far_key(du, dv, prev[k][2], sep)
                                             : bm_near_wanted(box[k], du, dv, key[k]);
                    mask |= (unsigned)w << k;
                }
                return mask;
            };
            for (int cv0 = Vlo; cv0 <= Vhi; cv0 += CV)
                for (int cu0 = Ulo; cu0 <= Uhi; cu0 += CU) {
                    const int eu = min(CU, Uhi - cu0 + 1), ev = min(CV, Vhi - cv0 + 1);
                    bool mine = false;
#pragma unroll
                    for (int k = 0; k < NPT; ++k) {
                        if (pass == 0) {
                            mine = mine || (box[k][0] < cu0 + eu && box[k][1] >= cu0 && box[k][2] < cv0 + ev &&
                                            box[k][3] >= cv0);
                        } else {
                            const int pu = bm_key_du(key[k]), pv = bm_key_dv(key[k]);
                            mine = mine || (key[k] != GQ_BM_NOPICK && pu >= cu0 - 1 && pu <= cu0 + eu &&
                                            pv >= cv0 - 1 && pv <= cv0 + ev);
                        }
                    }
                    // the barrier also ends the column pass of the chunk before: Bs and T are free
                    if (!any_lane(mine)) continue;
                    const int h = AH + eu - 1, w = AW + ev - 1;
                    for (int t = tid; t < h * w; t += BMR_THREADS) {
                        const int bm = m0 - ft + cu0 + t % h, bn = n0 - ft + cv0 + t / h;
                        Bs[t % h + BH * (t / h)] =
                            bm >= 0 && bm < M && bn >= 0 && bn < N ? B[bm + (int64_t)M * bn] : 0.0;
                    }
                    int du = cu0, dv = cv0;
                    unsigned mask = wants(du, dv);
                    bool go = any_lane(mask != 0);
                    const int nd = eu * ev;
                    for (int idx = 0; idx < nd; ++idx) {
                        int ndu = du + 1, ndv = dv;
                        if (ndu == cu0 + eu) {
                            ndu = cu0;
                            ++ndv;
                        }
                        const unsigned nmask = idx + 1 < nd ? wants(ndu, ndv) : 0u;
                        double *T = Ts + (done & 1u) * (BMR_TM * AW);
                        if (go)
                            for (int c = cg; c < AW; c += BMR_GROUPS) {
                                const int gn = n0 - ft + c;
                                T[lm + BMR_TM * c] = bm_rows(As + lm + AH * c, Bs + (lm + du - cu0) + BH * (c + dv - cv0),
                                                            ft, f, m0 + lm - ft, M, gn >= 0 && gn < N);
                            }
                        const bool next = any_lane(nmask != 0);
                        if (go) {
#pragma unroll
                            for (int k = 0; k < NPT; ++k) {
                                const double c = bm_cols(T + lm + BMR_TM * (cg + BMR_GROUPS * k), BMR_TM, ft, f);
                                if (pass == 0)
                                    bm_keep_window((mask >> k) & 1u, c, du, dv, best[k], key[k]);
                                else if constexpr (REFINE)
                                    bm_capture_window(du, dv, key[k], c, nbr[k]);
                            }
                            ++done;
                            if (pass == 0) ++scanned;
                        }
                        go = next;
                        mask = nmask;
                        du = ndu;
                        dv = ndv;
                    }
                }
        }
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
            const int gn = n0 + cg + BMR_GROUPS * k;
            if (gm < M && gn < N) {
                const int64_t o = gm + (int64_t)M * gn;
                double out[4];
                if constexpr (REFINE) {
                    bm_refined_window(key[k], best[k], nbr[k], box[k], true, out);
                } else {
                    BmNear none;
                    bm_near_clear(none);
                    bm_refined_window(key[k], best[k], none, box[k], false, out);
                }
                if (flow) {
                    flow[o + 2 * MN * j] = out[0];
                    flow[o + 2 * MN * j + MN] = out[1];
                }
                if (cost) cost[o + MN * j] = best[k];
                if (curv) {
                    curv[o + 2 * MN * j] = out[2];
                    curv[o + 2 * MN * j + MN] = out[3];
                }
                if (pick) {
                    const bool found = key[k] != GQ_BM_NOPICK;
                    pick[o + 2 * MN * j] = found ? bm_key_du(key[k]) : GQ_BM_NOPICK;
                    pick[o + 2 * MN * j + MN] = found ? bm_key_dv(key[k]) : GQ_BM_NOPICK;
                }
            }
            prev[k][2] = prev[k][1];
            prev[k][1] = prev[k][0];
            prev[k][0] = key[k];
        }
    }
    if (stats) {
        if (tid == 0) atomicAdd(&stats[0], scanned);
        if (area) atomicAdd(&stats[1], area);
    }
}

template <int NPT>
static hipError_t bmr_launch(const double *dA, const double *dB, const int *dwin, int4 cbox, int M, int N, int ft,
                             const BmFilter &f, bool refine, int CU, int CV, int H, int sep, double *dflow,
                             double *dcost, double *dcurv, int *dpick, unsigned long long *dstats, hipStream_t s)
{
    constexpr int TN = BMR_GROUPS * NPT;
    const auto kernel = refine ? &k_block_match_ranked<NPT, true> : &k_block_match_ranked<NPT, false>;
    const size_t bytes = bmw_lds_doubles(TN, CU, CV, ft) * sizeof(double);
    // above 64 KB the dynamic LDS limit must be raised, as for k_block_match_window
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return e;
    const int tiles_m = (M + BMR_TM - 1) / BMR_TM, tiles_n = (N + TN - 1) / TN;
    const dim3 grid((unsigned)((int64_t)tiles_m * tiles_n)), block(BMR_THREADS);
    kernel<<<grid, block, bytes, s>>>(dA, dB, dwin, cbox, M, N, ft, f, tiles_m, CU, CV, H, sep, dflow, dcost, dcurv,
                                      dpick, dstats);
    return hipGetLastError();
}

// one level on the device.  ext_u, ext_v: the largest extent of a box when the host knows it, else 0.
static hipError_t bmr_level(const double *dA, const double *dB, const int *dwin, int4 cbox, int M, int N, int ft,
                            const BmFilter &f, bool refine, int ext_u, int ext_v, int cus, int H, int sep,
                            double *dflow, double *dcost, double *dcurv, int *dpick, unsigned long long *dstats,
                            int *tiles)
{
    int fu = 0, fv = 0;
    bmw_forced_chunk(&fu, &fv);
    const auto extent = [](int forced, int ext) {
        return forced ? forced : std::min(GQ_BM_CHUNK, std::max(BMR_CHUNK_DEFAULT, ext));
    };
    const int CU = extent(fu, ext_u), CV = extent(fv, ext_v);
    int cols = bm_forced_cols();
    if (cols == 0) cols = bmw_choose_cols(M, N, CU, CV, ft, cus);
    *tiles = ((M + BMR_TM - 1) / BMR_TM) * ((N + cols - 1) / cols);
    return cols == 32   ? bmr_launch<4>(dA, dB, dwin, cbox, M, N, ft, f, refine, CU, CV, H, sep, dflow, dcost, dcurv,
                                        dpick, dstats, 0)
           : cols == 16 ? bmr_launch<2>(dA, dB, dwin, cbox, M, N, ft, f, refine, CU, CV, H, sep, dflow, dcost, dcurv,
                                        dpick, dstats, 0)
                        : bmr_launch<1>(dA, dB, dwin, cbox, M, N, ft, f, refine, CU, CV, H, sep, dflow, dcost, dcurv,
                                        dpick, dstats, 0);
}

}  // namespace gq

using namespace gq;

namespace {
struct DevBuf {
    void *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p) { o.p = nullptr; }
    ~DevBuf()
    {
        if (p) (void)hipFree(p);
    }
};
struct Events {
    hipEvent_t a = nullptr, b = nullptr;
    hipEvent_t level[GQ_BM_LEVELS + 1] = {};  // counting only: before each level's kernels and after the last
    ~Events()
    {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
        for (hipEvent_t e : level)
            if (e) (void)hipEventDestroy(e);
    }
};

// the tile count of the narrowest tile fits the grid
bool bmr_grid_fits(int M, int N) { return (int64_t)((M + BMR_TM - 1) / BMR_TM) * ((N + 7) / 8) <= 0x7fffffff; }

// gqmap_block_match_window_multi (win given, levels = 1) and gqmap_block_match_pyramid_multi (win null) behind one body
gqmap_status bmr_device(const char *who, const double *A, const double *B, const int *win, int M, int N, int U, int V,
                        int ft, double sigma, int levels, int r, int k, int H, int sep, bool subpixel, double *flow,
                        double *cost, double *curv, double *elapsed_ms, int device)
{
    GQ_CHECK(bmr_grid_fits(M, N), GQMAP_ERR_INVALID_ARG, "%s: %dx%d has too many tiles", who, M, N);
    GQ_CHECK(gqmap_device_count() > device && device >= 0, GQMAP_ERR_NO_DEVICE, "no HIP device %d", device);
    DeviceGuard dg(device);
    const BmFilter f = bm_filter(ft, sigma);
    int cus = 0;
    GQ_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    const int c = levels - 1;
    const bool stats = bmw_stats_on();
    std::vector<int> Ms(levels, M), Ns(levels, N), tiles(levels, 0);
    for (int l = 1; l < levels; ++l) Ms[l] = (Ms[l - 1] + 1) / 2, Ns[l] = (Ns[l - 1] + 1) / 2;
    // the largest extent of a box over all ranks, where the host has the windows
    int ext_u = 0, ext_v = 0;
    if (win) {
        const size_t MN = (size_t)M * N;
        for (int j = 0; j < H; ++j)
            for (size_t o = 0; o < MN; ++o) {
                const int *w = win + 4 * MN * j + o;
                ext_u = std::max(ext_u, w[MN] - w[0] + 1);
                ext_v = std::max(ext_v, w[3 * MN] - w[2 * MN] + 1);
            }
    }

    const size_t bytes = sizeof(double) * (size_t)M * N;
    std::vector<DevBuf> dA(levels), dB(levels), dwin(levels), dpick(levels);
    DevBuf dflow, dcost, dcurv, dstats;
    Events ev;
    for (int l = 0; l < levels; ++l) {
        const size_t mn = (size_t)Ms[l] * Ns[l];
        GQ_HIP(hipMalloc(&dA[l].p, sizeof(double) * mn));
        GQ_HIP(hipMalloc(&dB[l].p, sizeof(double) * mn));
        if (l < c || win) GQ_HIP(hipMalloc(&dwin[l].p, sizeof(int) * 4 * mn * H));
        if (l > 0) GQ_HIP(hipMalloc(&dpick[l].p, sizeof(int) * 2 * mn * H));
    }
    GQ_HIP(hipMalloc(&dflow.p, 2 * bytes * H));
    if (cost) GQ_HIP(hipMalloc(&dcost.p, bytes * H));
    if (curv) GQ_HIP(hipMalloc(&dcurv.p, 2 * bytes * H));
    if (stats) {
        GQ_HIP(hipMalloc(&dstats.p, sizeof(unsigned long long) * 2 * GQ_BM_LEVELS));
        GQ_HIP(hipMemset(dstats.p, 0, sizeof(unsigned long long) * 2 * GQ_BM_LEVELS));
    }
    GQ_HIP(hipMemcpy(dA[0].p, A, bytes, hipMemcpyHostToDevice));
    GQ_HIP(hipMemcpy(dB[0].p, B, bytes, hipMemcpyHostToDevice));
    if (win) GQ_HIP(hipMemcpy(dwin[0].p, win, sizeof(int) * 4 * (size_t)M * N * H, hipMemcpyHostToDevice));
    if (elapsed_ms) {
        GQ_HIP(hipEventCreate(&ev.a));
        GQ_HIP(hipEventCreate(&ev.b));
        GQ_HIP(hipEventRecord(ev.a, 0));
    }
    for (int l = 1; l < levels; ++l) {
        GQ_HIP(bmw_half_launch((const double *)dA[l - 1].p, Ms[l - 1], Ns[l - 1], (double *)dA[l].p, Ms[l], Ns[l], 0));
        GQ_HIP(bmw_half_launch((const double *)dB[l - 1].p, Ms[l - 1], Ns[l - 1], (double *)dB[l].p, Ms[l], Ns[l], 0));
    }
    const int Uc = bm_ceil_shift(U, c), Vc = bm_ceil_shift(V, c);
    if (stats)
        for (int l = 0; l <= levels; ++l) GQ_HIP(hipEventCreate(&ev.level[l]));
    for (int l = c; l >= 0; --l) {
        const bool coarsest = l == c && !win;
        const size_t mn = (size_t)Ms[l] * Ns[l];
        if (stats) GQ_HIP(hipEventRecord(ev.level[l + 1], 0));
        if (l < c) {
            const size_t mnc = (size_t)Ms[l + 1] * Ns[l + 1];
            for (int j = 0; j < H; ++j)  // box j from the coarse level's rank-j pick planes
                GQ_HIP(bmw_window_up_launch((const int *)dpick[l + 1].p + 2 * mnc * j, Ms[l + 1], Ns[l + 1], Ms[l], Ns[l],
                                            r, k, (int *)dwin[l].p + 4 * mn * j, 0));
        }
        unsigned long long *st = stats ? (unsigned long long *)dstats.p + 2 * l : nullptr;
        GQ_HIP(bmr_level((const double *)dA[l].p, (const double *)dB[l].p, coarsest ? nullptr : (const int *)dwin[l].p,
                         make_int4(-Uc, Uc, -Vc, Vc), Ms[l], Ns[l], ft, f, l == 0 && subpixel,
                         coarsest ? 2 * Uc + 1 : ext_u, coarsest ? 2 * Vc + 1 : ext_v, cus, H, sep,
                         l == 0 ? (double *)dflow.p : nullptr, l == 0 ? (double *)dcost.p : nullptr,
                         l == 0 ? (double *)dcurv.p : nullptr, l > 0 ? (int *)dpick[l].p : nullptr, st, &tiles[l]));
    }
    if (stats) GQ_HIP(hipEventRecord(ev.level[0], 0));
    if (elapsed_ms) {
        float ms = 0;
        GQ_HIP(hipEventRecord(ev.b, 0));
        GQ_HIP(hipEventSynchronize(ev.b));
        GQ_HIP(hipEventElapsedTime(&ms, ev.a, ev.b));
        *elapsed_ms = ms;
    }
    GQ_HIP(hipMemcpy(flow, dflow.p, 2 * bytes * H, hipMemcpyDeviceToHost));
    if (cost) GQ_HIP(hipMemcpy(cost, dcost.p, bytes * H, hipMemcpyDeviceToHost));
    if (curv) GQ_HIP(hipMemcpy(curv, dcurv.p, 2 * bytes * H, hipMemcpyDeviceToHost));
    if (stats) {
        unsigned long long st[2 * GQ_BM_LEVELS];
        GQ_HIP(hipMemcpy(st, dstats.p, sizeof st, hipMemcpyDeviceToHost));
        for (int l = 0; l < GQ_BM_LEVELS; ++l) {
            const bool on = l < levels;
            float ms = 0;
            if (on) GQ_HIP(hipEventElapsedTime(&ms, ev.level[l + 1], ev.level[l]));
            double *last = bmw_stats_last(l);
            last[4] = ms;
            last[0] = on ? (double)Ms[l] * Ns[l] : 0.0;
            last[1] = on ? (double)tiles[l] : 0.0;
            last[2] = on ? (double)st[2 * l] : 0.0;
            last[3] = on ? (double)st[2 * l + 1] : 0.0;
        }
    }
    return GQMAP_OK;
}
}  // namespace

extern "C" {

gqmap_status gqmap_block_match_window_multi(const double *A, const double *B, const int *win, int M, int N, int ft,
                                            double sigma, int H, int sep, int subpixel, double *flow, double *cost,
                                            double *curv, double *elapsed_ms, int device)
{
    clear_error();
    GQ_CHECK(A && B && win && flow, GQMAP_ERR_INVALID_ARG, "gqmap_block_match_window_multi: null argument");
    const char *bad = bm_bad_window(M, N, ft, sigma);
    GQ_CHECK(!bad, GQMAP_ERR_INVALID_ARG, "gqmap_block_match_window_multi: %s (M=%d N=%d ft=%d sigma=%g)", bad, M, N, ft,
             sigma);
    bad = bm_bad_multi(H, sep);
    GQ_CHECK(!bad, GQMAP_ERR_INVALID_ARG, "gqmap_block_match_window_multi: %s (H=%d sep=%d)", bad, H, sep);
    for (int j = 0; j < H; ++j)
        GQ_CHECK(!bm_bad_bounds(win + 4 * (size_t)M * N * j, M, N), GQMAP_ERR_INVALID_ARG,
                 "gqmap_block_match_window_multi: a window bound of rank %d outside [-%d,%d]", j, GQ_BM_DMAX, GQ_BM_DMAX);
    return bmr_device("gqmap_block_match_window_multi", A, B, win, M, N, 0, 0, ft, sigma, 1, 0, 0, H, sep, subpixel != 0,
                      flow, cost, curv, elapsed_ms, device);
}

gqmap_status gqmap_block_match_pyramid_multi(const double *A, const double *B, int M, int N, int U, int V, int ft,
                                             double sigma, int levels, int r, int k, int H, int sep, int subpixel,
                                             double *flow, double *cost, double *curv, double *elapsed_ms, int device)
{
    clear_error();
    GQ_CHECK(A && B && flow, GQMAP_ERR_INVALID_ARG, "gqmap_block_match_pyramid_multi: null argument");
    const char *bad = bm_bad_pyramid(M, N, U, V, ft, sigma, levels, r, k);
    GQ_CHECK(!bad, GQMAP_ERR_INVALID_ARG,
             "gqmap_block_match_pyramid_multi: %s (M=%d N=%d U=%d V=%d ft=%d sigma=%g levels=%d r=%d k=%d)", bad, M, N, U,
             V, ft, sigma, levels, r, k);
    bad = bm_bad_multi(H, sep);
    GQ_CHECK(!bad, GQMAP_ERR_INVALID_ARG, "gqmap_block_match_pyramid_multi: %s (H=%d sep=%d)", bad, H, sep);
    return bmr_device("gqmap_block_match_pyramid_multi", A, B, nullptr, M, N, U, V, ft, sigma, levels, r, k, H, sep,
                      subpixel != 0, flow, cost, curv, elapsed_ms, device);
}

}  // extern "C"
