// Block matching with a search window per pixel, the coarse-to-fine matcher
// built on it, and the ranked form of both ("Per-pixel windows", "Coarse to
// fine", "Ranked windows" and "Ranked coarse to fine" of gqmap_blockmatch.h,
// shared with the host models in gqmap_host.cpp).  This file is the tiling.
//
// k_block_match_window keeps the tile form of k_block_match (gqmap_blockmatch.hip):
// 256 lanes own 32 x TN outputs, lanes along m, the A tile and a B window in
// LDS, T double-buffered, one barrier per displacement.  What differs:
//   union box   every lane holds the boxes of its NPT output pixels in registers;
//               the workgroup reduces them to one box (LDS atomics, once).
//   chunks      the union box is walked in chunks of at most CU x CV
//               displacements, CU, CV <= GQ_BM_CHUNK = 65; B is restaged per
//               chunk, so the LDS is that of k_block_match at 2U + 1 = CU, 2V +
//               1 = CV whatever the windows span.  A chunk no pixel of the tile
//               reaches into is skipped before it is staged.
//   skipping    a displacement that no output pixel of the tile wants is not
//               evaluated.  The vote for displacement i + 1 rides on the barrier
//               of displacement i (a flag in LDS, three slots in rotation), so a
//               skipped displacement costs that barrier and a few integer compares.
//   keep        gated per lane by its own box, and by the tie rule of the
//               header, which knows no scan order: chunking, tile width and
//               skipping change no result.
//   sub-pixel   a second walk that evaluates only the neighbours of the picks
//               on their refinable axes and captures their costs (REFINE).
//   ranks       RANKED puts a rank loop around all of that except the A tile,
//               which is staged once.  Per rank the lane loads that rank's boxes
//               of its NPT outputs (4 NPT ints, not 4 NPT H), the workgroup
//               reduces the union box again (un is reset behind a barrier), walks
//               it, runs the refine walk over the neighbours of this rank's picks
//               and stores this rank's flow, cost, curv and pick planes.  Only the
//               keys of the earlier ranks survive a rank: three ints per output,
//               shifted down after every rank (no indexed register array).  A
//               lane wants a displacement only when it is in its box AND
//               bm_far_key from those keys, so keep and skipping follow the
//               allowed set.  Without RANKED none of this is compiled: one rank,
//               no keys, no rank offsets.
// k_bm_half and k_bm_window_up are one lane per output pixel, lanes along m; the
// ranked pyramid launches k_bm_window_up once per level and rank.
// The pyramids keep frames, picks and windows of every level on the device: the
// two frames go up, level 0's outputs come down.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "gqmap_internal.h"
#include "gqmap_blockmatch.h"

namespace gq {

int bm_forced_cols();  // gqmap_blockmatch.hip: the tile width of gqmap_debug_block_match_cols

constexpr int BMW_TM = 32;     // tile rows = lanes along m
constexpr int BMW_GROUPS = 8;  // column groups of a 256-lane workgroup
constexpr int BMW_THREADS = BMW_TM * BMW_GROUPS;
constexpr int BMW_CHUNK_DEFAULT = 17;  // chunk extent when the windows' extent is not known to the host

// LDS doubles of one workgroup: A tile, B window of one chunk, two T tiles; k_block_match's at CU = 2U+1, CV = 2V+1
static size_t bmw_lds_doubles(int TN, int CU, int CV, int ft)
{
    const size_t AH = BMW_TM + 2 * ft, AW = TN + 2 * ft;
    return AH * AW + (AH + CU - 1) * (AW + CV - 1) + 2 * (size_t)BMW_TM * AW;
}

// win (M x N x 4 x H) or, when null, the box cbox at every pixel and rank.  flow, curv (M x N x 2 x H), cost (M x N x H)
// and pick (per rank the planes du, dv) may each be null; stats (null or two counters): displacements evaluated in the
// first walk summed over the tiles, and the pixels' box areas summed, both over the ranks.  Without RANKED there is
// one rank, the arrays have no rank axis, and H and sep are not read.  H and sep stand last: in front of the pointers
// they move the other arguments in the kernel's argument block, and the plain instantiations then reload 96 more
// scalars from spill lanes at TN = 32 (profiles/block_match_window_unified_times.txt).
template <int NPT, bool REFINE, bool RANKED>
__global__ __launch_bounds__(BMW_THREADS) void k_block_match_window(
    const double *__restrict__ A, const double *__restrict__ B, const int *__restrict__ win, int4 cbox, int M, int N,
    int ft, BmFilter f, int tiles_m, int CU, int CV, double *__restrict__ flow, double *__restrict__ cost,
    double *__restrict__ curv, int *__restrict__ pick, unsigned long long *__restrict__ stats, int H, int sep)
{
    extern __shared__ double bmw_lds[];
    __shared__ int un[4], vote[3];
    constexpr int TN = BMW_GROUPS * NPT;
    const int AH = BMW_TM + 2 * ft, AW = TN + 2 * ft, BH = AH + CU - 1, BW = AW + CV - 1;
    double *As = bmw_lds, *Bs = As + AH * AW, *Ts = Bs + BH * BW;
    const int tid = threadIdx.x;
    const int m0 = (int)(blockIdx.x % tiles_m) * BMW_TM, n0 = (int)(blockIdx.x / tiles_m) * TN;
    const int lm = tid % BMW_TM, cg = tid / BMW_TM;
    const int gm = m0 + lm;
    const int64_t MN = (int64_t)M * N;

    for (int t = tid; t < AH * AW; t += BMW_THREADS) {
        const int am = m0 - ft + t % AH, an = n0 - ft + t / AH;
        As[t] = am >= 0 && am < M && an >= 0 && an < N ? A[am + (int64_t)M * an] : 0.0;
    }
    if (tid == 0) vote[0] = vote[1] = vote[2] = 0;
    // the keys of the three ranks before this one, the latest first; GQ_BM_NOPICK excludes nothing
    [[maybe_unused]] int prev[NPT][3];
    if constexpr (RANKED) {
#pragma unroll
        for (int k = 0; k < NPT; ++k) prev[k][0] = prev[k][1] = prev[k][2] = GQ_BM_NOPICK;
    }
    // T's buffer parity runs on a counter over the displacements evaluated, as in k_block_match, through all ranks;
    // every barrier below is reached by every lane, the branches around them are block-uniform
    unsigned done = 0;
    unsigned long long scanned = 0, area = 0;
    // The workgroup's OR of a flag in ONE barrier (__syncthreads_or takes three): the lanes that hold the flag store 1
    // into the slot of this vote, all read it after the barrier.  Three slots in rotation: lane 0 then clears the slot
    // read one vote ago -- every lane is past that read, having arrived at this barrier -- and it is written again
    // only in the vote after the next, behind the next barrier.
    int slot = 0;
    const auto any_lane = [&](bool flag) {
        if (flag) vote[slot] = 1;
        __syncthreads();
        const bool any = vote[slot] != 0;
        if (tid == 0) vote[slot == 0 ? 2 : slot - 1] = 0;
        slot = slot == 2 ? 0 : slot + 1;
        return any;
    };
    const int ranks = RANKED ? H : 1;
    for (int j = 0; j < ranks; ++j) {
        const int64_t jo = RANKED ? MN * j : 0;  // rank j's plane of a one-plane array
        // later ranks: every lane has read the union box of the rank before and is past its last column pass, so un,
        // Bs and T are free.  At rank 0 nothing has read un yet.
        if (j > 0) __syncthreads();
        if (tid == 0) {
            un[0] = un[2] = GQ_BM_NOPICK;
            un[1] = un[3] = -GQ_BM_NOPICK;
        }
        // box j of this lane's output pixels; a pixel outside the frame has the empty box
        const int *wj = win ? win + 4 * jo : nullptr;
        int box[NPT][4];
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
            const int gn = n0 + cg + BMW_GROUPS * k;
            const bool inside = gm < M && gn < N;
            const int64_t o = gm + (int64_t)M * gn;
            box[k][0] = !inside ? 1 : wj ? wj[o] : cbox.x;
            box[k][1] = !inside ? 0 : wj ? wj[o + MN] : cbox.y;
            box[k][2] = !inside ? 1 : wj ? wj[o + 2 * MN] : cbox.z;
            box[k][3] = !inside ? 0 : wj ? wj[o + 3 * MN] : cbox.w;
        }
        __syncthreads();  // un is reset; at rank 0 the A tile and the vote slots are written too
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
                    const bool w = pass != 0 ? bm_near_wanted(box[k], du, dv, key[k])
                                             : bm_in_box(box[k], du, dv) &&
                                                   (!RANKED || (bm_far_key(du, dv, prev[k][0], sep) &&
                                                                bm_far_key(du, dv, prev[k][1], sep) &&
                                                                bm_far_key(du, dv, prev[k][2], sep)));
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
                    for (int t = tid; t < h * w; t += BMW_THREADS) {
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
                        double *T = Ts + (done & 1u) * (BMW_TM * AW);
                        if (go)
                            for (int c = cg; c < AW; c += BMW_GROUPS) {
                                const int gn = n0 - ft + c;
                                T[lm + BMW_TM * c] = bm_rows(As + lm + AH * c, Bs + (lm + du - cu0) + BH * (c + dv - cv0),
                                                            ft, f, m0 + lm - ft, M, gn >= 0 && gn < N);
                            }
                        const bool next = any_lane(nmask != 0);
                        if (go) {
#pragma unroll
                            for (int k = 0; k < NPT; ++k) {
                                const double c = bm_cols(T + lm + BMW_TM * (cg + BMW_GROUPS * k), BMW_TM, ft, f);
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
            const int gn = n0 + cg + BMW_GROUPS * k;
            if (gm < M && gn < N) {
                const int64_t o = gm + (int64_t)M * gn, o2 = o + 2 * jo;  // in a one-plane and a two-plane array
                double out[4];
                if constexpr (REFINE) {
                    bm_refined_window(key[k], best[k], nbr[k], box[k], true, out);
                } else {
                    BmNear none;
                    bm_near_clear(none);
                    bm_refined_window(key[k], best[k], none, box[k], false, out);
                }
                if (flow) {
                    flow[o2] = out[0];
                    flow[o2 + MN] = out[1];
                }
                if (cost) cost[o + jo] = best[k];
                if (curv) {
                    curv[o2] = out[2];
                    curv[o2 + MN] = out[3];
                }
                if (pick) {
                    const bool found = key[k] != GQ_BM_NOPICK;
                    pick[o2] = found ? bm_key_du(key[k]) : GQ_BM_NOPICK;
                    pick[o2 + MN] = found ? bm_key_dv(key[k]) : GQ_BM_NOPICK;
                }
            }
            if constexpr (RANKED) {
                prev[k][2] = prev[k][1];
                prev[k][1] = prev[k][0];
                prev[k][0] = key[k];
            }
        }
    }
    if (stats) {
        if (tid == 0) atomicAdd(&stats[0], scanned);
        if (area) atomicAdd(&stats[1], area);
    }
}

__global__ __launch_bounds__(256) void k_bm_half(const double *__restrict__ P, int M, int N, double *__restrict__ out,
                                                 int Mh, int Nh)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
    if (i < Mh && j < Nh) out[i + (int64_t)Mh * j] = bm_half(P, M, N, i, j);
}

__global__ __launch_bounds__(256) void k_bm_window_up(const int *__restrict__ pick, int Mc, int Nc, int M, int N, int r,
                                                      int k, int *__restrict__ win)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x, n = blockIdx.y;
    if (m < M && n < N) {
        int box[4];
        bm_window_up(pick, Mc, Nc, m, n, r, k, box);
        const int64_t o = m + (int64_t)M * n, MN = (int64_t)M * N;
#pragma unroll
        for (int q = 0; q < 4; ++q) win[o + MN * q] = box[q];
    }
}

// tile width by the rule of bm_choose_cols (gqmap_blockmatch.hip): the widest that keeps 4 workgroups per CU
static int bmw_choose_cols(int M, int N, int CU, int CV, int ft, int cus)
{
    const double lds_cu = 160.0 * 1024, tiles_m = (M + BMW_TM - 1) / BMW_TM;
    int cols = 8;
    double most = -1;
    for (int tn = 32; tn >= 8; tn /= 2) {
        const double by_lds = std::floor(lds_cu / (bmw_lds_doubles(tn, CU, CV, ft) * sizeof(double)));
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

// chunk extent forced by gqmap_debug_block_match_chunk (0: chosen), and the counters of the last call
static int g_bmw_cu = 0, g_bmw_cv = 0;
static bool g_bmw_stats = false;
static double g_bmw_last[GQ_BM_LEVELS][5];

// H = 0: plain, the RANKED = false instantiations and arrays without a rank axis; H >= 1 runs the ranked ones, H = 1 too
template <int NPT>
static hipError_t bmw_launch(const double *dA, const double *dB, const int *dwin, int4 cbox, int M, int N, int ft,
                             const BmFilter &f, bool refine, int CU, int CV, int H, int sep, double *dflow,
                             double *dcost, double *dcurv, int *dpick, unsigned long long *dstats, hipStream_t s)
{
    constexpr int TN = BMW_GROUPS * NPT;
    const auto kernel = H ? (refine ? &k_block_match_window<NPT, true, true> : &k_block_match_window<NPT, false, true>)
                          : (refine ? &k_block_match_window<NPT, true, false> : &k_block_match_window<NPT, false, false>);
    const size_t bytes = bmw_lds_doubles(TN, CU, CV, ft) * sizeof(double);
    // above 64 KB (up to 117 KB at CU = CV = 65, ft = 4, TN = 32) the dynamic LDS limit must be raised
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return e;
    const int tiles_m = (M + BMW_TM - 1) / BMW_TM, tiles_n = (N + TN - 1) / TN;
    const dim3 grid((unsigned)((int64_t)tiles_m * tiles_n)), block(BMW_THREADS);
    kernel<<<grid, block, bytes, s>>>(dA, dB, dwin, cbox, M, N, ft, f, tiles_m, CU, CV, dflow, dcost, dcurv, dpick,
                                      dstats, H, sep);
    return hipGetLastError();
}

// one level on the device.  ext_u, ext_v: the largest extent of a box when the host knows it, else 0.
static hipError_t bmw_level(const double *dA, const double *dB, const int *dwin, int4 cbox, int M, int N, int ft,
                            const BmFilter &f, bool refine, int ext_u, int ext_v, int cus, int H, int sep,
                            double *dflow, double *dcost, double *dcurv, int *dpick, unsigned long long *dstats,
                            int *tiles)
{
    const auto extent = [](int forced, int ext) {
        return forced ? forced : std::min(GQ_BM_CHUNK, std::max(BMW_CHUNK_DEFAULT, ext));
    };
    const int CU = extent(g_bmw_cu, ext_u), CV = extent(g_bmw_cv, ext_v);
    int cols = bm_forced_cols();
    if (cols == 0) cols = bmw_choose_cols(M, N, CU, CV, ft, cus);
    *tiles = ((M + BMW_TM - 1) / BMW_TM) * ((N + cols - 1) / cols);
    const auto launch = cols == 32 ? &bmw_launch<4> : cols == 16 ? &bmw_launch<2> : &bmw_launch<1>;
    return launch(dA, dB, dwin, cbox, M, N, ft, f, refine, CU, CV, H, sep, dflow, dcost, dcurv, dpick, dstats, 0);
}

}  // namespace gq

using namespace gq;

namespace {
// the tile count of the narrowest tile fits the grid
bool bmw_grid_fits(int M, int N) { return (int64_t)((M + BMW_TM - 1) / BMW_TM) * ((N + 7) / 8) <= 0x7fffffff; }

// gqmap_block_match_window[_multi] (win given, levels = 1) and gqmap_block_match_pyramid[_multi] (win null) behind one
// body; H = 0: the plain entry points, one rank and no rank axis
gqmap_status bmw_device(const char *who, const double *A, const double *B, const int *win, int M, int N, int U, int V,
                        int ft, double sigma, int levels, int r, int k, int H, int sep, bool subpixel, double *flow,
                        double *cost, double *curv, double *elapsed_ms, int device)
{
    GQ_CHECK(bmw_grid_fits(M, N), GQMAP_ERR_INVALID_ARG, "%s: %dx%d has too many tiles", who, M, N);
    GQ_CHECK(gqmap_device_count() > device && device >= 0, GQMAP_ERR_NO_DEVICE, "no HIP device %d", device);
    DeviceGuard dg(device);
    const BmFilter f = bm_filter(ft, sigma);
    int cus = 0;
    GQ_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    const int c = levels - 1;
    std::vector<int> Ms(levels, M), Ns(levels, N), tiles(levels, 0);
    for (int l = 1; l < levels; ++l) Ms[l] = (Ms[l - 1] + 1) / 2, Ns[l] = (Ns[l - 1] + 1) / 2;
    const size_t ranks = H ? (size_t)H : 1;
    // the largest extent of a box over all ranks, where the host has the windows
    int ext_u = 0, ext_v = 0;
    if (win) {
        const size_t MN = (size_t)M * N;
        for (size_t j = 0; j < ranks; ++j)
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
        if (l < c || win) GQ_HIP(hipMalloc(&dwin[l].p, sizeof(int) * 4 * mn * ranks));
        if (l > 0) GQ_HIP(hipMalloc(&dpick[l].p, sizeof(int) * 2 * mn * ranks));
    }
    GQ_HIP(hipMalloc(&dflow.p, 2 * bytes * ranks));
    if (cost) GQ_HIP(hipMalloc(&dcost.p, bytes * ranks));
    if (curv) GQ_HIP(hipMalloc(&dcurv.p, 2 * bytes * ranks));
    if (g_bmw_stats) {
        GQ_HIP(hipMalloc(&dstats.p, sizeof(unsigned long long) * 2 * GQ_BM_LEVELS));
        GQ_HIP(hipMemset(dstats.p, 0, sizeof(unsigned long long) * 2 * GQ_BM_LEVELS));
    }
    GQ_HIP(hipMemcpy(dA[0].p, A, bytes, hipMemcpyHostToDevice));
    GQ_HIP(hipMemcpy(dB[0].p, B, bytes, hipMemcpyHostToDevice));
    if (win) GQ_HIP(hipMemcpy(dwin[0].p, win, sizeof(int) * 4 * (size_t)M * N * ranks, hipMemcpyHostToDevice));
    if (elapsed_ms) {
        GQ_HIP(hipEventCreate(&ev.a));
        GQ_HIP(hipEventCreate(&ev.b));
        GQ_HIP(hipEventRecord(ev.a, 0));
    }
    for (int l = 1; l < levels; ++l) {
        const dim3 grid((unsigned)((Ms[l] + 255) / 256), (unsigned)Ns[l]);
        k_bm_half<<<grid, 256>>>((const double *)dA[l - 1].p, Ms[l - 1], Ns[l - 1], (double *)dA[l].p, Ms[l], Ns[l]);
        k_bm_half<<<grid, 256>>>((const double *)dB[l - 1].p, Ms[l - 1], Ns[l - 1], (double *)dB[l].p, Ms[l], Ns[l]);
        GQ_HIP(hipGetLastError());
    }
    const int Uc = bm_ceil_shift(U, c), Vc = bm_ceil_shift(V, c);
    if (g_bmw_stats) {  // counting only: an event before each level's kernels and one after the last
        ev.more.assign(levels + 1, nullptr);
        for (int l = 0; l <= levels; ++l) GQ_HIP(hipEventCreate(&ev.more[l]));
    }
    for (int l = c; l >= 0; --l) {
        const bool coarsest = l == c && !win;
        if (g_bmw_stats) GQ_HIP(hipEventRecord(ev.more[l + 1], 0));
        if (l < c) {
            const dim3 grid((unsigned)((Ms[l] + 255) / 256), (unsigned)Ns[l]);
            const size_t mn = (size_t)Ms[l] * Ns[l], mnc = (size_t)Ms[l + 1] * Ns[l + 1];
            for (size_t j = 0; j < ranks; ++j)  // box j from the coarse level's rank-j pick planes
                k_bm_window_up<<<grid, 256>>>((const int *)dpick[l + 1].p + 2 * mnc * j, Ms[l + 1], Ns[l + 1], Ms[l],
                                              Ns[l], r, k, (int *)dwin[l].p + 4 * mn * j);
            GQ_HIP(hipGetLastError());
        }
        unsigned long long *st = g_bmw_stats ? (unsigned long long *)dstats.p + 2 * l : nullptr;
        GQ_HIP(bmw_level((const double *)dA[l].p, (const double *)dB[l].p, coarsest ? nullptr : (const int *)dwin[l].p,
                         make_int4(-Uc, Uc, -Vc, Vc), Ms[l], Ns[l], ft, f, l == 0 && subpixel,
                         coarsest ? 2 * Uc + 1 : ext_u, coarsest ? 2 * Vc + 1 : ext_v, cus, H, sep,
                         l == 0 ? (double *)dflow.p : nullptr, l == 0 ? (double *)dcost.p : nullptr,
                         l == 0 ? (double *)dcurv.p : nullptr, l > 0 ? (int *)dpick[l].p : nullptr, st, &tiles[l]));
    }
    if (g_bmw_stats) GQ_HIP(hipEventRecord(ev.more[0], 0));
    if (elapsed_ms) {
        float ms = 0;
        GQ_HIP(hipEventRecord(ev.b, 0));
        GQ_HIP(hipEventSynchronize(ev.b));
        GQ_HIP(hipEventElapsedTime(&ms, ev.a, ev.b));
        *elapsed_ms = ms;
    }
    GQ_HIP(hipMemcpy(flow, dflow.p, 2 * bytes * ranks, hipMemcpyDeviceToHost));
    if (cost) GQ_HIP(hipMemcpy(cost, dcost.p, bytes * ranks, hipMemcpyDeviceToHost));
    if (curv) GQ_HIP(hipMemcpy(curv, dcurv.p, 2 * bytes * ranks, hipMemcpyDeviceToHost));
    if (g_bmw_stats) {
        unsigned long long st[2 * GQ_BM_LEVELS];
        GQ_HIP(hipMemcpy(st, dstats.p, sizeof st, hipMemcpyDeviceToHost));
        for (int l = 0; l < GQ_BM_LEVELS; ++l) {
            const bool on = l < levels;
            float ms = 0;
            if (on) GQ_HIP(hipEventElapsedTime(&ms, ev.more[l + 1], ev.more[l]));
            g_bmw_last[l][4] = ms;
            g_bmw_last[l][0] = on ? (double)Ms[l] * Ns[l] : 0.0;
            g_bmw_last[l][1] = on ? (double)tiles[l] : 0.0;
            g_bmw_last[l][2] = on ? (double)st[2 * l] : 0.0;
            g_bmw_last[l][3] = on ? (double)st[2 * l + 1] : 0.0;
        }
    }
    return GQMAP_OK;
}
}  // namespace

extern "C" {

// Not in the public header (tests): force the chunk extent (displacements per axis of one staged B window) to cu x cv,
// each in [1, 65]; 0 restores the choice.  Never changes a result.
int gqmap_debug_block_match_chunk(int cu, int cv)
{
    if (cu < 0 || cu > GQ_BM_CHUNK || cv < 0 || cv > GQ_BM_CHUNK) return -1;
    g_bmw_cu = cu;
    g_bmw_cv = cv;
    return 0;
}

// Not in the public header (scripts): count while on; out = GQ_BM_LEVELS x 5 doubles of the last device call, per level
// pixels, tiles, displacements evaluated in the first walk summed over the tiles, box areas summed over the pixels, and
// the time of the level's kernels in ms (the window rule and the matcher; the halving kernels are not in it)
int gqmap_debug_block_match_stats(int on, double *out)
{
    g_bmw_stats = on != 0;
    if (out)
        for (int l = 0; l < GQ_BM_LEVELS; ++l)
            for (int q = 0; q < 5; ++q) out[5 * l + q] = g_bmw_last[l][q];
    return 0;
}

gqmap_status gqmap_block_match_window(const double *A, const double *B, const int *win, int M, int N, int ft,
                                      double sigma, int subpixel, double *flow, double *cost, double *curv,
                                      double *elapsed_ms, int device)
{
    clear_error();
    GQ_CHECK(A && B && win && flow, GQMAP_ERR_INVALID_ARG, "gqmap_block_match_window: null argument");
    const char *bad = bm_bad_window(M, N, ft, sigma);
    GQ_CHECK(!bad, GQMAP_ERR_INVALID_ARG, "gqmap_block_match_window: %s (M=%d N=%d ft=%d sigma=%g)", bad, M, N, ft,
             sigma);
    GQ_CHECK(!bm_bad_bounds(win, M, N), GQMAP_ERR_INVALID_ARG, "gqmap_block_match_window: a window bound outside [-%d,%d]",
             GQ_BM_DMAX, GQ_BM_DMAX);
    return bmw_device("gqmap_block_match_window", A, B, win, M, N, 0, 0, ft, sigma, 1, 0, 0, 0, 0, subpixel != 0, flow,
                      cost, curv, elapsed_ms, device);
}

gqmap_status gqmap_block_match_pyramid(const double *A, const double *B, int M, int N, int U, int V, int ft,
                                       double sigma, int levels, int r, int k, int subpixel, double *flow, double *cost,
                                       double *curv, double *elapsed_ms, int device)
{
    clear_error();
    GQ_CHECK(A && B && flow, GQMAP_ERR_INVALID_ARG, "gqmap_block_match_pyramid: null argument");
    const char *bad = bm_bad_pyramid(M, N, U, V, ft, sigma, levels, r, k);
    GQ_CHECK(!bad, GQMAP_ERR_INVALID_ARG,
             "gqmap_block_match_pyramid: %s (M=%d N=%d U=%d V=%d ft=%d sigma=%g levels=%d r=%d k=%d)", bad, M, N, U, V, ft,
             sigma, levels, r, k);
    return bmw_device("gqmap_block_match_pyramid", A, B, nullptr, M, N, U, V, ft, sigma, levels, r, k, 0, 0,
                      subpixel != 0, flow, cost, curv, elapsed_ms, device);
}

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
    return bmw_device("gqmap_block_match_window_multi", A, B, win, M, N, 0, 0, ft, sigma, 1, 0, 0, H, sep, subpixel != 0,
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
    return bmw_device("gqmap_block_match_pyramid_multi", A, B, nullptr, M, N, U, V, ft, sigma, levels, r, k, H, sep,
                      subpixel != 0, flow, cost, curv, elapsed_ms, device);
}

}  // extern "C"
