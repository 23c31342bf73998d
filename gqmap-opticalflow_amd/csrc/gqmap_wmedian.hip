// Weighted median filter on the device.  The arithmetic is gqmap_wmedian.h
// (shared with the host model gqmap_flow_wmedian_host); this file is the tiling
// and the selection.
//
// One launch is one pass.  One workgroup of 256 lanes owns a 16 x 16 output
// tile and stages the (16 + 2r)^2 tile around it in LDS: the keys of both flow
// planes, the guide and the confidence (1.0 without a map, 0.0 outside the
// frame, so that nothing out there has a weight), 32 W^2 bytes with
// W = 16 + 2r, 32,768 B at r = 8.  The weight of an entry costs two divisions,
// so wq is computed once per pixel and shared by the two planes.  The selection
// is a rank count over the n = (2r+1)^2 entries: entry i sums the live wq_j with
// key_j <= key_i, and the answer is the smallest live key whose sum reaches half
// of the total.  The sums are exact integers, so no order shows.  Two shapes:
//
//   k_flow_wmedian_lane<R>  r = R <= 2 (n <= 25): a lane per pixel, the window's
//                 keys and weights in registers, both loops unrolled: 3 n^2
//                 instructions per pixel and plane, nothing crosses lanes.
//   k_flow_wmedian<NE>      r >= 3: a wave per pixel, 64 pixels in turn; a lane
//                 holds the entries lane, lane + 64, ... (NE = ceil(n / 64) of
//                 them, 1..5) in registers.  Every entry j is broadcast by
//                 v_readlane (three of them: key and wq) and each lane adds wq_j
//                 to the sums of its own entries; the minimum over the wave is
//                 taken by __shfl_xor.  n (3 + 3 NE) instructions per pixel and
//                 plane, against the 64 steps of ~5 NE + 18 of a radix
//                 selection: fewer up to r = 6, about 1.9x as many at r = 8.
//                 The results go through a 4 KB LDS buffer so that the stores
//                 run along m.
// Eight instantiations (R = 0, 1, 2; NE = 1..5).  No scratch, no atomics.
// Passes ping-pong two flow buffers on one stream, one launch per pass.
// Lanes run along m (the fastest index) in the staging loads and the stores.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "gqmap_internal.h"
#include "gqmap_wmedian.h"

namespace gq {

constexpr int WM_S = 16;  // output tile rows = columns
constexpr int WM_THREADS = 256;
constexpr int WM_LANE_RMAX = 2;  // up to here a lane holds a whole window

static size_t wm_lds_bytes(int r)
{
    const size_t W = WM_S + 2 * (size_t)r;
    return 4 * sizeof(double) * W * W;
}

// The tile of a workgroup in LDS: cell c = lm + W ln is the frame pixel (m0 - r + lm, n0 - r + ln).
struct WmTile {
    unsigned long long *K0, *K1;  // keys of the two planes
    double *Gd, *Cf;              // guide, confidence
};

__device__ __forceinline__ WmTile wm_stage(unsigned long long *lds, const double *__restrict__ fin,
                                           const double *__restrict__ guide, const double *__restrict__ conf, int M,
                                           int N, int m0, int n0, int r)
{
    const int W = WM_S + 2 * r, CELLS = W * W;
    const int64_t MN = (int64_t)M * N;
    WmTile t;
    t.K0 = lds;
    t.K1 = t.K0 + CELLS;
    t.Gd = reinterpret_cast<double *>(t.K1 + CELLS);
    t.Cf = t.Gd + CELLS;
    for (int c = threadIdx.x; c < CELLS; c += WM_THREADS) {
        const int lm = c % W, ln = c / W, gm = m0 - r + lm, gn = n0 - r + ln;
        const bool in = gm >= 0 && gm < M && gn >= 0 && gn < N;
        const int64_t o = gm + (int64_t)M * gn;
        t.K0[c] = in ? wm_key((uint64_t)__double_as_longlong(fin[o])) : 0ull;
        t.K1[c] = in ? wm_key((uint64_t)__double_as_longlong(fin[o + MN])) : 0ull;
        t.Gd[c] = in ? guide[o] : 0.0;
        t.Cf[c] = in ? (conf ? conf[o] : 1.0) : 0.0;
    }
    return t;
}

template <int R>
__global__ __launch_bounds__(WM_THREADS) void k_flow_wmedian_lane(const double *__restrict__ fin,
                                                                  const double *__restrict__ guide,
                                                                  const double *__restrict__ conf,
                                                                  double *__restrict__ fout, int M, int N,
                                                                  int tiles_m, double sigma_c, WmFilter f)
{
    constexpr int W = WM_S + 2 * R, D = 2 * R + 1, NN = D * D;
    extern __shared__ __align__(16) unsigned long long wm_lds[];
    const int tid = threadIdx.x;
    const int m0 = (int)(blockIdx.x % tiles_m) * WM_S, n0 = (int)(blockIdx.x / tiles_m) * WM_S;
    const WmTile t = wm_stage(wm_lds, fin, guide, conf, M, N, m0, n0, R);
    __syncthreads();

    // the window of tile pixel (lm, ln) starts at the tile cell (lm, ln)
    const int base = tid % WM_S + W * (tid / WM_S), centre = base + R + W * R;
    const double gc = t.Gd[centre];
    unsigned wq[NN];
#pragma unroll
    for (int e = 0; e < NN; ++e) {
        const int cell = base + e % D + W * (e / D);
        wq[e] = wm_wq(f.s[e % D] * f.s[e / D], t.Gd[cell], gc, sigma_c, t.Cf[cell]);
    }
    unsigned long long out[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const unsigned long long *K = c == 0 ? t.K0 : t.K1;
        unsigned long long key[NN];
        unsigned wl[NN], total = 0;
#pragma unroll
        for (int e = 0; e < NN; ++e) {
            key[e] = K[base + e % D + W * (e / D)];
            wl[e] = wm_key_nan(key[e]) ? 0u : wq[e];
            total += wl[e];
        }
        // the smallest live key whose sum reaches half of the total; ~0 is a NaN's key and never live
        unsigned long long best = ~0ull;
#pragma unroll
        for (int i = 0; i < NN; ++i) {
            unsigned cum = 0;
#pragma unroll
            for (int j = 0; j < NN; ++j) cum += key[j] <= key[i] ? wl[j] : 0u;
            if (wl[i] > 0u && 2u * cum >= total && key[i] < best) best = key[i];
        }
        out[c] = total == 0u ? K[centre] : best;
    }
    const int gm = m0 + tid % WM_S, gn = n0 + tid / WM_S;
    if (gm < M && gn < N) {
        const int64_t o = gm + (int64_t)M * gn;
        fout[o] = __longlong_as_double((long long)wm_unkey(out[0]));
        fout[o + (int64_t)M * N] = __longlong_as_double((long long)wm_unkey(out[1]));
    }
}

// the value of lane j of the wave (j the same in every lane)
__device__ __forceinline__ unsigned wm_bcast(unsigned v, int j) { return (unsigned)__builtin_amdgcn_readlane((int)v, j); }

template <int NE>
__global__ __launch_bounds__(WM_THREADS) void k_flow_wmedian(const double *__restrict__ fin,
                                                             const double *__restrict__ guide,
                                                             const double *__restrict__ conf,
                                                             double *__restrict__ fout, int M, int N, int tiles_m,
                                                             int r, double sigma_c, WmFilter f)
{
    extern __shared__ __align__(16) unsigned long long wm_lds[];
    __shared__ double s_tab[GQ_WM_TAPS];
    __shared__ unsigned long long res[2][WM_S * WM_S];
    const int W = WM_S + 2 * r, D = 2 * r + 1, n = D * D;  // 64 (NE - 1) < n <= 64 NE
    const int tid = threadIdx.x;
    const int m0 = (int)(blockIdx.x % tiles_m) * WM_S, n0 = (int)(blockIdx.x / tiles_m) * WM_S;
    if (tid < GQ_WM_TAPS) s_tab[tid] = f.s[tid];
    const WmTile t = wm_stage(wm_lds, fin, guide, conf, M, N, m0, n0, r);
    __syncthreads();

    // what a lane's entries are does not depend on the pixel: entry e is the window cell (e % D, e / D)
    const int lane = tid & 63;
    int off[NE];
    double ss[NE];
#pragma unroll
    for (int k = 0; k < NE; ++k) {
        const bool held = lane + k * 64 < n;
        const int e = held ? lane + k * 64 : 0, di = e % D, dj = e / D;  // a lane past the window reads cell 0, weight 0
        off[k] = di + W * dj;
        ss[k] = s_tab[di] * s_tab[dj];
    }

    for (int q = 0; q < 64; ++q) {
        // tile pixel p = lm + 16 ln; its window starts at the tile cell (lm, ln)
        const int p = (tid & ~63) + q;
        const int base = p % WM_S + W * (p / WM_S), centre = base + r + W * r;
        const double gc = t.Gd[centre];
        unsigned long long key[2][NE];
        unsigned wq[2][NE];
#pragma unroll
        for (int k = 0; k < NE; ++k) {
            const int cell = base + off[k];
            const unsigned w = lane + k * 64 < n ? wm_wq(ss[k], t.Gd[cell], gc, sigma_c, t.Cf[cell]) : 0u;
            key[0][k] = t.K0[cell];
            key[1][k] = t.K1[cell];
            wq[0][k] = wm_key_nan(key[0][k]) ? 0u : w;
            wq[1][k] = wm_key_nan(key[1][k]) ? 0u : w;
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            unsigned cum[NE], total = 0;
#pragma unroll
            for (int i = 0; i < NE; ++i) cum[i] = 0;
#pragma unroll
            for (int k = 0; k < NE; ++k) {
                const int count = k < NE - 1 ? 64 : n - k * 64;
                for (int j = 0; j < count; ++j) {
                    const unsigned wj = wm_bcast(wq[c][k], j);
                    const unsigned long long kj = (unsigned long long)wm_bcast((unsigned)(key[c][k] >> 32), j) << 32 |
                                                  wm_bcast((unsigned)key[c][k], j);
                    total += wj;
#pragma unroll
                    for (int i = 0; i < NE; ++i) cum[i] += kj <= key[c][i] ? wj : 0u;
                }
            }
            // the smallest live key whose sum reaches half of the total; ~0 is a NaN's key and never live
            unsigned long long best = ~0ull;
#pragma unroll
            for (int i = 0; i < NE; ++i)
                if (wq[c][i] > 0u && 2u * cum[i] >= total && key[c][i] < best) best = key[c][i];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long other = (unsigned long long)(unsigned)__shfl_xor((int)(best >> 32), o) << 32 |
                                                 (unsigned)__shfl_xor((int)(unsigned)best, o);
                best = other < best ? other : best;
            }
            if (lane == 0) res[c][p] = total == 0u ? (c == 0 ? t.K0[centre] : t.K1[centre]) : best;
        }
    }
    __syncthreads();

    const int gm = m0 + tid % WM_S, gn = n0 + tid / WM_S;
    if (gm < M && gn < N) {
        const int64_t o = gm + (int64_t)M * gn;
        fout[o] = __longlong_as_double((long long)wm_unkey(res[0][tid]));
        fout[o + (int64_t)M * N] = __longlong_as_double((long long)wm_unkey(res[1][tid]));
    }
}

}  // namespace gq

using namespace gq;

namespace {
// kernel time on the null stream (off: no events, no waits)
struct Stopwatch {
    hipEvent_t a = nullptr, b = nullptr;
    bool on = false;
    double ms = 0;
    ~Stopwatch()
    {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
    hipError_t init(bool enable)
    {
        on = enable;
        if (!on) return hipSuccess;
        hipError_t e = hipEventCreate(&a);
        return e != hipSuccess ? e : hipEventCreate(&b);
    }
    hipError_t begin() { return on ? hipEventRecord(a, 0) : hipSuccess; }
    hipError_t end()
    {
        if (!on) return hipSuccess;
        float t = 0;
        hipError_t e = hipEventRecord(b, 0);
        if (e == hipSuccess) e = hipEventSynchronize(b);
        if (e == hipSuccess) e = hipEventElapsedTime(&t, a, b);
        ms += t;
        return e;
    }
};

struct WmArgs {
    unsigned blocks;
    const double *fin, *guide, *conf;
    double *fout;
    int M, N, tiles_m, r;
    double sigma_c;
    WmFilter f;
};

template <int R>
void wm_launch_lane(const WmArgs &a)
{
    k_flow_wmedian_lane<R><<<dim3(a.blocks), dim3(WM_THREADS), wm_lds_bytes(R), 0>>>(a.fin, a.guide, a.conf, a.fout, a.M,
                                                                                   a.N, a.tiles_m, a.sigma_c, a.f);
}

template <int NE>
void wm_launch_wave(const WmArgs &a)
{
    k_flow_wmedian<NE><<<dim3(a.blocks), dim3(WM_THREADS), wm_lds_bytes(a.r), 0>>>(a.fin, a.guide, a.conf, a.fout, a.M, a.N,
                                                                                 a.tiles_m, a.r, a.sigma_c, a.f);
}

// one pass: a lane per pixel up to WM_LANE_RMAX, above it a wave per pixel with ceil(n / 64) entries per lane
void wm_launch(const WmArgs &a)
{
    static_assert(WM_LANE_RMAX == 2 && GQ_WM_RMAX == 8, "the instantiations below");
    const int n = (2 * a.r + 1) * (2 * a.r + 1);
    switch (a.r <= WM_LANE_RMAX ? -a.r : (n + 63) / 64) {
    case 0: return wm_launch_lane<0>(a);
    case -1: return wm_launch_lane<1>(a);
    case -2: return wm_launch_lane<2>(a);
    case 1: return wm_launch_wave<1>(a);
    case 2: return wm_launch_wave<2>(a);
    case 3: return wm_launch_wave<3>(a);
    case 4: return wm_launch_wave<4>(a);
    default: return wm_launch_wave<5>(a);
    }
}
}  // namespace

extern "C" {

// Not in the public header (tests, DESIGN): the output tile (rows = columns),
// the dynamic LDS bytes of one workgroup at radius r, and the entries a lane
// holds there (0: a lane per pixel, the whole window).
int gqmap_debug_flow_wmedian_tile(void) { return WM_S; }
int gqmap_debug_flow_wmedian_lds(int r) { return r < 0 || r > GQ_WM_RMAX ? -1 : (int)wm_lds_bytes(r); }
int gqmap_debug_flow_wmedian_entries(int r)
{
    return r < 0 || r > GQ_WM_RMAX ? -1 : r <= WM_LANE_RMAX ? 0 : ((2 * r + 1) * (2 * r + 1) + 63) / 64;
}

gqmap_status gqmap_flow_wmedian(const double *flow, const double *guide, const double *conf, int M, int N, int r,
                                double sigma_s, double sigma_c, int passes, double *out, double *elapsed_ms,
                                int device)
{
    clear_error();
    GQ_CHECK(flow && guide && out, GQMAP_ERR_INVALID_ARG, "gqmap_flow_wmedian: null argument");
    const char *bad = wm_bad(M, N, r, sigma_s, sigma_c, passes);
    GQ_CHECK(!bad, GQMAP_ERR_INVALID_ARG, "gqmap_flow_wmedian: %s (M=%d N=%d r=%d sigma_s=%g sigma_c=%g passes=%d)",
             bad, M, N, r, sigma_s, sigma_c, passes);
    const int tiles_m = (M + WM_S - 1) / WM_S, tiles_n = (N + WM_S - 1) / WM_S;
    GQ_CHECK((int64_t)tiles_m * tiles_n <= 0x7fffffff, GQMAP_ERR_INVALID_ARG,
             "gqmap_flow_wmedian: %dx%d has too many tiles", M, N);
    GQ_CHECK(gqmap_device_count() > device && device >= 0, GQMAP_ERR_NO_DEVICE, "no HIP device %d", device);
    DeviceGuard dg(device);
    const size_t MN = (size_t)M * N, bytes = sizeof(double) * 2 * MN;
    const WmFilter f = wm_filter(r, sigma_s);
    const unsigned blocks = (unsigned)((int64_t)tiles_m * tiles_n);

    DevBuf dFa, dFb, dG, dC;
    Stopwatch sw;
    GQ_HIP(hipMalloc(&dFa.p, bytes));
    GQ_HIP(hipMalloc(&dFb.p, bytes));
    GQ_HIP(hipMalloc(&dG.p, sizeof(double) * MN));
    if (conf) GQ_HIP(hipMalloc(&dC.p, sizeof(double) * MN));
    GQ_HIP(hipMemcpy(dFa.p, flow, bytes, hipMemcpyHostToDevice));
    GQ_HIP(hipMemcpy(dG.p, guide, sizeof(double) * MN, hipMemcpyHostToDevice));
    if (conf) GQ_HIP(hipMemcpy(dC.p, conf, sizeof(double) * MN, hipMemcpyHostToDevice));
    GQ_HIP(sw.init(elapsed_ms != nullptr));
    GQ_HIP(sw.begin());
    double *fcur = dFa.d(), *fnxt = dFb.d();
    for (int p = 1; p <= passes; ++p) {
        wm_launch(WmArgs{blocks, fcur, dG.d(), dC.d(), fnxt, M, N, tiles_m, r, sigma_c, f});
        GQ_HIP(hipGetLastError());
        std::swap(fcur, fnxt);
    }
    GQ_HIP(sw.end());
    GQ_HIP(hipMemcpy(out, fcur, bytes, hipMemcpyDeviceToHost));
    if (elapsed_ms) *elapsed_ms = sw.ms;
    return GQMAP_OK;
}

}  // extern "C"
