// Structure-texture preprocessing on the device (optical_flowSuper.m:7-14 with
// preprocessed = true): ROF decomposition by Chambolle's dual projection.  The
// arithmetic is gqmap_rof.h (shared with the host model
// gqmap_structure_texture_host); this file is the tiling.
//
// The hot path is n_iter Jacobi sweeps over p1, p2 of every plane; one sweep
// reaches one pixel in every direction.  Two forms, chosen by T (the iterations
// one launch runs), which never changes a result:
//   T = 1       k_rof_plain: one lane per pixel, p read from and written to
//               device memory (ping-pong), u of the three pixels a step needs
//               recomputed in registers.  No LDS, no barrier.
//   T = 2, 4, 8 k_rof_fused<T>: one workgroup of 256 lanes owns a 32 x 32
//               output tile and holds the (32 + 2T)^2 tile around it, x, p1,
//               p2 and u, in LDS: 4 (32 + 2T)^2 doubles = 32 (32 + 2T)^2 bytes,
//               73,728 B at T = 8.  It runs up to T iterations, two barriers
//               each (u, then p), and stores the inner 32 x 32.  An iteration
//               with R more to come updates only the cells the inner tile
//               still depends on, 32 + 2R on a side, so the halo shrinks by one
//               cell per iteration and no spoilt value is ever computed.
//               Where the frame edge falls inside the halo the frame's own
//               border rules hold (p = +0 outside, ix / iy = +0 in the last
//               column / row): those cells are exact like any other.  Tiles
//               overlap; there is no synchronisation between workgroups.
//               Planes are grid.y.
// Lanes run along m (the fastest index): global loads, stores and every LDS
// access are unit-stride 8-byte accesses over a wave.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "gqmap_internal.h"
#include "gqmap_rof.h"

namespace gq {

constexpr int ROF_S = 32;          // fused form: output tile rows = columns
constexpr int ROF_THREADS = 256;
constexpr int ROF_PM = 64, ROF_PN = 4;  // plain form: pixels of a workgroup (rows x columns)
constexpr int ROF_RED_BLOCKS = 1024;    // range reduction: at most this many partial triples
// Iterations per launch when nothing is forced: chosen from
// profiles/structure_texture_times.txt (DESIGN, structure-texture subsection).
constexpr int ROF_T_DEFAULT = 4;

static bool rof_legal_T(int T) { return T == 1 || T == 2 || T == 4 || T == 8; }
static size_t rof_lds_bytes(int T) { return 4 * sizeof(double) * (size_t)(ROF_S + 2 * T) * (ROF_S + 2 * T); }

// u(m, n) of an in-frame pixel from p in device memory
__device__ __forceinline__ double rof_u_at(const double *__restrict__ x, const double *__restrict__ p1,
                                           const double *__restrict__ p2, int m, int n, int M, double theta)
{
    const int64_t o = m + (int64_t)M * n;
    return rof_u(x[o], theta, rof_div(p1[o], n > 0 ? p1[o - M] : 0.0, p2[o], m > 0 ? p2[o - 1] : 0.0));
}

__global__ __launch_bounds__(ROF_THREADS) void k_rof_plain(const double *__restrict__ x,
                                                           const double *__restrict__ p1in,
                                                           const double *__restrict__ p2in,
                                                           double *__restrict__ p1out, double *__restrict__ p2out,
                                                           int M, int N, int tiles_m, double theta, double delta)
{
    const int64_t plane = (int64_t)M * N * blockIdx.y;
    const int m = (int)(blockIdx.x % tiles_m) * ROF_PM + (int)threadIdx.x % ROF_PM;
    const int n = (int)(blockIdx.x / tiles_m) * ROF_PN + (int)threadIdx.x / ROF_PM;
    if (m >= M || n >= N) return;
    x += plane, p1in += plane, p2in += plane;
    const int64_t o = m + (int64_t)M * n;
    const double u = rof_u_at(x, p1in, p2in, m, n, M, theta);
    const double ix = n < N - 1 ? rof_u_at(x, p1in, p2in, m, n + 1, M, theta) - u : 0.0;
    const double iy = m < M - 1 ? rof_u_at(x, p1in, p2in, m + 1, n, M, theta) - u : 0.0;
    double a1 = p1in[o], a2 = p2in[o];
    rof_step(a1, a2, ix, iy, delta);
    p1out[plane + o] = a1;
    p2out[plane + o] = a2;
}

// One iteration on the LDS tile of side W = 32 + 2T, with R iterations still to
// come after it: the new p is needed on the inner 32 x 32 widened by R cells
// (side A = 32 + 2R, origin O = T - R >= 1), u one column and one row beyond
// (ix, iy read right and down), the old p one beyond that to the left and
// up.  Every cell computed is exact, so nothing spoilt ever exists in the tile.
template <int T, int R>
__device__ __forceinline__ void rof_tile_iteration(const double *X, double *P1, double *P2, double *U, int tid,
                                                   int m0, int n0, int M, int N, double theta, double delta)
{
    constexpr int W = ROF_S + 2 * T, A = ROF_S + 2 * R, O = T - R;
    for (int i = tid; i < (A + 1) * (A + 1); i += ROF_THREADS) {
        const int c = O + i % (A + 1) + W * (O + i / (A + 1));
        U[c] = rof_u(X[c], theta, rof_div(P1[c], P1[c - W], P2[c], P2[c - 1]));
    }
    __syncthreads();
    for (int i = tid; i < A * A; i += ROF_THREADS) {
        const int lm = O + i % A, ln = O + i / A, c = lm + W * ln, gm = m0 + lm, gn = n0 + ln;
        // cells outside the frame keep p = +0
        if (gm >= 0 && gm < M && gn >= 0 && gn < N) {
            const double u = U[c];
            const double ix = gn < N - 1 ? U[c + W] - u : 0.0;
            const double iy = gm < M - 1 ? U[c + 1] - u : 0.0;
            double a1 = P1[c], a2 = P2[c];
            rof_step(a1, a2, ix, iy, delta);
            P1[c] = a1;
            P2[c] = a2;
        }
    }
    __syncthreads();
}

// the last `iters` of the iterations R = T-1 .. 0 (iters is uniform over the workgroup)
template <int T, int R>
__device__ __forceinline__ void rof_tile_run(const double *X, double *P1, double *P2, double *U, int tid, int m0,
                                             int n0, int M, int N, double theta, double delta, int iters)
{
    if (R < iters) rof_tile_iteration<T, R>(X, P1, P2, U, tid, m0, n0, M, N, theta, delta);
    if constexpr (R > 0) rof_tile_run<T, R - 1>(X, P1, P2, U, tid, m0, n0, M, N, theta, delta, iters);
}

template <int T>
__global__ __launch_bounds__(ROF_THREADS) void k_rof_fused(const double *__restrict__ x,
                                                           const double *__restrict__ p1in,
                                                           const double *__restrict__ p2in,
                                                           double *__restrict__ p1out, double *__restrict__ p2out,
                                                           int M, int N, int tiles_m, double theta, double delta,
                                                           int iters)
{
    constexpr int W = ROF_S + 2 * T, CELLS = W * W;
    extern __shared__ __align__(16) double rof_lds[];
    double *X = rof_lds, *P1 = X + CELLS, *P2 = P1 + CELLS, *U = P2 + CELLS;
    const int tid = threadIdx.x;
    const int64_t plane = (int64_t)M * N * blockIdx.y;
    const int m0 = (int)(blockIdx.x % tiles_m) * ROF_S - T, n0 = (int)(blockIdx.x / tiles_m) * ROF_S - T;
    x += plane, p1in += plane, p2in += plane;

    // tile cell c -> (lm, ln) = (c % W, c / W), frame pixel (m0 + lm, n0 + ln); +0 outside the frame
    for (int c = tid; c < CELLS; c += ROF_THREADS) {
        const int gm = m0 + c % W, gn = n0 + c / W;
        const bool in = gm >= 0 && gm < M && gn >= 0 && gn < N;
        const int64_t o = gm + (int64_t)M * gn;
        X[c] = in ? x[o] : 0.0;
        P1[c] = in ? p1in[o] : 0.0;
        P2[c] = in ? p2in[o] : 0.0;
    }
    __syncthreads();

    rof_tile_run<T, T - 1>(X, P1, P2, U, tid, m0, n0, M, N, theta, delta, iters);

    // the inner 32 x 32 in the frame, unit stride along m
    for (int c = tid; c < ROF_S * ROF_S; c += ROF_THREADS) {
        const int lm = T + c % ROF_S, ln = T + c / ROF_S, gm = m0 + lm, gn = n0 + ln;
        if (gm < M && gn < N) {
            const int64_t o = plane + gm + (int64_t)M * gn;
            p1out[o] = P1[lm + W * ln];
            p2out[o] = P2[lm + W * ln];
        }
    }
}

// s = x + theta*d of the final p, t = x - alp*s  (s may be null)
__global__ __launch_bounds__(ROF_THREADS) void k_rof_finish(const double *__restrict__ x,
                                                            const double *__restrict__ p1,
                                                            const double *__restrict__ p2, int M, int N,
                                                            int tiles_m, double theta, double alp,
                                                            double *__restrict__ t, double *__restrict__ s)
{
    const int64_t plane = (int64_t)M * N * blockIdx.y;
    const int m = (int)(blockIdx.x % tiles_m) * ROF_PM + (int)threadIdx.x % ROF_PM;
    const int n = (int)(blockIdx.x / tiles_m) * ROF_PN + (int)threadIdx.x / ROF_PM;
    if (m >= M || n >= N) return;
    const int64_t o = plane + m + (int64_t)M * n;
    const double sv = rof_u_at(x + plane, p1 + plane, p2 + plane, m, n, M, theta);
    t[o] = rof_t(x[o], alp, sv);
    if (s) s[o] = sv;
}

__global__ __launch_bounds__(ROF_THREADS) void k_rof_scale_in(const double *__restrict__ im, double *__restrict__ x,
                                                              int64_t n, double lo, double hi)
{
    for (int64_t i = blockIdx.x * (int64_t)ROF_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * ROF_THREADS)
        x[i] = rof_scale_in(im[i], lo, hi);
}

__global__ __launch_bounds__(ROF_THREADS) void k_rof_scale_out(double *__restrict__ t, int64_t n, double tlo,
                                                               double thi)
{
    for (int64_t i = blockIdx.x * (int64_t)ROF_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * ROF_THREADS)
        t[i] = rof_scale_out(t[i], tlo, thi);
}

// min, max and "a non-finite value was seen" of v[0..n): part[3 b + 0..2] per workgroup b.
// min and max do not depend on the order; the host folds the partials.
__global__ __launch_bounds__(ROF_THREADS) void k_rof_range(const double *__restrict__ v, int64_t n,
                                                           double *__restrict__ part)
{
    __shared__ double red[3 * (ROF_THREADS / 64)];
    double lo = INFINITY, hi = -INFINITY, bad = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)ROF_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * ROF_THREADS) {
        const double a = v[i];
        if (!isfinite(a)) bad = 1.0;
        lo = fmin(lo, a);
        hi = fmax(hi, a);
    }
    for (int d = 32; d > 0; d >>= 1) {
        lo = fmin(lo, __shfl_down(lo, d, 64));
        hi = fmax(hi, __shfl_down(hi, d, 64));
        bad = fmax(bad, __shfl_down(bad, d, 64));
    }
    const int wave = threadIdx.x / 64;
    if (threadIdx.x % 64 == 0) {
        red[3 * wave] = lo;
        red[3 * wave + 1] = hi;
        red[3 * wave + 2] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < ROF_THREADS / 64; ++w) {
            lo = fmin(lo, red[3 * w]);
            hi = fmax(hi, red[3 * w + 1]);
            bad = fmax(bad, red[3 * w + 2]);
        }
        part[3 * blockIdx.x] = lo;
        part[3 * blockIdx.x + 1] = hi;
        part[3 * blockIdx.x + 2] = bad;
    }
}

// iterations per launch forced by gqmap_debug_rof_T (0: ROF_T_DEFAULT)
static int g_rof_T = 0;

template <int T>
static hipError_t rof_launch_fused(const double *x, const double *p1in, const double *p2in, double *p1out,
                                   double *p2out, int M, int N, int C, double theta, double delta, int iters,
                                   hipStream_t s)
{
    // above 64 KB (T = 8) the dynamic LDS limit must be raised
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rof_fused<T>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)rof_lds_bytes(T));
    if (e != hipSuccess) return e;
    const int tiles_m = (M + ROF_S - 1) / ROF_S, tiles_n = (N + ROF_S - 1) / ROF_S;
    k_rof_fused<T><<<dim3((unsigned)((int64_t)tiles_m * tiles_n), (unsigned)C), dim3(ROF_THREADS), rof_lds_bytes(T),
                     s>>>(x, p1in, p2in, p1out, p2out, M, N, tiles_m, theta, delta, iters);
    return hipGetLastError();
}

}  // namespace gq

using namespace gq;

namespace {
// kernel time over several stretches of the null stream (off: no events, no waits)
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

// range of a device array: one reduction launch, the partials folded here
gqmap_status rof_range(const double *dv, int64_t n, double *dpart, double *lo, double *hi, bool *bad,
                       Stopwatch &sw)
{
    const int blocks = (int)std::min<int64_t>(ROF_RED_BLOCKS, (n + ROF_THREADS - 1) / ROF_THREADS);
    std::vector<double> part(3 * (size_t)blocks);
    GQ_HIP(sw.begin());
    k_rof_range<<<dim3(blocks), dim3(ROF_THREADS), 0, 0>>>(dv, n, dpart);
    GQ_HIP(hipGetLastError());
    GQ_HIP(sw.end());
    GQ_HIP(hipMemcpy(part.data(), dpart, sizeof(double) * part.size(), hipMemcpyDeviceToHost));
    *lo = INFINITY, *hi = -INFINITY, *bad = false;
    for (int b = 0; b < blocks; ++b) {
        *lo = std::fmin(*lo, part[3 * b]);
        *hi = std::fmax(*hi, part[3 * b + 1]);
        *bad = *bad || part[3 * b + 2] != 0.0;
    }
    return GQMAP_OK;
}
}  // namespace

extern "C" {

// Not in the public header (tests, scripts/time_structure_texture.py): force
// the iterations one launch runs to 1 (plain form), 2, 4 or 8 (fused form); 0
// restores the default.  Never changes a result.
int gqmap_debug_rof_T(int T)
{
    if (T != 0 && !rof_legal_T(T)) return -1;
    g_rof_T = T;
    return 0;
}
// the fused form's output tile (rows = columns) and the default T
int gqmap_debug_rof_tile(void) { return ROF_S; }
int gqmap_debug_rof_default_T(void) { return ROF_T_DEFAULT; }

gqmap_status gqmap_structure_texture(const double *im, int M, int N, int C, double theta, int n_iter, double alp,
                                     double *texture, double *structure, double *elapsed_ms, int device)
{
    clear_error();
    GQ_CHECK(im && texture, GQMAP_ERR_INVALID_ARG, "gqmap_structure_texture: null argument");
    const char *bad = rof_bad_args(M, N, C, theta, n_iter, alp);
    GQ_CHECK(!bad, GQMAP_ERR_INVALID_ARG, "gqmap_structure_texture: %s (M=%d N=%d C=%d theta=%g n_iter=%d alp=%g)",
             bad, M, N, C, theta, n_iter, alp);
    const int ptiles_m = (M + ROF_PM - 1) / ROF_PM, ptiles_n = (N + ROF_PN - 1) / ROF_PN;
    GQ_CHECK((int64_t)ptiles_m * ptiles_n <= 0x7fffffff, GQMAP_ERR_INVALID_ARG,
             "gqmap_structure_texture: %dx%d has too many tiles", M, N);
    GQ_CHECK(gqmap_device_count() > device && device >= 0, GQMAP_ERR_NO_DEVICE, "no HIP device %d", device);
    DeviceGuard dg(device);
    const int T = g_rof_T ? g_rof_T : ROF_T_DEFAULT;
    const int64_t MN = (int64_t)M * N, n_all = MN * C;
    const size_t bytes = sizeof(double) * (size_t)n_all;

    // dIm holds the input, then (x taken) t and the texture; p1 and p2 of a side are one buffer
    DevBuf dIm, dX, dPa, dPb, dS, dPart;
    Stopwatch sw;
    GQ_HIP(hipMalloc(&dIm.p, bytes));
    GQ_HIP(hipMalloc(&dX.p, bytes));
    GQ_HIP(hipMalloc(&dPa.p, 2 * bytes));
    GQ_HIP(hipMalloc(&dPb.p, 2 * bytes));
    if (structure) GQ_HIP(hipMalloc(&dS.p, bytes));
    GQ_HIP(hipMalloc(&dPart.p, sizeof(double) * 3 * ROF_RED_BLOCKS));
    GQ_HIP(hipMemcpy(dIm.p, im, bytes, hipMemcpyHostToDevice));
    GQ_HIP(sw.init(elapsed_ms != nullptr));

    double lo, hi;
    bool nonfinite;
    gqmap_status st = rof_range(dIm.d(), n_all, dPart.d(), &lo, &hi, &nonfinite, sw);
    if (st != GQMAP_OK) return st;
    GQ_CHECK(!rof_bad_range(lo, hi, nonfinite), GQMAP_ERR_INVALID_ARG,
             "gqmap_structure_texture: input range [%g, %g] is zero or not finite", lo, hi);

    const double delta = rof_delta(theta);
    const int flat_blocks = (int)std::min<int64_t>(4096, (n_all + ROF_THREADS - 1) / ROF_THREADS);
    GQ_HIP(sw.begin());
    k_rof_scale_in<<<dim3(flat_blocks), dim3(ROF_THREADS), 0, 0>>>(dIm.d(), dX.d(), n_all, lo, hi);
    GQ_HIP(hipGetLastError());
    GQ_HIP(hipMemsetAsync(dPa.p, 0, 2 * bytes, 0));
    double *cur = dPa.d(), *nxt = dPb.d();
    for (int left = n_iter; left > 0;) {
        const int run = left < T ? left : T;
        if (T == 1) {
            k_rof_plain<<<dim3((unsigned)((int64_t)ptiles_m * ptiles_n), (unsigned)C), dim3(ROF_THREADS), 0, 0>>>(
                dX.d(), cur, cur + n_all, nxt, nxt + n_all, M, N, ptiles_m, theta, delta);
            GQ_HIP(hipGetLastError());
        } else {
            GQ_HIP(T == 2   ? rof_launch_fused<2>(dX.d(), cur, cur + n_all, nxt, nxt + n_all, M, N, C, theta, delta,
                                                  run, 0)
                   : T == 4 ? rof_launch_fused<4>(dX.d(), cur, cur + n_all, nxt, nxt + n_all, M, N, C, theta, delta,
                                                  run, 0)
                            : rof_launch_fused<8>(dX.d(), cur, cur + n_all, nxt, nxt + n_all, M, N, C, theta, delta,
                                                  run, 0));
        }
        std::swap(cur, nxt);
        left -= run;
    }
    k_rof_finish<<<dim3((unsigned)((int64_t)ptiles_m * ptiles_n), (unsigned)C), dim3(ROF_THREADS), 0, 0>>>(
        dX.d(), cur, cur + n_all, M, N, ptiles_m, theta, alp, dIm.d(), dS.d());
    GQ_HIP(hipGetLastError());
    GQ_HIP(sw.end());

    double tlo, thi;
    st = rof_range(dIm.d(), n_all, dPart.d(), &tlo, &thi, &nonfinite, sw);
    if (st != GQMAP_OK) return st;
    GQ_CHECK(!rof_bad_range(tlo, thi, nonfinite), GQMAP_ERR_INVALID_ARG,
             "gqmap_structure_texture: texture range [%g, %g] is zero or not finite", tlo, thi);
    GQ_HIP(sw.begin());
    k_rof_scale_out<<<dim3(flat_blocks), dim3(ROF_THREADS), 0, 0>>>(dIm.d(), n_all, tlo, thi);
    GQ_HIP(hipGetLastError());
    GQ_HIP(sw.end());

    GQ_HIP(hipMemcpy(texture, dIm.p, bytes, hipMemcpyDeviceToHost));
    if (structure) GQ_HIP(hipMemcpy(structure, dS.p, bytes, hipMemcpyDeviceToHost));
    if (elapsed_ms) *elapsed_ms = sw.ms;
    return GQMAP_OK;
}

}  // extern "C"
