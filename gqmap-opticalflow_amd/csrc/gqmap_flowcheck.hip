// Forward-backward check and fill on the device.  The arithmetic is
// gqmap_flowcheck.h (shared with the host models gqmap_flow_consistency_host and
// gqmap_flow_fill_host); this file is the tiling.
//
//   k_flow_check  one lane per pixel, lanes along m.  The four samples of each
//                 bwd plane are gathered straight from device memory: they lie
//                 within the matcher's window of the pixel, so neighbouring
//                 lanes share cache lines.  No LDS, no barrier.
//   k_flow_fill   one pass of the fill.  One workgroup of 256 lanes owns a
//                 32 x 32 output tile and stages the (32 + 2r)^2 tile around it,
//                 V, S_0 and S_1, in LDS.  Per plane the row pass writes the
//                 32 x (32 + 2r) strip T and the column pass reads it into
//                 registers (four pixels per lane), so T is one buffer used
//                 three times: with W = 32 + 2r the workgroup holds
//                 8 W (3 W + 32) bytes, 114,688 B at r = 16.  A tile with
//                 nothing to fill (block-uniform, from the staged states)
//                 copies through.  Passes ping-pong two flow and two state
//                 buffers on one stream, one launch per pass; workgroups never
//                 wait for each other.
// Lanes run along m (the fastest index): global loads, stores and every LDS
// access are unit-stride over a wave.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "gqmap_flowcheck.h"
#include "gqmap_internal.h"

namespace gq {

constexpr int FC_S = 32;  // fill: output tile rows = columns
constexpr int FC_THREADS = 256;
constexpr int FC_PER_LANE = FC_S * FC_S / FC_THREADS;
constexpr int FC_PM = 64, FC_PN = 4;  // check: pixels of a workgroup (rows x columns)

static size_t fc_lds_bytes(int r)
{
    const size_t W = FC_S + 2 * (size_t)r;
    return sizeof(double) * W * (3 * W + FC_S);
}

__global__ __launch_bounds__(FC_THREADS) void k_flow_check(const double *__restrict__ fwd,
                                                           const double *__restrict__ bwd, int M, int N,
                                                           int tiles_m, double a1, double a2,
                                                           double *__restrict__ err,
                                                           unsigned char *__restrict__ mask)
{
    const int m = (int)(blockIdx.x % tiles_m) * FC_PM + (int)threadIdx.x % FC_PM;
    const int n = (int)(blockIdx.x / tiles_m) * FC_PN + (int)threadIdx.x / FC_PM;
    if (m >= M || n >= N) return;
    double e;
    const bool ok = fc_check(fwd, bwd, m, n, M, N, a1, a2, &e);
    const int64_t o = m + (int64_t)M * n;
    if (err) err[o] = e;
    if (mask) mask[o] = ok ? 1 : 0;
}

__global__ __launch_bounds__(FC_THREADS) void k_flow_fill(const double *__restrict__ fin,
                                                          const unsigned char *__restrict__ sin,
                                                          double *__restrict__ fout,
                                                          unsigned char *__restrict__ sout, int M, int N,
                                                          int tiles_m, int r, int pass, FcFilter f)
{
    extern __shared__ __align__(16) double fc_lds[];
    const int W = FC_S + 2 * r, CELLS = W * W;
    double *X = fc_lds, *T = X + 3 * CELLS;  // X: V, S_0, S_1, CELLS each
    const int tid = threadIdx.x;
    const int64_t MN = (int64_t)M * N;
    const int m0 = (int)(blockIdx.x % tiles_m) * FC_S, n0 = (int)(blockIdx.x / tiles_m) * FC_S;

    // tile cell c -> (lm, ln) = (c % W, c / W), frame pixel (m0 - r + lm, n0 - r + ln)
    int todo = 0;
    for (int c = tid; c < CELLS; c += FC_THREADS) {
        const int lm = c % W, ln = c / W, gm = m0 - r + lm, gn = n0 - r + ln;
        const bool in = gm >= 0 && gm < M && gn >= 0 && gn < N;
        const int64_t o = gm + (int64_t)M * gn;
        const bool valid = in && sin[o] != GQ_FC_UNFILLED;
        X[c] = valid ? 1.0 : 0.0;
        X[c + CELLS] = valid ? fin[o] : 0.0;
        X[c + 2 * CELLS] = valid ? fin[o + MN] : 0.0;
        if (in && !valid && lm >= r && lm < r + FC_S && ln >= r && ln < r + FC_S) todo = 1;
    }
    todo = __syncthreads_or(todo);  // the barrier after staging as well

    double y[3][FC_PER_LANE];
    if (todo) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const double *Xq = X + q * CELLS;
            // rows: T(lm, c) of output row lm and tile column c from the rows lm .. lm + 2r
            for (int i = tid; i < FC_S * W; i += FC_THREADS) T[i] = fc_rows(&Xq[i % FC_S + W * (i / FC_S)], r, f);
            __syncthreads();
            // columns: output pixel (lm, ln) from the tile columns ln .. ln + 2r
#pragma unroll
            for (int k = 0; k < FC_PER_LANE; ++k) y[q][k] = fc_cols(&T[tid + FC_THREADS * k], FC_S, r, f);
            __syncthreads();
        }
    }
#pragma unroll
    for (int k = 0; k < FC_PER_LANE; ++k) {
        const int i = tid + FC_THREADS * k, gm = m0 + i % FC_S, gn = n0 + i / FC_S;
        if (gm < M && gn < N) {
            const int64_t o = gm + (int64_t)M * gn;
            const unsigned char st = sin[o];
            const bool fill = todo && fc_fills(st, y[0][k]);
            fout[o] = fill ? y[1][k] / y[0][k] : fin[o];
            fout[o + MN] = fill ? y[2][k] / y[0][k] : fin[o + MN];
            sout[o] = fill ? (unsigned char)pass : st;
        }
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
}  // namespace

extern "C" {

// Not in the public header (tests, DESIGN): the fill's output tile (rows =
// columns) and the LDS bytes of one workgroup at radius r.
int gqmap_debug_flow_fill_tile(void) { return FC_S; }
int gqmap_debug_flow_fill_lds(int r) { return r < 0 || r > GQ_FC_RMAX ? -1 : (int)fc_lds_bytes(r); }

gqmap_status gqmap_flow_consistency(const double *fwd, const double *bwd, int M, int N, double a1, double a2,
                                    double *err, unsigned char *mask, double *elapsed_ms, int device)
{
    clear_error();
    GQ_CHECK(fwd && bwd && (err || mask), GQMAP_ERR_INVALID_ARG, "gqmap_flow_consistency: null argument");
    const char *bad = fc_bad_check(M, N, a1, a2);
    GQ_CHECK(!bad, GQMAP_ERR_INVALID_ARG, "gqmap_flow_consistency: %s (M=%d N=%d a1=%g a2=%g)", bad, M, N, a1, a2);
    const int tiles_m = (M + FC_PM - 1) / FC_PM, tiles_n = (N + FC_PN - 1) / FC_PN;
    GQ_CHECK((int64_t)tiles_m * tiles_n <= 0x7fffffff, GQMAP_ERR_INVALID_ARG,
             "gqmap_flow_consistency: %dx%d has too many tiles", M, N);
    GQ_CHECK(gqmap_device_count() > device && device >= 0, GQMAP_ERR_NO_DEVICE, "no HIP device %d", device);
    DeviceGuard dg(device);
    const size_t MN = (size_t)M * N, bytes = sizeof(double) * 2 * MN;
    DevBuf dF, dB, dE, dK;
    Stopwatch sw;
    GQ_HIP(hipMalloc(&dF.p, bytes));
    GQ_HIP(hipMalloc(&dB.p, bytes));
    if (err) GQ_HIP(hipMalloc(&dE.p, sizeof(double) * MN));
    if (mask) GQ_HIP(hipMalloc(&dK.p, MN));
    GQ_HIP(hipMemcpy(dF.p, fwd, bytes, hipMemcpyHostToDevice));
    GQ_HIP(hipMemcpy(dB.p, bwd, bytes, hipMemcpyHostToDevice));
    GQ_HIP(sw.init(elapsed_ms != nullptr));
    GQ_HIP(sw.begin());
    k_flow_check<<<dim3((unsigned)((int64_t)tiles_m * tiles_n)), dim3(FC_THREADS), 0, 0>>>(dF.d(), dB.d(), M, N, tiles_m,
                                                                                         a1, a2, dE.d(), dK.b());
    GQ_HIP(hipGetLastError());
    GQ_HIP(sw.end());
    if (err) GQ_HIP(hipMemcpy(err, dE.p, sizeof(double) * MN, hipMemcpyDeviceToHost));
    if (mask) GQ_HIP(hipMemcpy(mask, dK.p, MN, hipMemcpyDeviceToHost));
    if (elapsed_ms) *elapsed_ms = sw.ms;
    return GQMAP_OK;
}

gqmap_status gqmap_flow_fill(const double *flow, const unsigned char *mask, int M, int N, int r, double sigma,
                             int passes, double *out, unsigned char *filled, double *elapsed_ms, int device)
{
    clear_error();
    GQ_CHECK(flow && mask && out, GQMAP_ERR_INVALID_ARG, "gqmap_flow_fill: null argument");
    const char *bad = fc_bad_fill(M, N, r, sigma, passes);
    GQ_CHECK(!bad, GQMAP_ERR_INVALID_ARG, "gqmap_flow_fill: %s (M=%d N=%d r=%d sigma=%g passes=%d)", bad, M, N, r,
             sigma, passes);
    const int tiles_m = (M + FC_S - 1) / FC_S, tiles_n = (N + FC_S - 1) / FC_S;
    GQ_CHECK((int64_t)tiles_m * tiles_n <= 0x7fffffff, GQMAP_ERR_INVALID_ARG,
             "gqmap_flow_fill: %dx%d has too many tiles", M, N);
    GQ_CHECK(gqmap_device_count() > device && device >= 0, GQMAP_ERR_NO_DEVICE, "no HIP device %d", device);
    DeviceGuard dg(device);
    const size_t MN = (size_t)M * N, bytes = sizeof(double) * 2 * MN;
    const FcFilter f = fc_filter(r, sigma);
    std::vector<unsigned char> state(MN);
    for (size_t i = 0; i < MN; ++i) state[i] = mask[i] ? 0 : GQ_FC_UNFILLED;

    DevBuf dFa, dFb, dSa, dSb;
    Stopwatch sw;
    GQ_HIP(hipMalloc(&dFa.p, bytes));
    GQ_HIP(hipMalloc(&dFb.p, bytes));
    GQ_HIP(hipMalloc(&dSa.p, MN));
    GQ_HIP(hipMalloc(&dSb.p, MN));
    GQ_HIP(hipMemcpy(dFa.p, flow, bytes, hipMemcpyHostToDevice));
    GQ_HIP(hipMemcpy(dSa.p, state.data(), MN, hipMemcpyHostToDevice));
    // above 64 KB (r >= 7) the dynamic LDS limit must be raised
    GQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_flow_fill), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)fc_lds_bytes(GQ_FC_RMAX)));
    GQ_HIP(sw.init(elapsed_ms != nullptr));
    GQ_HIP(sw.begin());
    double *fcur = dFa.d(), *fnxt = dFb.d();
    unsigned char *scur = dSa.b(), *snxt = dSb.b();
    for (int p = 1; p <= passes; ++p) {
        k_flow_fill<<<dim3((unsigned)((int64_t)tiles_m * tiles_n)), dim3(FC_THREADS), fc_lds_bytes(r), 0>>>(
            fcur, scur, fnxt, snxt, M, N, tiles_m, r, p, f);
        GQ_HIP(hipGetLastError());
        std::swap(fcur, fnxt);
        std::swap(scur, snxt);
    }
    GQ_HIP(sw.end());
    GQ_HIP(hipMemcpy(out, fcur, bytes, hipMemcpyDeviceToHost));
    if (filled) GQ_HIP(hipMemcpy(filled, scur, MN, hipMemcpyDeviceToHost));
    if (elapsed_ms) *elapsed_ms = sw.ms;
    return GQMAP_OK;
}

}  // extern "C"
