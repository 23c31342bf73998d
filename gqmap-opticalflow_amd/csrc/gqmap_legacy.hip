// gqmap_legacy.hip -- device drop-in for legacy/gqmap_cpu.m, the legacy
// flow-denoising QGMAP ([mu,sigma,rou] = gqmap_cpu(options, flow)): a
// Gaussian observation of a given flow field (node, :20-26), truncated
// quadratic pairwise terms (edges, :28-54), the reference's own neighbour
// shift in the gradient sum (:58-60), plain gradient ascent with
// sigma = |sigma + dsigma*step| and rou clamped to +-0.97 (:62-65).
//
// Per iteration: k_legacy_grad (one thread per node m < M-1, n < N-1, edge
// and layer: one K x K edge rule, plus the K-point node rule on the j = 0
// threads, written to dnode/dedge in the reference's M x N x 2 x 2 /
// M x N x 2 x 5 x 2 layout), k_legacy_update (one thread per node and layer:
// sums, step, clamps, per-workgroup maxima on the bit patterns of |x|),
// k_legacy_ctl (their maxima -> trace, stop rule).
// No host round trip inside the loop.  Plain fp64 with contraction off in the
// order of the MATLAB expressions, so the device matches the C restatement
// (oracle/gqmap_legacy_oracle.c) bit for bit.
//
// gqmap_flow_denoise is the same loop with a variance field and an observation
// select in the node rule, a start of its own and the adjoint scatter in the
// sum (gqmap_denoise.h holds the rules of both): further instantiations of
// k_legacy_grad / k_legacy_update, and k_legacy_finite once before the loop.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "gqmap_denoise.h"
#include "gqmap_internal.h"

#pragma clang fp contract(off)

namespace gq {
namespace {

constexpr int LG_KMAX = GQMAP_KMAX;

struct LgParams {
    const double *flow;
    const double *varf;           // the variance field (M x N x 2) or null: the scalar var
    double *mu, *sigma, *rou, *dnode, *dedge;
    unsigned long long *blkmax;   // [update workgroups][3]: |dmu|, |dsigma|, |drou| maxima as bits
    int *ctl;                     // it, stop, done
    double *trace;
    int M, N, K, its, min_its, nblk;
    double var, gama, dta, step0, step_decay, corr, tor;
    double X[LG_KMAX], W[LG_KMAX];
    double WW[LG_KMAX * LG_KMAX];  // W[c] * W[r] at r + K*c (WIWJ, :5-6), the host's product
};

// One thread per node m < M-1, n < N-1, edge j and layer l ((j, l) slowest:
// a wave stays on one edge of one layer): the edge rule (j, l) of the node,
// and on the j = 0 threads the node rule of layer l too (9 of ~170 points).
// The rules are gqmap_denoise.h's, expanded here (see there why not called).
// KT: K as a template constant (0: P.K at run time); GAMA1: gama == 1; VM: the
// scalar var, var == 1, or the variance field P.varf with the observation
// select (one more coalesced load on the node-rule threads; P.varf == NULL:
// the scalar var, observed where the flow is finite); DTA_INF: dta == inf.
template <int KT, bool GAMA1, int VM, bool DTA_INF>
__global__ __launch_bounds__(256) void k_legacy_grad(LgParams P)
{
    if (P.ctl[1]) return;
    const int M = P.M, N = P.N;
    const int64_t MN1 = (int64_t)(M - 1) * (N - 1);
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 4 * MN1) return;
    const int jl = (int)(t / MN1), j = jl & 1, l = jl >> 1;
    t -= jl * MN1;
    const int m = (int)(t % (M - 1)), n = (int)(t / (M - 1));
    const double o1 = P.sigma[dn_i3(M, N, m, n, l)], u1 = P.mu[dn_i3(M, N, m, n, l)];
    if (j == 0) {  // (:20-26)
        const double f = P.flow[dn_i3(M, N, m, n, l)];
        double var = P.var;
        bool obs = true;
        if (VM == GQ_DN_VAR_FIELD) {
            if (P.varf) var = P.varf[dn_i3(M, N, m, n, l)];
            obs = dn_observed(f, P.varf != nullptr, var);
        }
        double dn[2];
        GQ_DN_NODE_RULE(P, KT, VM, sqrt(2.0) * o1, u1, f, var, obs, dn);
        P.dnode[dn_i4(M, N, m, n, 0, l)] = dn[0];
        P.dnode[dn_i4(M, N, m, n, 1, l)] = dn[1];
    }
    {  // (:28-54)
        const int m2 = m + (j == 0), n2 = n + (j == 1);
        const double p = P.rou[dn_i4(M, N, m, n, j, l)];
        const double o2 = P.sigma[dn_i3(M, N, m2, n2, l)], u2 = P.mu[dn_i3(M, N, m2, n2, l)];
        double de[5];
        GQ_DN_EDGE_RULE(P, KT, GAMA1, DTA_INF, p, o1, u1, o2, u2, de);
        for (int q = 0; q < 5; ++q) P.dedge[dn_i5(M, N, m, n, j, q, l)] = de[q];
    }
}

// Maximum over the block of three bit patterns (thread 0 holds the result).
__device__ void block_max3(unsigned long long &a, unsigned long long &b, unsigned long long &c)
{
    __shared__ unsigned long long red[3][16];
    for (int o = 32; o > 0; o >>= 1) {
        a = max(a, __shfl_xor(a, o));
        b = max(b, __shfl_xor(b, o));
        c = max(c, __shfl_xor(c, o));
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = (int)(blockDim.x + 63) >> 6;
    if (lane == 0) { red[0][wave] = a; red[1][wave] = b; red[2][wave] = c; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < nw; ++w) {
            a = max(a, red[0][w]);
            b = max(b, red[1][w]);
            c = max(c, red[2][w]);
        }
}

// One thread per node and layer: sums, step, clamps; the workgroup's maxima
// of |dmu|, |dsigma|, |drou| go to its own blkmax row (plain stores: one
// atomicMax per workgroup on three shared addresses serialises in L2, and a
// last-workgroup reduction needs a device-scope release per workgroup, an L2
// writeback each -- 70 us per launch) and k_legacy_ctl reduces the rows.
// ADJ: the adjoint scatter of gqmap_denoise.h (dn_gather), otherwise the
// reference's own shift.
template <bool ADJ>
__global__ __launch_bounds__(256) void k_legacy_update(LgParams P)
{
    if (P.ctl[1]) return;
    const int M = P.M, N = P.N;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int it = P.ctl[0];
    // Threads past the last node contribute zeros: every thread reaches the
    // single block_max3 call below (its barrier is never on a divergent path).
    double a = 0, b = 0, mp = 0;
    if (t < (int64_t)M * N * 2) {
        const int m = (int)(t % M), n = (int)((t / M) % N), l = (int)(t / ((int64_t)M * N));
        dn_gather<ADJ>(P.dnode, P.dedge, M, N, m, n, l, a, b);
        mp = dn_apply(P.mu, P.sigma, P.rou, P.dedge, M, N, m, n, l, a, b, dn_step(P.step0, it, P.step_decay), P.corr);
    }
    unsigned long long ba = dn_abits(a), bb = dn_abits(b), bm = dn_abits(mp);
    block_max3(ba, bb, bm);
    if (threadIdx.x == 0) {
        unsigned long long *row = P.blkmax + 3 * (size_t)blockIdx.x;
        row[0] = ba;
        row[1] = bb;
        row[2] = bm;
    }
}

// Is any entry of a (or of b, which may be null) NaN or +-Inf?  flags[0] / flags[1]
// are zero on entry; every thread that finds one stores the same 1.
__global__ __launch_bounds__(256) void k_legacy_finite(const double *a, const double *b, int64_t n, int *flags)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (!dn_finite(a[i])) flags[0] = 1;
    if (b && !dn_finite(b[i])) flags[1] = 1;
}

// sigma = rand(M,N,2) + 2 (:10) from the library RNG stream 3: the host
// formula, evaluated on the device
__global__ void k_legacy_sigma0(double *sigma, int64_t n, uint64_t base)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sigma[i] = u01(base, (uint64_t)i) + 2;
}

// One workgroup: the maxima over the update's blkmax rows -> trace, then
// the iteration counter and the stop rule.
__global__ __launch_bounds__(1024) void k_legacy_ctl(LgParams P)
{
    if (P.ctl[1]) return;
    unsigned long long a = 0, b = 0, c = 0;
    for (int i = threadIdx.x; i < P.nblk; i += blockDim.x) {
        const unsigned long long *row = P.blkmax + 3 * (size_t)i;
        a = max(a, row[0]);
        b = max(b, row[1]);
        c = max(c, row[2]);
    }
    block_max3(a, b, c);
    if (threadIdx.x != 0) return;
    const int it = P.ctl[0];
    const unsigned long long bits[3] = {a, b, c};
    double mx[3];
    for (int q = 0; q < 3; ++q) {
        mx[q] = dn_from_bits(bits[q]);
        P.trace[3 * (it - 1) + q] = mx[q];
    }
    P.ctl[0] = it + 1;
    P.ctl[2] = it;
    if (dn_stop(it, P.its, P.min_its, mx[0], P.tor)) P.ctl[1] = 1;  // (:70)
}

// One device arena per host thread and device, kept across calls: the nine
// buffers (~300 B per pixel) of gqmap_cpu_run are carved from it, so a
// repeated call pays no hipMalloc/hipFree (they dominated a 50-iteration
// call's wall clock).  gqmap_cpu_release() frees the calling thread's arenas.
struct Arena {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t release()
    {
        void *q = p;
        p = nullptr;  // cleared before the result is checked: never a dangling pointer
        cap = 0;
        return q ? hipFree(q) : hipSuccess;
    }
    ~Arena() { (void)release(); }
};
constexpr int kArenaDev = 64;
thread_local Arena g_arenas[kArenaDev];

}  // namespace
}  // namespace gq

using namespace gq;

extern "C" {

void gqmap_cpu_options_default(gqmap_cpu_options *o)
{
    std::memset(o, 0, sizeof(*o));
    o->its = 50;
    o->K = 9;
    o->var = 1.0;
    o->gama = 1.0;
    o->dta = INFINITY;
    o->step0 = 0.1;          // step = 0.1/(1+it/1000) (:62)
    o->step_decay = 1000.0;
    o->corr_tor = 0.97;      // (:65)
    o->tor = 1e-3;           // (:12)
    o->min_its = 100;        // (:70)
}

gqmap_status gqmap_cpu_release(void)
{
    clear_error();
    int cur = -1;
    (void)hipGetDevice(&cur);
    hipError_t first = hipSuccess;
    for (int d = 0; d < kArenaDev; ++d) {
        if (!g_arenas[d].p) continue;
        if (hipSetDevice(d) != hipSuccess) continue;
        const hipError_t e = g_arenas[d].release();
        if (first == hipSuccess) first = e;
    }
    if (cur >= 0) (void)hipSetDevice(cur);
    GQ_HIP(first);
    return GQMAP_OK;
}

}  // extern "C"

namespace {

// Does p point into device memory of `device` (or managed memory)?  Memory
// of another GPU would be read through peer access, or fault.
bool on_device(const void *p, int device)
{
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();  // a plain host pointer: clear the sticky error
        return false;
    }
    if (at.type == hipMemoryTypeManaged) return true;
    return at.type == hipMemoryTypeDevice && at.device == device;
}

// Do the byte ranges [a, a + na) and [b, b + nb) overlap?
bool overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return na && nb && x < y + nb && y < x + na;
}

// gqmap_cpu_run (DEV = false: host arrays, copied in and out) and
// gqmap_cpu_run_device (DEV = true: flow / sigma0 / mu / sigma / rou / trace
// are device arrays; the iteration runs on mu / sigma / rou in place).
// DENOISE: gqmap_flow_denoise / gqmap_flow_denoise_device -- var and mu0 (each
// may be null) join the inputs, the start is checked by k_legacy_finite before
// the loop, scatter chooses the sum.  Without DENOISE var and mu0 are null,
// scatter is the reference's and nothing is checked: gqmap_cpu_run as it was.
gqmap_status cpu_run(const gqmap_cpu_options *o, const double *flow, const double *var, const double *mu0, int M, int N,
                     const double *sigma0, uint64_t seed, int scatter, double *mu, double *sigma, double *rou,
                     double *trace, int *its_done, int device, bool DEV, bool DENOISE)
{
    const char *fn = DENOISE ? (DEV ? "gqmap_flow_denoise_device" : "gqmap_flow_denoise")
                             : (DEV ? "gqmap_cpu_run_device" : "gqmap_cpu_run");
    GQ_CHECK(o && flow && mu && sigma && rou, GQMAP_ERR_INVALID_ARG, "%s: null argument", fn);
    GQ_CHECK(M >= 2 && N >= 2, GQMAP_ERR_INVALID_ARG, "%s: flow %dx%d too small", fn, M, N);
    GQ_CHECK(o->K >= 1 && o->K <= GQMAP_KMAX, GQMAP_ERR_INVALID_ARG, "K=%d outside [1,%d]", o->K, GQMAP_KMAX);
    GQ_CHECK(o->its >= 1, GQMAP_ERR_INVALID_ARG, "its=%d", o->its);
    GQ_CHECK(scatter == GQMAP_SCATTER_REFERENCE || scatter == GQMAP_SCATTER_ADJOINT, GQMAP_ERR_INVALID_ARG,
             "%s: scatter=%d (0: reference, 1: adjoint)", fn, scatter);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_error("no HIP device available");
        return GQMAP_ERR_NO_DEVICE;
    }
    GQ_CHECK(device >= 0 && device < ndev, GQMAP_ERR_INVALID_ARG, "device %d of %d", device, ndev);
    GQ_CHECK(device < kArenaDev, GQMAP_ERR_INVALID_ARG, "device %d >= %d", device, kArenaDev);
    DeviceGuard dg(device);
    const size_t MN = (size_t)M * N;
    if (DEV) {
        GQ_CHECK(on_device(flow, device) && on_device(mu, device) && on_device(sigma, device) &&
                     on_device(rou, device) && (!sigma0 || on_device(sigma0, device)) &&
                     (!trace || on_device(trace, device)) && (!var || on_device(var, device)) &&
                     (!mu0 || on_device(mu0, device)),
                 GQMAP_ERR_INVALID_ARG, "%s: every array must be device memory of device %d", fn, device);
        // the outputs (written in place during the run) must not overlap each
        // other or an input
        const size_t b2 = sizeof(double) * 2 * MN;
        const struct { const void *p; size_t n; } out[4] = {
            {mu, b2}, {sigma, b2}, {rou, 2 * b2}, {trace, trace ? sizeof(double) * 3 * (size_t)o->its : 0}};
        const struct { const void *p; size_t n; const char *name; } in[4] = {
            {flow, b2, "flow"}, {sigma0, sigma0 ? b2 : 0, "sigma0"}, {var, var ? b2 : 0, "var"}, {mu0, mu0 ? b2 : 0, "mu0"}};
        for (int i = 0; i < 4; ++i) {
            for (int j = i + 1; j < 4; ++j)
                GQ_CHECK(!overlap(out[i].p, out[i].n, out[j].p, out[j].n), GQMAP_ERR_INVALID_ARG,
                         "%s: output arrays %d and %d overlap (mu, sigma, rou, trace)", fn, i, j);
            for (int j = 0; j < 4; ++j)
                GQ_CHECK(!overlap(out[i].p, out[i].n, in[j].p, in[j].n), GQMAP_ERR_INVALID_ARG,
                         "%s: output array %d (mu, sigma, rou, trace) overlaps %s", fn, i, in[j].name);
        }
    }
    LgParams P{};
    P.M = M; P.N = N; P.K = o->K; P.its = o->its; P.min_its = o->min_its;
    P.var = o->var; P.gama = o->gama; P.dta = o->dta; P.step0 = o->step0; P.step_decay = o->step_decay;
    P.corr = o->corr_tor; P.tor = o->tor;
    if (gauss_hermite(o->K, P.X, P.W) != 0) {
        set_error("Gauss-Hermite did not converge for K=%d", o->K);
        return GQMAP_ERR_INVALID_ARG;
    }
    for (int c = 0; c < o->K; ++c)
        for (int r = 0; r < o->K; ++r) P.WW[r + o->K * c] = P.W[c] * P.W[r];  // WIWJ (:5-6)
    const int g1 = (int)((4 * (int64_t)(M - 1) * (N - 1) + 255) / 256), nblk = (int)((2 * (int64_t)MN + 255) / 256);
    P.nblk = nblk;
    // One device arena per host thread and device, kept across calls: the
    // buffers (~300 B per pixel with host arrays, ~200 with device arrays)
    // are carved from it, so a repeated call pays no hipMalloc/hipFree (they
    // dominated a 50-iteration call's wall clock).
    struct Buf { void *p = nullptr; };
    Buf bflow, bmu, bsg, brou, bdn, bde, bmax, bctl, btr, bvar;
    const size_t io = DEV ? 0 : 1, tr = DEV && trace ? 0 : 1, vf = !DEV && var ? 1 : 0;
    constexpr int NBUF = 10;
    const size_t sizes[NBUF] = {io * sizeof(double) * 2 * MN, io * sizeof(double) * 2 * MN, io * sizeof(double) * 2 * MN,
                                io * sizeof(double) * 4 * MN, sizeof(double) * 4 * MN, sizeof(double) * 20 * MN,
                                sizeof(unsigned long long) * 3 * (size_t)nblk, sizeof(int) * 8,
                                tr * sizeof(double) * 3 * (size_t)o->its, vf * sizeof(double) * 2 * MN};
    Buf *bufs[NBUF] = {&bflow, &bmu, &bsg, &brou, &bdn, &bde, &bmax, &bctl, &btr, &bvar};
    size_t need = 0;
    for (size_t sz : sizes) need += (sz + 255) & ~(size_t)255;
    Arena &A = g_arenas[device];
    // Regrow when too small, shrink when a call needs under a quarter of it
    // (a large call does not pin its footprint for the thread's lifetime).
    if (A.cap < need || need < A.cap / 4) {
        GQ_HIP(A.release());
        const size_t cap = need + need / 8;  // headroom: a longer run reuses it
        GQ_HIP(hipMalloc(&A.p, cap));
        A.cap = cap;
    }
    size_t off = 0;
    for (int i = 0; i < NBUF; ++i) {
        bufs[i]->p = (char *)A.p + off;
        off += (sizes[i] + 255) & ~(size_t)255;
    }
    if (DEV) {
        bflow.p = const_cast<double *>(flow);
        bmu.p = mu;
        bsg.p = sigma;
        brou.p = rou;
        if (trace) btr.p = trace;
    } else {
        GQ_HIP(hipMemcpy(bflow.p, flow, sizeof(double) * 2 * MN, hipMemcpyHostToDevice));
        if (var) GQ_HIP(hipMemcpy(bvar.p, var, sizeof(double) * 2 * MN, hipMemcpyHostToDevice));
    }
    const int ctl0[8] = {1, 0, 0, 0, 0, 0, 0, 0};  // it, stop, done, -, start not finite, flow not finite
    GQ_HIP(hipMemcpy(bctl.p, ctl0, sizeof(ctl0), hipMemcpyHostToDevice));
    // the start: mu0 (host arrays: uploaded straight into the arena's mu) or the flow
    const bool up = !DEV && mu0;
    if (up) GQ_HIP(hipMemcpy(bmu.p, mu0, sizeof(double) * 2 * MN, hipMemcpyHostToDevice));
    const double *start = mu0 ? (DEV ? mu0 : (const double *)bmu.p) : (const double *)bflow.p;
    bool flow_finite = true;
    if (DENOISE) {  // before anything is written to an output
        k_legacy_finite<<<(int)((2 * MN + 255) / 256), 256>>>(start, mu0 ? (const double *)bflow.p : nullptr,
                                                             (int64_t)(2 * MN), (int *)bctl.p + 4);
        GQ_HIP(hipGetLastError());
        int flags[2];
        GQ_HIP(hipMemcpy(flags, (int *)bctl.p + 4, sizeof(flags), hipMemcpyDeviceToHost));
        GQ_CHECK(!flags[0], GQMAP_ERR_INVALID_ARG, "%s: %s", fn,
                 mu0 ? "mu0 must be finite everywhere" : "without mu0 the flow is the start and must be finite everywhere");
        flow_finite = !flags[1];
    }
    // mu = flow (:9) or mu0; sigma = rand(M,N,2) + 2 (:10, library RNG stream
    // 3, drawn on the device) unless given; rou = 0 (:11)
    if (!up) GQ_HIP(hipMemcpy(bmu.p, start, sizeof(double) * 2 * MN, hipMemcpyDeviceToDevice));
    if (sigma0)
        GQ_HIP(hipMemcpy(bsg.p, sigma0, sizeof(double) * 2 * MN, DEV ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    else
        k_legacy_sigma0<<<(int)((2 * MN + 255) / 256), 256>>>((double *)bsg.p, (int64_t)(2 * MN), stream_base(seed, 3));
    GQ_HIP(hipMemset(brou.p, 0, sizeof(double) * 4 * MN));
    GQ_HIP(hipMemset(bdn.p, 0, sizeof(double) * 4 * MN));   // dnode = zeros (:14): last row/col stay 0
    GQ_HIP(hipMemset(bde.p, 0, sizeof(double) * 20 * MN));  // dedge = zeros (:15)
    P.varf = var ? (DEV ? var : (const double *)bvar.p) : nullptr;
    P.flow = (const double *)bflow.p; P.mu = (double *)bmu.p; P.sigma = (double *)bsg.p; P.rou = (double *)brou.p;
    P.dnode = (double *)bdn.p; P.dedge = (double *)bde.p; P.blkmax = (unsigned long long *)bmax.p;
    P.ctl = (int *)bctl.p; P.trace = (double *)btr.p;
    // the grad kernel's compile-time variants: K = 9 (the reference's) or any
    // K; gama / var == 1; dta == inf (the defaults).  The variance-field
    // variant (with its observation select) runs only where it is needed: a
    // field is given, or the flow holds an entry that is not finite.  Every
    // other call -- gqmap_cpu_run always -- takes the scalar variants.
    using Kern = void (*)(LgParams);
#define GQ_LG_ROW(KT, G) \
    {{k_legacy_grad<KT, G, 0, false>, k_legacy_grad<KT, G, 0, true>}, \
     {k_legacy_grad<KT, G, 1, false>, k_legacy_grad<KT, G, 1, true>}, \
     {k_legacy_grad<KT, G, 2, false>, k_legacy_grad<KT, G, 2, true>}}
    static constexpr Kern kGrad[2][2][3][2] = {{GQ_LG_ROW(0, false), GQ_LG_ROW(0, true)},
                                               {GQ_LG_ROW(9, false), GQ_LG_ROW(9, true)}};
#undef GQ_LG_ROW
    static_assert(GQ_DN_VAR_SCALAR == 0 && GQ_DN_VAR_ONE == 1 && GQ_DN_VAR_FIELD == 2, "kGrad's third index");
    const int vm = P.varf || !flow_finite ? GQ_DN_VAR_FIELD : P.var == 1.0 ? GQ_DN_VAR_ONE : GQ_DN_VAR_SCALAR;
    const Kern grad = kGrad[P.K == 9][P.gama == 1.0][vm][P.dta == INFINITY];
    const Kern update = scatter == GQMAP_SCATTER_ADJOINT ? k_legacy_update<true> : k_legacy_update<false>;
    for (int it = 0; it < o->its; ++it) {
        grad<<<g1, 256>>>(P);
        update<<<nblk, 256>>>(P);
        k_legacy_ctl<<<1, 1024>>>(P);
    }
    GQ_HIP(hipGetLastError());
    GQ_HIP(hipDeviceSynchronize());
    int ctl[4];
    GQ_HIP(hipMemcpy(ctl, bctl.p, sizeof(ctl), hipMemcpyDeviceToHost));
    if (!DEV) {
        GQ_HIP(hipMemcpy(mu, bmu.p, sizeof(double) * 2 * MN, hipMemcpyDeviceToHost));
        GQ_HIP(hipMemcpy(sigma, bsg.p, sizeof(double) * 2 * MN, hipMemcpyDeviceToHost));
        GQ_HIP(hipMemcpy(rou, brou.p, sizeof(double) * 4 * MN, hipMemcpyDeviceToHost));
        if (trace)
            GQ_HIP(hipMemcpy(trace, btr.p, sizeof(double) * 3 * (size_t)ctl[2], hipMemcpyDeviceToHost));
    }
    if (its_done) *its_done = ctl[2];
    return GQMAP_OK;
}

}  // namespace

extern "C" {

gqmap_status gqmap_cpu_run(const gqmap_cpu_options *o, const double *flow, int M, int N, const double *sigma0,
                           uint64_t seed, double *mu, double *sigma, double *rou, double *trace, int *its_done,
                           int device)
{
    clear_error();
    return cpu_run(o, flow, nullptr, nullptr, M, N, sigma0, seed, GQMAP_SCATTER_REFERENCE, mu, sigma, rou, trace,
                   its_done, device, false, false);
}

gqmap_status gqmap_cpu_run_device(const gqmap_cpu_options *o, const double *flow, int M, int N,
                                  const double *sigma0, uint64_t seed, double *mu, double *sigma, double *rou,
                                  double *trace, int *its_done, int device)
{
    clear_error();
    return cpu_run(o, flow, nullptr, nullptr, M, N, sigma0, seed, GQMAP_SCATTER_REFERENCE, mu, sigma, rou, trace,
                   its_done, device, true, false);
}

gqmap_status gqmap_flow_denoise(const gqmap_cpu_options *o, const double *flow, const double *var, const double *mu0,
                                int M, int N, const double *sigma0, uint64_t seed, int scatter, double *mu,
                                double *sigma, double *rou, double *trace, int *its_done, int device)
{
    clear_error();
    return cpu_run(o, flow, var, mu0, M, N, sigma0, seed, scatter, mu, sigma, rou, trace, its_done, device, false, true);
}

gqmap_status gqmap_flow_denoise_device(const gqmap_cpu_options *o, const double *flow, const double *var,
                                       const double *mu0, int M, int N, const double *sigma0, uint64_t seed,
                                       int scatter, double *mu, double *sigma, double *rou, double *trace,
                                       int *its_done, int device)
{
    clear_error();
    return cpu_run(o, flow, var, mu0, M, N, sigma0, seed, scatter, mu, sigma, rou, trace, its_done, device, true, true);
}

}  // extern "C"
