// Scalar-load latency on gfx950: a chain of dependent scalar loads (each
// load's address is the value the one before returned) over a 5 KB constant
// table, the size of the K = 9 quadrature table, between two s_memtime
// stamps.  One and two waves per SIMD (workgroups of 256 and 512 threads: a
// workgroup's waves go round its CU's four SIMDs), one workgroup alone on the
// device and one per CU.  A hop is the load, its wait and the two SALU adds
// that form the next address.  s_memrealtime (100 MHz) beside it gives the
// rate of the s_memtime counter.
//   hipcc -O2 --offload-arch=gfx950 -o smem_latency scripts/micro/smem_latency.hip
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

constexpr int TAB_BYTES = 5 * 1024, TAB_N = TAB_BYTES / 4;
using ctab_t = const __attribute__((address_space(4))) uint32_t *;

__global__ void k_chain(const uint32_t *tab, int hops, unsigned long long *out)
{
    ctab_t t = (ctab_t)tab;
    uint32_t i = 0;
    // warm pass: every entry once, the table into the scalar cache
    for (int h = 0; h < TAB_N; ++h) i = t[__builtin_amdgcn_readfirstlane(i)];
    i = __builtin_amdgcn_readfirstlane(i);
    const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    for (int h = 0; h < hops; ++h) i = t[__builtin_amdgcn_readfirstlane(i)];
    asm volatile("" : "+s"(i));
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    const unsigned long long r1 = __builtin_amdgcn_s_memrealtime();
    if ((threadIdx.x & 63) == 0) {
        const int w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
        out[3 * w] = t1 - t0;
        out[3 * w + 1] = r1 - r0;
        out[3 * w + 2] = i;
    }
}

int main()
{
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, 0) != hipSuccess) return 2;
    const int cus = p.multiProcessorCount;
    // one cycle through all TAB_N entries: entry e holds the index of the next, a stride coprime to TAB_N
    std::vector<uint32_t> h(TAB_N);
    for (int e = 0; e < TAB_N; ++e) h[e] = (uint32_t)((e + 461) % TAB_N);
    uint32_t *tab;
    unsigned long long *out;
    const int maxw = cus * 8;
    if (hipMalloc(&tab, TAB_BYTES) != hipSuccess || hipMalloc(&out, sizeof(unsigned long long) * 3 * maxw) != hipSuccess) return 2;
    (void)hipMemcpy(tab, h.data(), TAB_BYTES, hipMemcpyHostToDevice);
    const int hops = 8192;
    printf("device %s, %d CUs, table %d bytes, %d dependent hops per wave\n", p.gcnArchName, cus, TAB_BYTES, hops);
    for (int blocks : {1, cus})
        for (int wps : {1, 2}) {
            const int threads = 256 * wps, nw = blocks * threads / 64;
            std::vector<unsigned long long> r(3 * nw);
            for (int rep = 0; rep < 2; ++rep) {  // (the second launch is the one read)
                k_chain<<<blocks, threads>>>(tab, hops, out);
                if (hipDeviceSynchronize() != hipSuccess) return 3;
            }
            (void)hipMemcpy(r.data(), out, sizeof(unsigned long long) * 3 * nw, hipMemcpyDeviceToHost);
            std::vector<double> c(nw);
            double rate = 0;
            for (int w = 0; w < nw; ++w) {
                c[w] = (double)r[3 * w] / hops;
                rate += (double)r[3 * w] / (double)r[3 * w + 1];
            }
            std::sort(c.begin(), c.end());
            printf("workgroups=%4d waves/SIMD=%d : s_memtime ticks per hop min %.1f median %.1f max %.1f  "
                   "(s_memtime / s_memrealtime = %.3f)\n",
                   blocks, wps, c[0], c[nw / 2], c[nw - 1], rate / nw);
        }
    (void)hipFree(tab);
    (void)hipFree(out);
    return 0;
}
