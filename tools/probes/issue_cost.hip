// Issue cost of the vector instructions the Tier-1 modeller's block load could do without -- v_mul_lo_u32, v_mul_u32_u24,
// v_mad_u64_u32 (row addresses), v_rcp_f32 (inside the division), v_lshlrev_b64 (sign masks) -- against a plain v_add_u32:
// four independent chains per wave, four waves per SIMD on every CU, so the issue rate is what is timed.
//   hipcc -O2 --offload-arch=gfx950 -o /tmp/issue_cost tools/probes/issue_cost.hip && /tmp/issue_cost
#include <hip/hip_runtime.h>
#include <cstdio>
typedef unsigned long long u64;
template <int KIND> __global__ void k(unsigned *out, unsigned seed, int iters)
{
    unsigned a = seed + threadIdx.x, b = seed * 3 + threadIdx.x, c = seed * 5 + 1, d = seed * 7 + 3;
    u64 p = a, q = b, r = c, s = d;
    float f = 1.0f + a, g = 2.0f + b, h = 3.0f + c, j = 5.0f + d;
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            if (KIND == 0)
                asm volatile("v_add_u32 %0, %0, %4\n v_add_u32 %1, %1, %4\n v_add_u32 %2, %2, %4\n v_add_u32 %3, %3, %4" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "s"(0x1020409u));
            else if (KIND == 1)
                asm volatile("v_mul_lo_u32 %0, %0, %4\n v_mul_lo_u32 %1, %1, %4\n v_mul_lo_u32 %2, %2, %4\n v_mul_lo_u32 %3, %3, %4" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "s"(0x1020409u));
            else if (KIND == 2)
                asm volatile("v_mul_u32_u24 %0, %0, %4\n v_mul_u32_u24 %1, %1, %4\n v_mul_u32_u24 %2, %2, %4\n v_mul_u32_u24 %3, %3, %4" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "s"(0x204081u));
            else if (KIND == 3)
                asm volatile("v_mad_u64_u32 %0, vcc, %4, %5, %0\n v_mad_u64_u32 %1, vcc, %4, %5, %1\n v_mad_u64_u32 %2, vcc, %4, %5, %2\n v_mad_u64_u32 %3, vcc, %4, %5, %3"
                             : "+v"(p), "+v"(q), "+v"(r), "+v"(s) : "v"(a), "s"(0x1020409u) : "vcc");
            else if (KIND == 4)
                asm volatile("v_rcp_f32 %0, %0\n v_rcp_f32 %1, %1\n v_rcp_f32 %2, %2\n v_rcp_f32 %3, %3" : "+v"(f), "+v"(g), "+v"(h), "+v"(j));
            else
                asm volatile("v_lshlrev_b64 %0, %4, %0\n v_lshlrev_b64 %1, %4, %1\n v_lshlrev_b64 %2, %4, %2\n v_lshlrev_b64 %3, %4, %3" : "+v"(p), "+v"(q), "+v"(r), "+v"(s) : "v"(a & 1u));
        }
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = a ^ b ^ c ^ d ^ (unsigned)(p ^ q ^ r ^ s) ^ (unsigned)((p ^ q ^ r ^ s) >> 32) ^ __float_as_uint(f + g + h + j);
}
template <int KIND> float run(unsigned *d, int iters, hipEvent_t e0, hipEvent_t e1)
{
    hipEventRecord(e0);
    // 1024 workgroups of 256 threads = 4 waves per SIMD on 256 CUs: issue-bound
    hipLaunchKernelGGL(k<KIND>, dim3(1024), dim3(256), 0, 0, d, 12345u, iters);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    return ms;
}
int main()
{
    unsigned *d = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&d), 1024 * 256 * 4) != hipSuccess) { std::printf("no device memory\n"); return 1; }
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    const int iters = 2000;
    const char *names[6] = {"v_add_u32", "v_mul_lo_u32", "v_mul_u32_u24", "v_mad_u64_u32", "v_rcp_f32", "v_lshlrev_b64"};
    float base = 0;
    for (int rep = 0; rep < 2; ++rep) // (the first round warms up)
        for (int kind = 0; kind < 6; ++kind) {
            const float ms = kind == 0 ? run<0>(d, iters, e0, e1) : kind == 1 ? run<1>(d, iters, e0, e1) : kind == 2 ? run<2>(d, iters, e0, e1)
                           : kind == 3 ? run<3>(d, iters, e0, e1) : kind == 4 ? run<4>(d, iters, e0, e1) : run<5>(d, iters, e0, e1);
            if (kind == 0) base = ms;
            const double insts = 1024.0 * 4 * iters * 64; // wave-instructions
            std::printf("round %d  %-14s %8.3f ms  %5.2f cycles per wave-instruction per SIMD (at 2.4 GHz)  %.2f x v_add_u32\n", rep, names[kind], ms,
                        ms * 1e-3 * 2.4e9 / (insts / 1024.0), ms / base);
        }
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
