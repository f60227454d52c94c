// Is the three-instruction quotient  q = f * r;  e = fma(-q, s, f);  q = fma(e, r, q)  with r = the correctly rounded 1 / s
// (Markstein) the same float as __fdiv_rn(f, s), and does the modeller's scaled sample  t = rint(q * 64)  come out the
// same?  Compared for EVERY float f (2^32 bit patterns) against every one of the 2 048 step-size mantissas
// s = (1 + m / 2048) * 2^0  (a step size of the codestream has 11 mantissa bits).
//   hipcc -O3 -ffp-contract=off --offload-arch=gfx950 -o /tmp/div_markstein tools/probes/div_markstein.hip && /tmp/div_markstein
// Reported: quotients that differ for 2^-60 <= |f| <= 2^60, scaled samples that differ for |f| <= 2^60 (zero, subnormal and
// tiny f included) and for the rest (huge, infinite, NaN), with the first few cases of each.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
typedef unsigned long long u64;
struct Result { u64 q_diff_in, t_diff_low, t_diff_high; unsigned n_ex; unsigned ex[16][3]; };
__device__ __forceinline__ float quotient3(float f, float s, float r)
{
    const float q = __fmul_rn(f, r);
    const float e = __fmaf_rn(-q, s, f);
    return __fmaf_rn(e, r, q);
}
__global__ __launch_bounds__(256) void k(unsigned first, const float *recip, Result *res)
{
    const unsigned bits = first + blockIdx.x * 256u + threadIdx.x;
    const float f = __uint_as_float(bits);
    const float af = fabsf(f);
    const bool in = af >= 0x1p-60f && af <= 0x1p60f, low = af <= 0x1p60f;
    unsigned qd = 0, tl = 0, th = 0;
    for (unsigned m = 0; m < 2048; ++m) {
        const float s = __uint_as_float(0x3f800000u | (m << 12)), r = recip[m];
        const float q0 = __fdiv_rn(f, s), q1 = quotient3(f, s, r);
        const int t0 = __float2int_rn(__fmul_rn(q0, 64.0f)), t1 = __float2int_rn(__fmul_rn(q1, 64.0f));
        const bool dq = in && __float_as_uint(q0) != __float_as_uint(q1), dt = t0 != t1;
        qd += dq; tl += dt && low; th += dt && !low;
        if (dq || (dt && low)) {
            const unsigned i = atomicAdd(&res->n_ex, 1u);
            if (i < 16) { res->ex[i][0] = bits; res->ex[i][1] = m; res->ex[i][2] = __float_as_uint(q1); }
        }
    }
    if (qd) atomicAdd(&res->q_diff_in, (u64)qd);
    if (tl) atomicAdd(&res->t_diff_low, (u64)tl);
    if (th) atomicAdd(&res->t_diff_high, (u64)th);
}
int main()
{
    static float recip[2048];
    for (unsigned m = 0; m < 2048; ++m) recip[m] = 1.0f / (1.0f + (float)m / 2048.0f); // (IEEE division on the host: correctly rounded)
    float *d_recip = nullptr;
    Result *d_res = nullptr, h;
    if (hipMalloc(reinterpret_cast<void **>(&d_recip), sizeof(recip)) != hipSuccess || hipMalloc(reinterpret_cast<void **>(&d_res), sizeof(Result)) != hipSuccess) return 1;
    if (hipMemcpy(d_recip, recip, sizeof(recip), hipMemcpyHostToDevice) != hipSuccess || hipMemset(d_res, 0, sizeof(Result)) != hipSuccess) return 1;
    const unsigned per_launch = 1u << 26; // 64 launches of 2^26 floats x 2 048 step sizes
    for (unsigned l = 0; l < 64; ++l) {
        hipLaunchKernelGGL(k, dim3(per_launch / 256), dim3(256), 0, 0, l * per_launch, d_recip, d_res);
        if (hipDeviceSynchronize() != hipSuccess) { std::printf("launch %u failed: %s\n", l, hipGetErrorString(hipGetLastError())); return 1; }
        if (l % 8 == 7) { std::printf("floats 0x%08x.. done\n", l * per_launch); std::fflush(stdout); }
    }
    if (hipMemcpy(&h, d_res, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    std::printf("2^32 floats x 2048 step sizes (1 + m/2048):\n");
    std::printf("  quotients that differ from __fdiv_rn, 2^-60 <= |f| <= 2^60 : %llu\n", h.q_diff_in);
    std::printf("  scaled samples that differ, |f| <= 2^60 (zero and tiny too) : %llu\n", h.t_diff_low);
    std::printf("  scaled samples that differ, |f| > 2^60, infinite, NaN       : %llu\n", h.t_diff_high);
    for (unsigned i = 0; i < h.n_ex && i < 16; ++i) {
        float f; std::memcpy(&f, &h.ex[i][0], 4);
        std::printf("  case: f = 0x%08x (%g), m = %u, three-instruction quotient 0x%08x\n", h.ex[i][0], f, h.ex[i][1], h.ex[i][2]);
    }
    return 0;
}
