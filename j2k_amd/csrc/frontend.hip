// frontend.hip -- fused sample front end for gfx950 (HBM-bound, one pass over the frame).
//
// Replaces, in one kernel:
//   A1  PromoteWorld/Promote           reference: src/aftereffects/FrameSeq.cpp:311-355
//   A2  Codec::CopyBuffer/CopyChannel  reference: src/common/j2k_codec.cpp:222-427
//   A4  DC level shift                 T.800 G.1  (OpenJPEG tcd.c, reached from opj_encode,
//   A5  RCT / ICT                      T.800 G.2 / G.3          j2k_openjpeg_codec.cpp:730)
// Algorithmic bytes per pixel: 4*S read (S = bytes per sample, interleaved ARGB; 4 for a float world) + 4*Ncomp written.
// When the frame has the After Effects layout and 1 or 3 components, this stage is fused into the
// level-1 DWT kernel instead (dwt.hip) and this kernel is not launched at all.
// A second kernel (frontend_sycc_kernel, below) makes Y, Cb, Cr from R, G, B and decimates the chroma as it loads it.
// A third (frontend_xyz_kernel) makes cinema X'Y'Z' code values from R'G'B' by table, matrix and threshold search.
#include "frontend_ops.h"

#include <type_traits>

namespace j2k_hip {
namespace {

// FLT: the frame has 32-bit float channels (fe_load: quantised as they are loaded); everything behind the load is one text.
template <bool REV, bool FLT>
__global__ __launch_bounds__(256) void frontend_kernel(FrontendArgs a)
{
    using T = typename std::conditional<REV, int, float>::type;
    const int x = a.x0 + (int)(blockIdx.x * 256 + threadIdx.x);
    if (x >= a.width) return;
    for (int y = a.y0 + (int)blockIdx.y; y < a.y1; y += (int)gridDim.y) {
        unsigned raw[4] = {0, 0, 0, 0};
        fe_load<FLT>(a, x, y, raw);
        T v[4];
        fe_convert<REV, T>(a, raw, v);
        const long long o = (long long)(y - a.dst_y0) * a.dst_stride + (x - a.dst_x0);
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < a.ncomp) reinterpret_cast<T *>(a.dst[c])[o] = v[c];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// RGB -> Y Cb Cr with chroma decimation (j2k_hip_params.rgb_to_sycc): the analysis to the replicating sYCC read of the decode's
// RGBA output kernel.  One lane = one chroma sample = SX x SY pixels: it loads each of them once (the interleaved pixel as one
// 4- or 8-byte word, or the strided samples), applies Promote and the depth conversion, writes their Y (and A) -- SX adjacent
// words of a row, one 8-byte store for SX = 2 -- and one Cb and one Cr.  Lanes run along the row, so a wave's loads and stores
// cover contiguous bytes; nothing of full size but Y (and A) is ever written.  A pixel beyond the right or bottom edge repeats
// the last column or row -- out of the registers that hold it, not out of memory.
// Exact integer arithmetic (include/j2k_hip.h): Y's sum stays below 2^32, a pixel's chroma term within +-2^31, the sum over up
// to four pixels in 64 bits; the shift is arithmetic (floor).  The float planes of the 9/7 path receive the same integers.
// Algorithmic bytes per pixel: 4*S read + 4*(1 [+ 1 alpha] + 2 / (SX*SY)) written.

template <bool REV, int SX, int SY, bool FLT>
__global__ __launch_bounds__(256) void frontend_sycc_kernel(FrontendArgs a)
{
    using T = typename std::conditional<REV, int, float>::type;
    constexpr int K = (SX == 2 ? 1 : 0) + (SY == 2 ? 1 : 0);
    const int cw = (a.width + SX - 1) / SX, ch = (a.y1 + SY - 1) / SY;
    const int cx = (int)(blockIdx.x * 256 + threadIdx.x);
    if (cx >= cw) return;
    const int dc = 1 << (a.prec - 1), top = (1 << a.prec) - 1;
    const bool alpha = a.ncomp == 4;
    T *const dy = reinterpret_cast<T *>(a.dst[0]), *const dcb = reinterpret_cast<T *>(a.dst[1]), *const dcr = reinterpret_cast<T *>(a.dst[2]);
    T *const da = reinterpret_cast<T *>(a.dst[3]);
    for (int cy = (int)blockIdx.y; cy < ch; cy += (int)gridDim.y) {
        long long scb = 0, scr = 0, rcb = 0, rcr = 0;
#pragma unroll
        for (int j = 0; j < SY; ++j) {
            const int y = cy * SY + j;
            if (y < a.y1) { // (a row below the image repeats the sums of the row above it)
                rcb = 0; rcr = 0;
                T yv[SX], av[SX];
                long long pcb = 0, pcr = 0;
#pragma unroll
                for (int i = 0; i < SX; ++i) {
                    const int x = cx * SX + i;
                    if (x < a.width) { // (a column right of the image repeats the pixel left of it)
                        unsigned raw[4] = {0, 0, 0, 0};
                        fe_load<FLT>(a, x, y, raw);
                        const int r = fe_sample(a, 0, raw[0]), g = fe_sample(a, 1, raw[1]), b = fe_sample(a, 2, raw[2]);
                        const unsigned yy = (19595u * (unsigned)r + 38470u * (unsigned)g + 7471u * (unsigned)b + 32768u) >> 16;
                        yv[i] = (T)((int)yy - dc);
                        av[i] = alpha ? (T)(fe_sample(a, 3, raw[3]) - dc) : (T)0;
                        pcb = -11059LL * r - 21709LL * g + 32768LL * b;
                        pcr = 32768LL * r - 27439LL * g - 5329LL * b;
                    }
                    rcb += pcb; rcr += pcr;
                }
                const long long o = (long long)y * a.dst_stride + (long long)cx * SX;
                if constexpr (SX == 2) {
                    if (cx * 2 + 1 < a.width) { // (dst_stride is even and the planes are 8-byte aligned)
                        using T2 = typename std::conditional<REV, int2, float2>::type;
                        *reinterpret_cast<T2 *>(dy + o) = T2{yv[0], yv[1]};
                        if (alpha) *reinterpret_cast<T2 *>(da + o) = T2{av[0], av[1]};
                    } else {
                        dy[o] = yv[0];
                        if (alpha) da[o] = av[0];
                    }
                } else {
                    dy[o] = yv[0];
                    if (alpha) da[o] = av[0];
                }
            }
            scb += rcb; scr += rcr;
        }
        const long long half = 1LL << (15 + K);
        long long cb = dc + ((scb + half) >> (16 + K)), cr = dc + ((scr + half) >> (16 + K));
        cb = cb < 0 ? 0 : (cb > top ? top : cb);
        cr = cr < 0 ? 0 : (cr > top ? top : cr);
        const long long oc = (long long)cy * a.dst_stride + cx;
        dcb[oc] = (T)((int)cb - dc);
        dcr[oc] = (T)((int)cr - dc);
    }
}

template <bool REV, bool FLT>
void launch_sycc(const FrontendArgs &a, int sub_x, int sub_y, dim3 grid, hipStream_t s)
{
    if (sub_x == 1 && sub_y == 1) hipLaunchKernelGGL((frontend_sycc_kernel<REV, 1, 1, FLT>), grid, dim3(256), 0, s, a);
    else if (sub_x == 2 && sub_y == 1) hipLaunchKernelGGL((frontend_sycc_kernel<REV, 2, 1, FLT>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((frontend_sycc_kernel<REV, 2, 2, FLT>), grid, dim3(256), 0, s, a);
}

// ---------------------------------------------------------------------------------------------------------------------
// R'G'B' -> X'Y'Z' code values (j2k_hip_params.rgb_to_xyz; include/j2k_hip.h has the definition to the rounding).  One lane per
// pixel along the row, rows by grid-y striding, as frontend_kernel.  Per pixel: three reads of the linear-light tables (global
// memory, at most 256 KiB each: they live in L2), nine multiplies and six adds rounded one by one, and three searches of the
// threshold table.  The code is DEFINED as the number of thresholds <= X; the search starts from an estimate of
// top * X^(1/2.6) (hardware log2 / exp2, good to a fraction of a code) and walks the thresholds until both neighbours agree, so
// the estimate's accuracy only decides how many steps it takes -- usually none or one -- never the result.
// LDS: the thresholds (prec <= 12: at most 16 KiB) are copied into LDS once per workgroup, which strides over many rows (the
// launch keeps the grid small for that); deeper destinations search the table in global memory.
// Algorithmic bytes per pixel: 4*S read + 4*Ncomp written (ARGB64 -> three planes: 8 + 12).

// thr[0 .. top): the thresholds of codes 1 .. top, increasing.  Returns how many are <= x.
__device__ __forceinline__ int xyz_code(const float *thr, int top, float x)
{
    int c = (int)(__builtin_amdgcn_exp2f(__builtin_amdgcn_logf(x) * (1.0f / 2.6f)) * (float)top + 0.5f); // (v_log_f32 / v_exp_f32; x = 0: log2 = -inf, exp2 = 0)
    c = c < 0 ? 0 : (c > top ? top : c);
    while (c < top && thr[c] <= x) ++c;
    while (c > 0 && thr[c - 1] > x) --c;
    return c;
}

template <bool REV, bool FLT, bool LDS>
__global__ __launch_bounds__(256) void frontend_xyz_kernel(FrontendArgs a)
{
    using T = typename std::conditional<REV, int, float>::type;
    __shared__ float4 sthr[LDS ? 1024 : 1];
    const int top = (1 << a.prec) - 1, dc = 1 << (a.prec - 1);
    if constexpr (LDS) { // (the table holds max(2^prec, 4) words -- the thresholds, then +inf -- and prec <= 12: at most 1024 x 16 bytes)
        const int n4 = top >= 3 ? (top + 1) >> 2 : 1;
        for (int i = (int)threadIdx.x; i < n4; i += 256) sthr[i] = reinterpret_cast<const float4 *>(a.xyz_thr)[i];
        __syncthreads();
    }
    const int x = a.x0 + (int)(blockIdx.x * 256 + threadIdx.x);
    if (x >= a.width) return;
    for (int y = a.y0 + (int)blockIdx.y; y < a.y1; y += (int)gridDim.y) {
        unsigned raw[4] = {0, 0, 0, 0};
        fe_load<FLT>(a, x, y, raw);
        float l[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            unsigned v = raw[c];
            if (a.promote && a.sample_bytes[c] == 2) v = promote16(v);
            const unsigned vmax = (1u << a.src_depth[c]) - 1u;
            l[c] = a.xyz_lin[c][v > vmax ? vmax : v];
        }
        int s[4] = {0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float X = __fadd_rn(__fadd_rn(__fmul_rn(a.xyz_m[3 * c], l[0]), __fmul_rn(a.xyz_m[3 * c + 1], l[1])), __fmul_rn(a.xyz_m[3 * c + 2], l[2]));
            if constexpr (LDS) s[c] = xyz_code(reinterpret_cast<const float *>(sthr), top, X) - dc;
            else s[c] = xyz_code(a.xyz_thr, top, X) - dc;
        }
        if (a.ncomp == 4) s[3] = fe_sample(a, 3, raw[3]) - dc;
        T v[4];
        fe_colour<REV, T>(a, s, v);
        const long long o = (long long)(y - a.dst_y0) * a.dst_stride + (x - a.dst_x0);
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < a.ncomp) reinterpret_cast<T *>(a.dst[c])[o] = v[c];
    }
}

template <bool REV, bool FLT>
void launch_xyz(const FrontendArgs &a, dim3 grid, hipStream_t s)
{
    if (a.prec <= 12) hipLaunchKernelGGL((frontend_xyz_kernel<REV, FLT, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((frontend_xyz_kernel<REV, FLT, false>), grid, dim3(256), 0, s, a);
}

bool has_float(const FrontendArgs &a)
{
    for (int c = 0; c < a.ncomp; ++c)
        if (a.sample_bytes[c] == 4) return true;
    return false;
}

} // namespace

void launch_frontend_sycc(const FrontendArgs &a, int sub_x, int sub_y, hipStream_t s)
{
    if (a.y1 <= 0 || a.width <= 0) return;
    const int cw = (a.width + sub_x - 1) / sub_x, ch = (a.y1 + sub_y - 1) / sub_y;
    dim3 grid((unsigned)((cw + 255) / 256), (unsigned)(ch < 65535 ? ch : 65535), 1);
    if (has_float(a)) {
        if (a.reversible) launch_sycc<true, true>(a, sub_x, sub_y, grid, s);
        else launch_sycc<false, true>(a, sub_x, sub_y, grid, s);
    } else if (a.reversible) launch_sycc<true, false>(a, sub_x, sub_y, grid, s);
    else launch_sycc<false, false>(a, sub_x, sub_y, grid, s);
}

void launch_frontend_xyz(const FrontendArgs &a, hipStream_t s)
{
    if (a.y1 <= a.y0 || a.width <= a.x0) return;
    const int rows = a.y1 - a.y0;
    // a workgroup copies the thresholds once and then strides over its rows: about as many workgroups as the chip holds at once
    const int gx = (a.width - a.x0 + 255) / 256, gy = gx >= 2048 ? 1 : 2048 / gx;
    dim3 grid((unsigned)gx, (unsigned)(rows < gy ? rows : gy), 1);
    if (has_float(a)) {
        if (a.reversible) launch_xyz<true, true>(a, grid, s);
        else launch_xyz<false, true>(a, grid, s);
    } else if (a.reversible) launch_xyz<true, false>(a, grid, s);
    else launch_xyz<false, false>(a, grid, s);
}

void launch_frontend(const FrontendArgs &a, hipStream_t s)
{
    if (a.y1 <= a.y0 || a.width <= a.x0) return;
    const int rows = a.y1 - a.y0;
    dim3 grid((unsigned)((a.width - a.x0 + 255) / 256), (unsigned)(rows < 65535 ? rows : 65535), 1);
    if (has_float(a)) {
        if (a.reversible) hipLaunchKernelGGL((frontend_kernel<true, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((frontend_kernel<false, true>), grid, dim3(256), 0, s, a);
    } else if (a.reversible) hipLaunchKernelGGL((frontend_kernel<true, false>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((frontend_kernel<false, false>), grid, dim3(256), 0, s, a);
}

} // namespace j2k_hip
