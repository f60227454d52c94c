// rgba_out.hip -- the decode's output stage straight to R, G, B, A (gfx950).
//
// Replaces, after the inverse DWT, what the host did per pixel on the CPU once the codec channels had arrived (reference:
// RGBAinputFile::ReadFile, src/common/j2k_rgba_file.cpp:450-735 -- sYCC -> RGB :185-278, grey into three channels, the
// palette look-up :72-137, the alpha fill :407-448 -- and DemoteWorld, src/aftereffects/j2k.cpp:482-492).
//
// A thread per destination pixel, a workgroup = 256 neighbours of one row, rows strided over gridDim.y like
// decode_output_kernel.  Reads: component words at (org + x) / sub_x -- a wavefront reads 64 (or, sub-sampled, 32)
// consecutive words of each component.  Writes: in the packed form the pixel's record in one 4- or 8-byte store, so a
// wavefront writes 256 or 512 contiguous bytes (float destinations: one 16-byte store, 1 KiB); in the general form one store per
// given channel at the channel's strides.
// The RGB mode has two more variants that make R, G, B from X'Y'Z' code values (below: "X'Y'Z' -> R'G'B'").
// The build passes -ffp-contract=off: the sYCC arithmetic below rounds every product and every sum on its own.
#include "kernels.h"
#include "out_sample.h"

#include <algorithm>

namespace j2k_hip {
namespace {

// the reference's constants: doubles narrowed to float (j2k_rgba_file.cpp:185-278)
constexpr float kCrR = (float)(2 * (1 - 0.299));
constexpr float kCbB = (float)(2 * (1 - 0.114));
constexpr float kCrG = (float)(2 * 0.299 * (1 - 0.299) / 0.587);
constexpr float kCbG = (float)(2 * 0.114 * (1 - 0.114) / 0.587);

__device__ __forceinline__ unsigned sycc_channel(float f, int h, int top)
{
    return (unsigned)min(max((int)((f + (float)h) + 0.5f), 0), top); // (the cast truncates; |f| < 2^19: always in range)
}

// Float destinations (FLT; out_sample.h: out_float): the pixel's record is four floats -- After Effects' ARGB128 -- stored as one
// 16-byte word, so a wavefront writes 1 KiB of contiguous bytes.  The samples go to their slots by comparisons (no indexed
// register array: nothing lands in scratch memory).
template <typename ARGS>
__device__ __forceinline__ void store_record128(const ARGS &a, int x, int y, const unsigned out[4], int D)
{
    float f[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) f[c] = out_float(out[c], D, a.demote != 0);
    float w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = a.slot[0] == k ? f[0] : (a.slot[1] == k ? f[1] : (a.slot[2] == k ? f[2] : f[3]));
    *reinterpret_cast<float4 *>(a.pix + (long long)y * a.pix_rowbytes + (long long)x * 16) = float4{w[0], w[1], w[2], w[3]};
}

// ---------------------------------------------------------------------------------------------------------------------
// X'Y'Z' -> R'G'B' (j2k_hip_decode_set_xyz_to_rgb; include/j2k_hip.h has the definition to the rounding): the inverse of
// frontend_xyz_kernel, inside the RGB mode.  XYZ, the kernels' compile-time parameter: 0 = off (the kernels as they were, on
// DecRgbaCore), 1 = both tables in LDS, 2 = both tables in global memory.  Per pixel: three reads of the code -> linear light
// table, nine multiplies and six adds rounded one by one, three searches of the threshold table.  The channel is DEFINED as
// the number of thresholds <= r; the search starts from an estimate of top * OETF(r) (hardware log2 / exp2) and walks the
// thresholds until both neighbours agree, so the estimate only decides how many steps it takes, never the result.
// LDS (XYZ 1, component and destination depth <= 12): 2 x 16 KiB copied once per workgroup, which then strides over many rows
// -- the launch keeps the grid small for that, as launch_frontend_xyz does.  Deeper tables (at most 256 KiB each) live in L2.
template <int XYZ> struct RgbaKernelArgs { using type = DecRgbaArgs; };
template <> struct RgbaKernelArgs<0> { using type = DecRgbaCore; };

constexpr int kXyzLdsWords = 4096; // per table: 2^12

// othr[0 .. top): the thresholds of codes 1 .. top, increasing, and othr[top] = +infinity (the table's padding).  Returns how many
// thresholds are <= r (r < 0, out of gamut: 0).
__device__ __forceinline__ unsigned xyz_rgb_code(const float *othr, int top, int target, float r)
{
    int c = 0;
    if (r > 0.0f) { // (a NaN cannot occur: the tables and the matrix are finite)
        float e = r; // target 3: linear light
        if (target == 2) e = __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(r) * (1.0f / 2.4f));
        else if (target == 1) e = r <= 0.0031308f ? 12.92f * r : 1.055f * __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(r) * (1.0f / 2.4f)) - 0.055f;
        e = e < 2.0f ? e : 2.0f; // (keeps the product below within int for every r the matrix can make)
        c = (int)(e * (float)top + 0.5f);
        c = c < 0 ? 0 : (c > top ? top : c);
    }
    // both neighbours of the estimate at once (two independent reads; othr[top] is the table's +infinity): nearly always they agree
    const float hi = othr[c], lo = othr[c > 0 ? c - 1 : 0];
    if (!(hi <= r) && !(c > 0 && lo > r)) return (unsigned)c;
    while (c < top && othr[c] <= r) ++c;
    while (c > 0 && othr[c - 1] > r) --c;
    return (unsigned)c;
}

// R, G, B of depth D from the three component samples (0 .. 2^P - 1 each).  N: the matrix, row by row.
__device__ __forceinline__ void xyz_rgb_pixel(const float *dl, const float *othr, const float *N, int target, int top, const int v[4], unsigned out[4])
{
    const float lx = dl[v[0]], ly = dl[v[1]], lz = dl[v[2]];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float r = __fadd_rn(__fadd_rn(__fmul_rn(N[3 * c], lx), __fmul_rn(N[3 * c + 1], ly)), __fmul_rn(N[3 * c + 2], lz));
        out[c] = xyz_rgb_code(othr, top, target, r);
    }
}

// Both tables into LDS, once per workgroup: dl at s_tab, the thresholds at s_tab + kXyzLdsWords.  (The tables hold
// max(2^depth, 4) words and the depths are <= 12: whole float4s, at most kXyzLdsWords / 4 of them each.)
__device__ __forceinline__ void xyz_tables_to_lds(float4 *s_tab, const float *dl, int P, const float *othr, int D)
{
    const int n_dl = P >= 2 ? (1 << P) >> 2 : 1, n_thr = D >= 2 ? (1 << D) >> 2 : 1;
    for (int i = (int)threadIdx.x; i < n_dl; i += 256) s_tab[i] = reinterpret_cast<const float4 *>(dl)[i];
    for (int i = (int)threadIdx.x; i < n_thr; i += 256) s_tab[kXyzLdsWords / 4 + i] = reinterpret_cast<const float4 *>(othr)[i];
    __syncthreads();
}

template <bool REV, int MODE, bool PACKED, bool FLT, int XYZ = 0>
__global__ __launch_bounds__(256) void decode_rgba_kernel(typename RgbaKernelArgs<XYZ>::type a)
{
    __shared__ unsigned s_lut[MODE == J2K_HIP_RGBA_PALETTE ? 256 : 1];
    if constexpr (MODE == J2K_HIP_RGBA_PALETTE) { // the table, once per workgroup (entries from lut_size on are 0)
        s_lut[threadIdx.x] = a.lut[threadIdx.x];
        __syncthreads();
    }
    __shared__ float4 s_xyz[XYZ == 1 ? 2 * kXyzLdsWords / 4 : 1];
    if constexpr (XYZ == 1) xyz_tables_to_lds(s_xyz, a.xyz_dl, a.cprec[0], a.xyz_othr, a.depth);
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= a.width) return;
    const int D = a.depth, top = (1 << D) - 1;
    const unsigned mask = a.sample_bytes == 1 ? 0xffu : 0xffffu;
    for (int y = blockIdx.y; y < a.height; y += gridDim.y) {
        int v[4];
        component_samples<REV>(a, x, y, v);
        unsigned out[4]; // R, G, B, A
        out[3] = (unsigned)top;
        if constexpr (MODE == J2K_HIP_RGBA_RGB) {
            if constexpr (XYZ == 1) {
                const float *t = reinterpret_cast<const float *>(s_xyz);
                xyz_rgb_pixel(t, t + kXyzLdsWords, a.xyz_n, a.xyz_to_rgb, top, v, out);
            } else if constexpr (XYZ == 2) {
                xyz_rgb_pixel(a.xyz_dl, a.xyz_othr, a.xyz_n, a.xyz_to_rgb, top, v, out);
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) out[c] = depth_out((unsigned)v[c], a.cprec[c], D, mask);
            }
            if (a.alpha_comp == 3) out[3] = depth_out((unsigned)v[3], a.cprec[3], D, mask);
        } else if constexpr (MODE == J2K_HIP_RGBA_GREY) {
            out[0] = out[1] = out[2] = depth_out((unsigned)v[0], a.cprec[0], D, mask);
            if (a.alpha_comp == 1) out[3] = depth_out((unsigned)v[1], a.cprec[1], D, mask);
        } else if constexpr (MODE == J2K_HIP_RGBA_PALETTE) {
            const unsigned idx = (unsigned)v[0];
            const unsigned e = idx < a.lut_size ? s_lut[idx] : 0u;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const unsigned b = (e >> (8 * c)) & 0xffu;
                if constexpr (FLT) out[c] = D <= 8 ? b : ((b << 8) | b); // (a float stands for the integer type that holds its depth)
                else out[c] = a.sample_bytes == 1 ? b : ((b << 8) | b); // ConvertToType: whatever the depth
            }
        } else { // sYCC, the reference's irreversible branch
            const int h = 1 << (D - 1);
            const float sY = (float)((int)depth_out((unsigned)v[0], a.cprec[0], D, mask) - h);
            const float sCb = (float)((int)depth_out((unsigned)v[1], a.cprec[1], D, mask) - h);
            const float sCr = (float)((int)depth_out((unsigned)v[2], a.cprec[2], D, mask) - h);
            out[0] = sycc_channel(sY + kCrR * sCr, h, top);
            out[1] = sycc_channel((sY - kCrG * sCr) - kCbG * sCb, h, top);
            out[2] = sycc_channel(sY + kCbB * sCb, h, top);
        }
        if (a.demote) { // Demote (FrameSeq.cpp:265-268)
#pragma unroll
            for (int c = 0; c < 4; ++c) out[c] = out[c] > 32768u ? ((out[c] - 1) >> 1) + 1 : out[c] >> 1;
        }
        if constexpr (PACKED) {
            if (x < a.dst_w[0] && y < a.dst_h[0]) {
                if constexpr (FLT) {
                    store_record128(a, x, y, out, D);
                } else if (a.sample_bytes == 1) {
                    unsigned w = 0;
#pragma unroll
                    for (int c = 0; c < 4; ++c) w |= (out[c] & 0xffu) << (8 * a.slot[c]);
                    *reinterpret_cast<unsigned *>(a.pix + (long long)y * a.pix_rowbytes + (long long)x * 4) = w;
                } else {
                    unsigned long long w = 0;
#pragma unroll
                    for (int c = 0; c < 4; ++c) w |= (unsigned long long)(out[c] & 0xffffu) << (16 * a.slot[c]);
                    *reinterpret_cast<unsigned long long *>(a.pix + (long long)y * a.pix_rowbytes + (long long)x * 8) = w;
                }
            }
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (a.dst[c] && x < a.dst_w[c] && y < a.dst_h[c]) {
                    uint8_t *p = a.dst[c] + (long long)y * a.rowbytes[c] + (long long)x * a.colbytes[c];
                    if constexpr (FLT) store_float(p, out[c], D, a.demote != 0);
                    else if (a.sample_bytes == 1) *p = (uint8_t)out[c];
                    else *reinterpret_cast<unsigned short *>(p) = (unsigned short)out[c];
                }
        }
    }
}

template <bool REV, int MODE>
void launch_form(const DecRgbaArgs &a, const dim3 &grid, hipStream_t s)
{
    if (a.sample_bytes == 4) {
        if (a.packed) hipLaunchKernelGGL((decode_rgba_kernel<REV, MODE, true, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((decode_rgba_kernel<REV, MODE, false, true>), grid, dim3(256), 0, s, a);
    } else if (a.packed) hipLaunchKernelGGL((decode_rgba_kernel<REV, MODE, true, false>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((decode_rgba_kernel<REV, MODE, false, false>), grid, dim3(256), 0, s, a);
}

template <bool REV, int XYZ>
void launch_form_xyz(const DecRgbaArgs &a, const dim3 &grid, hipStream_t s)
{
    constexpr int M = J2K_HIP_RGBA_RGB;
    if (a.sample_bytes == 4) {
        if (a.packed) hipLaunchKernelGGL((decode_rgba_kernel<REV, M, true, true, XYZ>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((decode_rgba_kernel<REV, M, false, true, XYZ>), grid, dim3(256), 0, s, a);
    } else if (a.packed) hipLaunchKernelGGL((decode_rgba_kernel<REV, M, true, false, XYZ>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((decode_rgba_kernel<REV, M, false, false, XYZ>), grid, dim3(256), 0, s, a);
}

// Whether the X'Y'Z' -> R'G'B' tables of these arguments fit LDS (the XYZ = 1 variants), and the grid of those variants:
// about as many workgroups as the chip holds at once, each striding over its rows, so that the copy of the tables is amortised.
bool xyz_in_lds(const DecRgbaArgs &a) { return a.cprec[0] <= 12 && a.depth <= 12; }
dim3 xyz_lds_grid(const DecRgbaArgs &a, int nframes)
{
    const int gx = (a.width + 255) / 256, per = gx * nframes, gy = per >= 2048 ? 1 : 2048 / per;
    return dim3((unsigned)gx, (unsigned)std::min(a.height, gy), (unsigned)nframes);
}

template <bool REV>
void launch_mode(const DecRgbaArgs &a, const dim3 &grid, hipStream_t s)
{
    if (a.xyz_to_rgb) { // (mode RGB: decode_rgba_args)
        if (xyz_in_lds(a)) launch_form_xyz<REV, 1>(a, xyz_lds_grid(a, 1), s);
        else launch_form_xyz<REV, 2>(a, grid, s);
        return;
    }
    switch (a.mode) {
    case J2K_HIP_RGBA_RGB: launch_form<REV, J2K_HIP_RGBA_RGB>(a, grid, s); break;
    case J2K_HIP_RGBA_GREY: launch_form<REV, J2K_HIP_RGBA_GREY>(a, grid, s); break;
    case J2K_HIP_RGBA_PALETTE: launch_form<REV, J2K_HIP_RGBA_PALETTE>(a, grid, s); break;
    default: launch_form<REV, J2K_HIP_RGBA_SYCC>(a, grid, s); break;
    }
}

// One pixel of decode_rgba_kernel (that kernel's own lines as a function, for its sequence form below).
// XYZ != 0: the tables (in LDS or in global memory), the matrix and the target of the X'Y'Z' -> R'G'B' conversion.
struct RgbaXyzRefs { const float *dl, *othr, *n; int target; };

template <bool REV, int MODE, bool PACKED, bool FLT, int XYZ, typename ARGS>
__device__ __forceinline__ void rgba_pixel(const ARGS &a, const unsigned *s_lut, const RgbaXyzRefs &z, int x, int y, int D, int top, unsigned mask)
{
    int v[4];
    component_samples<REV>(a, x, y, v);
    unsigned out[4]; // R, G, B, A
    out[3] = (unsigned)top;
    if constexpr (MODE == J2K_HIP_RGBA_RGB) {
        if constexpr (XYZ != 0) {
            xyz_rgb_pixel(z.dl, z.othr, z.n, z.target, top, v, out);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) out[c] = depth_out((unsigned)v[c], a.cprec[c], D, mask);
        }
        if (a.alpha_comp == 3) out[3] = depth_out((unsigned)v[3], a.cprec[3], D, mask);
    } else if constexpr (MODE == J2K_HIP_RGBA_GREY) {
        out[0] = out[1] = out[2] = depth_out((unsigned)v[0], a.cprec[0], D, mask);
        if (a.alpha_comp == 1) out[3] = depth_out((unsigned)v[1], a.cprec[1], D, mask);
    } else if constexpr (MODE == J2K_HIP_RGBA_PALETTE) {
        const unsigned idx = (unsigned)v[0];
        const unsigned e = idx < a.lut_size ? s_lut[idx] : 0u;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned b = (e >> (8 * c)) & 0xffu;
            if constexpr (FLT) out[c] = D <= 8 ? b : ((b << 8) | b); // (a float stands for the integer type that holds its depth)
            else out[c] = a.sample_bytes == 1 ? b : ((b << 8) | b); // ConvertToType: whatever the depth
        }
    } else { // sYCC, the reference's irreversible branch
        const int h = 1 << (D - 1);
        const float sY = (float)((int)depth_out((unsigned)v[0], a.cprec[0], D, mask) - h);
        const float sCb = (float)((int)depth_out((unsigned)v[1], a.cprec[1], D, mask) - h);
        const float sCr = (float)((int)depth_out((unsigned)v[2], a.cprec[2], D, mask) - h);
        out[0] = sycc_channel(sY + kCrR * sCr, h, top);
        out[1] = sycc_channel((sY - kCrG * sCr) - kCbG * sCb, h, top);
        out[2] = sycc_channel(sY + kCbB * sCb, h, top);
    }
    if (a.demote) { // Demote (FrameSeq.cpp:265-268)
#pragma unroll
        for (int c = 0; c < 4; ++c) out[c] = out[c] > 32768u ? ((out[c] - 1) >> 1) + 1 : out[c] >> 1;
    }
    if constexpr (PACKED) {
        if (x < a.dst_w[0] && y < a.dst_h[0]) {
            if constexpr (FLT) {
                store_record128(a, x, y, out, D);
            } else if (a.sample_bytes == 1) {
                unsigned w = 0;
#pragma unroll
                for (int c = 0; c < 4; ++c) w |= (out[c] & 0xffu) << (8 * a.slot[c]);
                *reinterpret_cast<unsigned *>(a.pix + (long long)y * a.pix_rowbytes + (long long)x * 4) = w;
            } else {
                unsigned long long w = 0;
#pragma unroll
                for (int c = 0; c < 4; ++c) w |= (unsigned long long)(out[c] & 0xffffu) << (16 * a.slot[c]);
                *reinterpret_cast<unsigned long long *>(a.pix + (long long)y * a.pix_rowbytes + (long long)x * 8) = w;
            }
        }
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (a.dst[c] && x < a.dst_w[c] && y < a.dst_h[c]) {
                uint8_t *p = a.dst[c] + (long long)y * a.rowbytes[c] + (long long)x * a.colbytes[c];
                if constexpr (FLT) store_float(p, out[c], D, a.demote != 0);
                else if (a.sample_bytes == 1) *p = (uint8_t)out[c];
                else *reinterpret_cast<unsigned short *>(p) = (unsigned short)out[c];
            }
    }
}

// The frames of a sequence decode in one launch: frame = blockIdx.z, its descriptor (kernels.h: DecSeqFrameDev) read from the
// table at a wave-uniform address (scalar loads, once per workgroup).  The pixel code reads a frame's arguments: DecRgbaArgs
// without the palette (which stays where the launch put it: a copy of the whole struct would live in scratch memory).
struct RgbaFrameArgs {
    const void *comp[4]; long long stride;
    int ncomp, mct, cprec[4], sub_x[4], sub_y[4], org_x, org_y;
    int alpha_comp, sample_bytes, demote, slot[4];
    uint8_t *pix; long long pix_rowbytes;
    uint8_t *dst[4]; long long colbytes[4], rowbytes[4];
    int dst_w[4], dst_h[4];
    uint32_t lut_size;
};

template <bool REV, int MODE, bool PACKED, bool FLT, int XYZ = 0>
__global__ __launch_bounds__(256) void decode_rgba_seq_kernel(typename RgbaKernelArgs<XYZ>::type a, const DecSeqFrameDev *__restrict__ frames)
{
    __shared__ unsigned s_lut[MODE == J2K_HIP_RGBA_PALETTE ? 256 : 1];
    if constexpr (MODE == J2K_HIP_RGBA_PALETTE) {
        s_lut[threadIdx.x] = a.lut[threadIdx.x];
        __syncthreads();
    }
    __shared__ float4 s_xyz[XYZ == 1 ? 2 * kXyzLdsWords / 4 : 1];
    RgbaXyzRefs z{nullptr, nullptr, nullptr, 0};
    if constexpr (XYZ == 1) {
        xyz_tables_to_lds(s_xyz, a.xyz_dl, a.cprec[0], a.xyz_othr, a.depth);
        const float *t = reinterpret_cast<const float *>(s_xyz);
        z = RgbaXyzRefs{t, t + kXyzLdsWords, a.xyz_n, a.xyz_to_rgb};
    } else if constexpr (XYZ == 2) z = RgbaXyzRefs{a.xyz_dl, a.xyz_othr, a.xyz_n, a.xyz_to_rgb};
    const DecSeqFrameDev &F = frames[blockIdx.z];
    RgbaFrameArgs f;
    f.stride = a.stride; f.ncomp = a.ncomp; f.mct = a.mct; f.org_x = a.org_x; f.org_y = a.org_y;
    f.alpha_comp = a.alpha_comp; f.sample_bytes = a.sample_bytes; f.demote = a.demote; f.lut_size = a.lut_size;
    f.pix = F.pix; f.pix_rowbytes = F.pix_rowbytes;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        f.comp[c] = reinterpret_cast<const unsigned *>(a.comp[c]) + F.comp_off;
        f.cprec[c] = a.cprec[c]; f.sub_x[c] = a.sub_x[c]; f.sub_y[c] = a.sub_y[c]; f.slot[c] = a.slot[c];
        f.dst[c] = F.dst[c]; f.colbytes[c] = F.colbytes[c]; f.rowbytes[c] = F.rowbytes[c];
        f.dst_w[c] = F.dst_w[c]; f.dst_h[c] = F.dst_h[c];
    }
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= a.width) return;
    const int D = a.depth, top = (1 << D) - 1;
    const unsigned mask = a.sample_bytes == 1 ? 0xffu : 0xffffu;
    for (int y = blockIdx.y; y < a.height; y += gridDim.y) rgba_pixel<REV, MODE, PACKED, FLT, XYZ>(f, s_lut, z, x, y, D, top, mask);
}

template <bool REV, int MODE>
void launch_form_seq(const DecRgbaArgs &a, const DecSeqFrameDev *f, const dim3 &grid, hipStream_t s)
{
    if (a.sample_bytes == 4) {
        if (a.packed) hipLaunchKernelGGL((decode_rgba_seq_kernel<REV, MODE, true, true>), grid, dim3(256), 0, s, a, f);
        else hipLaunchKernelGGL((decode_rgba_seq_kernel<REV, MODE, false, true>), grid, dim3(256), 0, s, a, f);
    } else if (a.packed) hipLaunchKernelGGL((decode_rgba_seq_kernel<REV, MODE, true, false>), grid, dim3(256), 0, s, a, f);
    else hipLaunchKernelGGL((decode_rgba_seq_kernel<REV, MODE, false, false>), grid, dim3(256), 0, s, a, f);
}

template <bool REV, int XYZ>
void launch_form_seq_xyz(const DecRgbaArgs &a, const DecSeqFrameDev *f, const dim3 &grid, hipStream_t s)
{
    constexpr int M = J2K_HIP_RGBA_RGB;
    if (a.sample_bytes == 4) {
        if (a.packed) hipLaunchKernelGGL((decode_rgba_seq_kernel<REV, M, true, true, XYZ>), grid, dim3(256), 0, s, a, f);
        else hipLaunchKernelGGL((decode_rgba_seq_kernel<REV, M, false, true, XYZ>), grid, dim3(256), 0, s, a, f);
    } else if (a.packed) hipLaunchKernelGGL((decode_rgba_seq_kernel<REV, M, true, false, XYZ>), grid, dim3(256), 0, s, a, f);
    else hipLaunchKernelGGL((decode_rgba_seq_kernel<REV, M, false, false, XYZ>), grid, dim3(256), 0, s, a, f);
}

template <bool REV>
void launch_mode_seq(const DecRgbaArgs &a, const DecSeqFrameDev *f, const dim3 &grid, hipStream_t s)
{
    if (a.xyz_to_rgb) { // (mode RGB: decode_rgba_args)
        if (xyz_in_lds(a)) launch_form_seq_xyz<REV, 1>(a, f, xyz_lds_grid(a, (int)grid.z), s);
        else launch_form_seq_xyz<REV, 2>(a, f, grid, s);
        return;
    }
    switch (a.mode) {
    case J2K_HIP_RGBA_RGB: launch_form_seq<REV, J2K_HIP_RGBA_RGB>(a, f, grid, s); break;
    case J2K_HIP_RGBA_GREY: launch_form_seq<REV, J2K_HIP_RGBA_GREY>(a, f, grid, s); break;
    case J2K_HIP_RGBA_PALETTE: launch_form_seq<REV, J2K_HIP_RGBA_PALETTE>(a, f, grid, s); break;
    default: launch_form_seq<REV, J2K_HIP_RGBA_SYCC>(a, f, grid, s); break;
    }
}

} // namespace

void launch_decode_rgba(const DecRgbaArgs &a, hipStream_t s)
{
    if (a.width <= 0 || a.height <= 0) return;
    const dim3 grid((unsigned)((a.width + 255) / 256), (unsigned)std::min(a.height, 65535), 1);
    if (a.reversible) launch_mode<true>(a, grid, s);
    else launch_mode<false>(a, grid, s);
}

void launch_decode_rgba_seq(const DecRgbaArgs &a, const DecSeqFrameDev *frames, int nframes, hipStream_t s)
{
    if (a.width <= 0 || a.height <= 0 || nframes <= 0) return;
    const dim3 grid((unsigned)((a.width + 255) / 256), (unsigned)std::min(a.height, 65535), (unsigned)nframes);
    if (a.reversible) launch_mode_seq<true>(a, frames, grid, s);
    else launch_mode_seq<false>(a, frames, grid, s);
}

} // namespace j2k_hip
