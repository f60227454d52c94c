// frontend_ops.h -- per-pixel arithmetic of the sample front end, shared by frontend.hip and the
// fused front-end + level-1 DWT kernel in dwt.hip (one definition = one rounding behaviour).
//   A1 Promote              reference: src/aftereffects/FrameSeq.cpp:311-314
//   A2 CopyChannel shifts   reference: src/common/j2k_codec.cpp:254-371
//   A4 DC level shift, A5 RCT / ICT   T.800 G.1-G.3
//   A0 float worlds         reference: src/aftereffects/FrameSeq.cpp:95-110 (CopyWorldIterate<PF_FpShort, ...>), FrameSeq.h:47
#pragma once

#include "kernels.h"

namespace j2k_hip {

// Promote() returns A_u_short: the result wraps to 16 bits
__device__ __forceinline__ unsigned promote16(unsigned v) { return (v > 16384u ? ((v - 1u) << 1) + 1u : v << 1) & 0xffffu; }

// CopyChannel<int,SRC>: bitShift = dest.depth - src.depth
__device__ __forceinline__ unsigned depth_convert(unsigned v, int src_depth, int dst_depth)
{
    const int shift = dst_depth - src_depth;
    if (shift == 0) return v;
    if (shift < 0) return v >> (-shift);
    if (src_depth >= 8) {
        if (shift <= src_depth) return (v << shift) | (v >> (src_depth - shift));
        const int second = shift - src_depth;
        const unsigned t = (v << src_depth) | v;
        return (t << second) | (t >> (src_depth * 2 - second));
    }
    unsigned pd = (unsigned)src_depth, t = v;
    while (pd * 2 < (unsigned)dst_depth) { t = (t << pd) | t; pd *= 2; }
    const int second = dst_depth - (int)pd;
    return (t << second) | (t >> ((int)pd - second));
}

// A 32-bit float sample of nominal range 0..1 as the unsigned integer of depth d that it stands for (include/j2k_hip.h): the
// one definition of that rounding.  NaN, -0.0, negatives and -inf fail both comparisons and give 0, +inf gives 2^d - 1.  The
// product and the sum are each rounded to binary32 (-ffp-contract=off), the cast truncates a value in 0 .. 65535.5.
// promote (d = 16): the After Effects 15+1-bit value the float world converts to (x 32768), then Promote.
__device__ __forceinline__ unsigned fe_quantise_float(float x, int d, bool promote)
{
    const float t = x > 1.0f ? 1.0f : (x > 0.0f ? x : 0.0f);
    if (promote) return promote16((unsigned)(t * 32768.0f + 0.5f));
    return (unsigned)(t * (float)((1 << d) - 1) + 0.5f);
}

// raw = sample of codec channel c as stored (fe_load); the unsigned sample of a.prec bits it stands for: Promote and the depth
// conversion, before the DC shift and any colour transform (the Y Cb Cr front end and the compare kernel work on these).
__device__ __forceinline__ int fe_sample(const FrontendArgs &a, int c, unsigned raw)
{
    if (a.promote && a.sample_bytes[c] == 2) raw = promote16(raw);
    return (int)depth_convert(raw, a.src_depth[c], a.prec);
}

// s[c] = DC-shifted sample of component c; out[c] = the component value after the colour transform (RCT for the reversible
// path, ICT otherwise) on components 0..2 when a.mct is set: the one text of both transforms (fe_convert, the X'Y'Z' front end).
template <bool REV, typename T>
__device__ __forceinline__ void fe_colour(const FrontendArgs &a, int s[4], T out[4])
{
    if constexpr (REV) {
        if (a.mct) {
            const int r = s[0], g = s[1], b = s[2];
            s[0] = (r + 2 * g + b) >> 2;
            s[1] = b - g;
            s[2] = r - g;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) out[c] = s[c];
    } else {
        float f[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) f[c] = (float)s[c];
        if (a.mct) {
            const float r = f[0], g = f[1], b = f[2];
            // every product and every sum individually rounded to float32, left to right (the
            // library is built with -ffp-contract=off): bit-identical to the oracle's SSE2 arithmetic
            f[0] = (0.299f * r + 0.587f * g) + 0.114f * b;
            f[1] = (-0.16875f * r + -0.331260f * g) + 0.5f * b;
            f[2] = (0.5f * r + -0.41869f * g) + -0.08131f * b;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) out[c] = f[c];
    }
}

// raw[c] = sample of codec channel c as stored (a float sample: as quantised, Promote included); out[c] = component value after promote, depth
// conversion, DC shift and colour transform (int for the reversible path, float otherwise).
template <bool REV, typename T>
__device__ __forceinline__ void fe_convert(const FrontendArgs &a, const unsigned raw[4], T out[4])
{
    int s[4] = {0, 0, 0, 0};
    const int dc = 1 << (a.prec - 1);
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (c < a.ncomp) {
            unsigned t = raw[c];
            if (a.promote && a.sample_bytes[c] == 2) t = promote16(t);
            s[c] = (int)depth_convert(t, a.src_depth[c], a.prec) - dc;
        }
    fe_colour<REV, T>(a, s, out);
}

// the samples of codec channels 0..ncomp-1 from one interleaved pixel (After Effects layout)
__device__ __forceinline__ void fe_unpack64(const FrontendArgs &a, uint2 q, unsigned raw[4])
{
    const unsigned s[4] = {q.x & 0xffffu, q.x >> 16, q.y & 0xffffu, q.y >> 16};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int k = a.chan_off[c] >> 1;
        raw[c] = k == 0 ? s[0] : (k == 1 ? s[1] : (k == 2 ? s[2] : s[3]));
    }
}
__device__ __forceinline__ void fe_unpack32(const FrontendArgs &a, unsigned q, unsigned raw[4])
{
#pragma unroll
    for (int c = 0; c < 4; ++c) raw[c] = (q >> (8 * a.chan_off[c])) & 0xffu;
}
// one ARGB128 pixel (four floats, one 16-byte load per lane: a wave reads 1 KiB of contiguous bytes), quantised
__device__ __forceinline__ void fe_unpack128(const FrontendArgs &a, uint4 q, unsigned raw[4])
{
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int k = a.chan_off[c] >> 2;
        const unsigned bits = k == 0 ? q.x : (k == 1 ? q.y : (k == 2 ? q.z : q.w));
        raw[c] = c < a.ncomp ? fe_quantise_float(__uint_as_float(bits), a.src_depth[c], a.promote != 0) : 0u;
    }
}

// The stored samples of pixel (x, y) of codec channels 0 .. ncomp - 1.  FLT: the frame has float channels -- an interleaved
// pixel is ARGB128, a strided sample is loaded by its own width (1, 2 or 4 bytes).  Without FLT the text is what the kernels
// held before float samples existed, so their code does not change.
template <bool FLT>
__device__ __forceinline__ void fe_load(const FrontendArgs &a, int x, int y, unsigned raw[4])
{
    if (a.interleaved) {
        const uint8_t *p = a.pixel_base + (long long)y * a.rowbytes[0] + (long long)x * a.pixel_bytes;
        if constexpr (FLT) {
            fe_unpack128(a, *reinterpret_cast<const uint4 *>(p), raw);
        } else {
            if (a.pixel_bytes == 8) fe_unpack64(a, *reinterpret_cast<const uint2 *>(p), raw); // one ARGB64 pixel
            else fe_unpack32(a, *reinterpret_cast<const unsigned *>(p), raw);                  // one ARGB32 pixel
        }
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < a.ncomp) {
                const uint8_t *p = a.src[c] + (long long)y * a.rowbytes[c] + (long long)x * a.colbytes[c];
                if constexpr (FLT) {
                    if (a.sample_bytes[c] == 4) raw[c] = fe_quantise_float(*reinterpret_cast<const float *>(p), a.src_depth[c], a.promote != 0);
                    else raw[c] = a.sample_bytes[c] == 2 ? *reinterpret_cast<const unsigned short *>(p) : *p;
                } else {
                    raw[c] = a.sample_bytes[c] == 2 ? *reinterpret_cast<const unsigned short *>(p) : *p;
                }
            }
    }
}

} // namespace j2k_hip
