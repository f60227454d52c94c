// out_sample.h -- what the decode's output kernels share (idwt.hip: decode_output_kernel, rgba_out.hip:
// decode_rgba_kernel, and the sequence forms of both): CopyChannel's depth conversion and the saturating rounding; the
// component samples, decode_output_kernel's own lines as a function (that kernel keeps its text); and the store of a
// pixel's channel samples, again that kernel's lines, for its sequence form.  Device code only.
#pragma once

#include <climits>

namespace j2k_hip {

// CopyChannel<DESTTYPE, int> of the reference for unsigned samples: bitShift = dest.depth - src.depth
__device__ __forceinline__ unsigned depth_out(unsigned v, int src_depth, int dst_depth, unsigned dst_mask)
{
    const int shift = dst_depth - src_depth;
    if (shift == 0) return v;
    if (shift < 0) return v >> (-shift);
    if (src_depth >= 8) {
        if (shift <= src_depth) return (v << shift) | (v >> (src_depth - shift));
        const int second = shift - src_depth;
        const unsigned t = ((v << src_depth) | v) & dst_mask; // DESTTYPE t: truncated before the second fill
        return (t << second) | (t >> (src_depth * 2 - second));
    }
    unsigned pd = (unsigned)src_depth, t = v;
    while (pd * 2 < (unsigned)dst_depth) { t = ((t << pd) | t) & dst_mask; pd *= 2; }
    const int second = dst_depth - (int)pd;
    return (t << second) | (t >> ((int)pd - second));
}

// lrintf with libopenjp2's explicit limits (opj_lrintf behind comparisons against +-2^31): a float below -2^31 and NaN give
// the lowest value, one at or above 2^31 the highest, everything between rounds to nearest even.  The cast is reached by
// in-range values only, so no bit pattern's result depends on what the compiler makes of an out-of-range conversion; the
// clamp behind the DC offset turns the two ends into 0 and 2^prec - 1.
__device__ __forceinline__ int sat_lrintf(float f)
{
    if (!(f >= -2147483648.0f)) return INT_MIN;
    if (f >= 2147483648.0f) return INT_MAX;
    return (int)__builtin_rintf(f);
}

// The samples of components 0 .. a.ncomp - 1 for position (x, y) of the destination, each clamped to its own precision
// (v[c] in 0 .. 2^cprec[c] - 1).  A component's own grid is coarser by its sub-sampling factors, and the reference's
// CopyChannel repeats samples onto the channel (src/common/j2k_codec.cpp:274, :374).  A signed component is clamped to
// its signed range and offset by 2^(depth-1) there (:250-252), an unsigned one gets the DC level shift back: one formula.
// ARGS: DecOutArgs or DecRgbaArgs (comp, stride, ncomp, cprec, sub_x, sub_y, org_x, org_y, mct).
template <bool REV, typename ARGS>
__device__ __forceinline__ void component_samples(const ARGS &a, int x, int y, int v[4])
{
    long long o[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = c < a.ncomp ? (long long)((a.org_y + y) / a.sub_y[c]) * a.stride + ((a.org_x + x) / a.sub_x[c]) : 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = 0;
    if constexpr (REV) {
        int s[4] = {0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < 4; ++c) if (c < a.ncomp) s[c] = reinterpret_cast<const int *>(a.comp[c])[o[c]];
        if (a.mct) { // inverse RCT (G.2.2)
            const int yy = s[0], u = s[1], w = s[2];
            const int g = yy - ((u + w) >> 2);
            s[0] = w + g; s[1] = g; s[2] = u + g;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = min(max(s[c] + (1 << (a.cprec[c] - 1)), 0), (1 << a.cprec[c]) - 1);
    } else {
        float f[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 4; ++c) if (c < a.ncomp) f[c] = reinterpret_cast<const float *>(a.comp[c])[o[c]];
        if (a.mct) { // inverse ICT (G.3.2), libopenjp2's constants and operation order
            const float yy = f[0], u = f[1], w = f[2];
            f[0] = yy + w * 1.402f;
            f[1] = (yy - u * 0.34413f) - w * 0.71414f;
            f[2] = yy + u * 1.772f;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const long long t = (long long)sat_lrintf(f[c]) + (1 << (a.cprec[c] - 1));
            v[c] = (int)min(max(t, 0LL), (long long)((1 << a.cprec[c]) - 1));
        }
    }
}

// A destination sample of 32-bit float type (include/j2k_hip.h): the integer ov of depth d, computed as for an integer
// destination, as the float of nominal range 0..1 that it stands for -- ov / (2^d - 1), an IEEE division (correctly rounded:
// what `/` is on this target without fast-math; a multiplication by the reciprocal would miss it for most depths).
// demoted: ov is an After Effects 15+1-bit value (0 .. 32768) and the divisor 32768 (exact).  The highest value gives 1.0f.
__device__ __forceinline__ float out_float(unsigned ov, int d, bool demoted)
{
    return (float)ov / (demoted ? 32768.0f : (float)((1 << d) - 1));
}
__device__ __forceinline__ void store_float(uint8_t *p, unsigned ov, int d, bool demoted)
{
    *reinterpret_cast<float *>(p) = out_float(ov, d, demoted); // (4-byte aligned: base, colbytes and rowbytes are multiples of 4)
}

// Destination channels c < nout of pixel (x, y) from its component samples v[]: CopyChannel's depth conversion, one store per
// channel that has the sample (decode_output_kernel's last loop).  ARGS: DecOutArgs.  FLT: some channel is of float type
// (dst_bytes 4); without it the text is the one the kernels held before float destinations existed.
template <bool FLT, typename ARGS>
__device__ __forceinline__ void store_channels(const ARGS &a, int x, int y, const int v[4])
{
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (c < a.nout && c < a.ncomp && x < a.dst_w[c] && y < a.dst_h[c]) {
            const unsigned mask = a.dst_bytes[c] == 1 ? 0xffu : 0xffffu;
            const unsigned ov = depth_out((unsigned)v[c], a.cprec[c], a.dst_depth[c], mask);
            uint8_t *p = a.dst[c] + (long long)y * a.rowbytes[c] + (long long)x * a.colbytes[c];
            if constexpr (FLT) {
                if (a.dst_bytes[c] == 4) { store_float(p, ov, a.dst_depth[c], false); continue; }
            }
            if (a.dst_bytes[c] == 1) *p = (uint8_t)ov;
            else *reinterpret_cast<unsigned short *>(p) = (unsigned short)ov;
        }
}

} // namespace j2k_hip
