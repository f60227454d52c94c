// compare.hip -- decoded samples against the source samples the front end makes, for gfx950: a streaming reduction
// (include/j2k_hip.h: j2k_hip_compare; kernels.h: CompareArgs).
//
// Per component and sample e = D - S, where S is what the encode's front end would have made of the caller's planes -- loaded
// through frontend_ops.h (fe_load, fe_sample: one definition, one rounding) or read from the planes a front-end kernel wrote --
// and D the decoded 16-bit sample.  A lane takes kV adjacent samples of a row (one 8-byte load of the decoded plane, one 4- or
// 8-byte load per dense source plane, one pixel load each for interleaved frames) and walks down the rows gridDim.y apart, so
// a wave reads contiguous bytes of every plane.  It keeps, per component, 64-bit sums of e^2 and |e|, the count and the maximum
// of the samples that differ and the smallest linear index of one; those are folded across the wave by shuffles, across the
// workgroup's four waves through LDS, and a workgroup that met a difference adds its totals to the call's accumulators with
// ordinary 64-bit atomics (add, max) -- to one of kCompareSets sets of them, which the host folds.  A workgroup that met
// none -- every workgroup of a lossless file -- touches no atomic.  Everything is integer arithmetic: the result does not depend on the order of the reduction.
// Algorithmic bytes per sample: the source sample's bytes + 2.
#include "frontend_ops.h"

namespace j2k_hip {
namespace {

constexpr int kV = 4;         // samples of a row per lane
constexpr int kThreads = 256; // four waves

struct Acc {
    unsigned long long sq, ab, first; // first: the smallest linear index of a sample that differs (~0: none)
    unsigned cnt, mx;
};

// the stored samples of kV adjacent pixels as unsigned samples of a.src.prec bits; s[c][i] for i < n only
template <bool FLT, bool PLANES>
__device__ __forceinline__ void load_source(const CompareArgs &a, int x, int y, int n, int s[4][kV])
{
    if constexpr (PLANES) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < a.ncomp) {
                const int *p = a.planes[c] + (long long)y * a.plane_stride + x;
#pragma unroll
                for (int i = 0; i < kV; ++i)
                    if (i < n) s[c][i] = p[i] + a.plane_dc;
            }
    } else {
        const FrontendArgs &f = a.src;
        if (a.wide && n == kV) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < a.ncomp) {
                    const uint8_t *p = f.src[c] + (long long)y * f.rowbytes[c] + (long long)x * f.sample_bytes[c];
                    unsigned raw[kV];
                    if (f.sample_bytes[c] == 2) {
                        const uint2 q = *reinterpret_cast<const uint2 *>(p);
                        raw[0] = q.x & 0xffffu; raw[1] = q.x >> 16; raw[2] = q.y & 0xffffu; raw[3] = q.y >> 16;
                    } else {
                        const unsigned q = *reinterpret_cast<const unsigned *>(p);
                        raw[0] = q & 0xffu; raw[1] = (q >> 8) & 0xffu; raw[2] = (q >> 16) & 0xffu; raw[3] = q >> 24;
                    }
#pragma unroll
                    for (int i = 0; i < kV; ++i) s[c][i] = fe_sample(f, c, raw[i]);
                }
            return;
        }
#pragma unroll
        for (int i = 0; i < kV; ++i)
            if (i < n) {
                unsigned raw[4] = {0, 0, 0, 0};
                fe_load<FLT>(f, x + i, y, raw);
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (c < a.ncomp) s[c][i] = fe_sample(f, c, raw[c]);
            }
    }
}

__device__ __forceinline__ void load_decoded(const CompareArgs &a, int c, int x, int y, int n, int d[kV])
{
    const uint16_t *p = a.dec[c] + (long long)y * a.dec_sy[c] * a.dec_stride[c] + (long long)x * a.dec_sx[c];
    if (n == kV && a.dec_sx[c] == 1 && (reinterpret_cast<uintptr_t>(p) & 7) == 0) {
        const uint2 q = *reinterpret_cast<const uint2 *>(p);
        d[0] = (int)(q.x & 0xffffu); d[1] = (int)(q.x >> 16); d[2] = (int)(q.y & 0xffffu); d[3] = (int)(q.y >> 16);
        return;
    }
#pragma unroll
    for (int i = 0; i < kV; ++i)
        if (i < n) d[i] = p[(long long)i * a.dec_sx[c]];
}

__device__ __forceinline__ void fold(Acc &v, const Acc &o)
{
    v.sq += o.sq; v.ab += o.ab; v.cnt += o.cnt;
    v.mx = v.mx > o.mx ? v.mx : o.mx;
    v.first = v.first < o.first ? v.first : o.first;
}

template <bool FLT, bool PLANES>
__global__ __launch_bounds__(kThreads) void compare_kernel(CompareArgs a)
{
    Acc acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = Acc{0, 0, ~0ull, 0, 0};
    const int x = (int)(blockIdx.x * kThreads + threadIdx.x) * kV;
    if (x < a.width) {
        const int n = a.width - x < kV ? a.width - x : kV;
        for (int y = (int)blockIdx.y; y < a.height; y += (int)gridDim.y) {
            int s[4][kV];
            load_source<FLT, PLANES>(a, x, y, n, s);
            const unsigned long long row = (unsigned long long)y * (unsigned)a.width + (unsigned)x;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < a.ncomp) {
                    int d[kV];
                    load_decoded(a, c, x, y, n, d);
#pragma unroll
                    for (int i = 0; i < kV; ++i)
                        if (i < n) {
                            const int e = d[i] - s[c][i];
                            const unsigned ae = (unsigned)(e < 0 ? -e : e);
                            // (no branch: selects; a lane's rows and samples come in raster order, so its first is its smallest)
                            acc[c].sq += (unsigned long long)(ae * ae); // |e| <= 65535: the square fits 32 bits
                            acc[c].ab += ae;
                            acc[c].first = (ae != 0 && acc[c].cnt == 0) ? row + (unsigned)i : acc[c].first;
                            acc[c].cnt += ae != 0;
                            acc[c].mx = acc[c].mx > ae ? acc[c].mx : ae;
                        }
                }
        }
    }
    // across the wave, then across the workgroup's waves
    __shared__ Acc part[kThreads / 64][4];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (c < a.ncomp) {
            Acc v = acc[c];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                Acc o;
                o.sq = __shfl_down(v.sq, off, 64); o.ab = __shfl_down(v.ab, off, 64); o.first = __shfl_down(v.first, off, 64);
                o.cnt = __shfl_down(v.cnt, off, 64); o.mx = __shfl_down(v.mx, off, 64);
                fold(v, o);
            }
            if (lane == 0) part[wave][c] = v;
        }
    __syncthreads();
    if ((int)threadIdx.x < a.ncomp) {
        const int c = (int)threadIdx.x;
        Acc v = part[0][c];
#pragma unroll
        for (int w = 1; w < kThreads / 64; ++w) fold(v, part[w][c]);
        if (v.cnt) {
            // (one of kCompareSets sets of accumulators, by workgroup: the atomics of a launch spread over that many lines)
            unsigned long long *out = a.acc + (size_t)kCompareWords * (4 * ((blockIdx.x + blockIdx.y) % kCompareSets) + a.slot[c]);
            atomicAdd(out + 0, v.sq);
            atomicAdd(out + 1, v.ab);
            atomicAdd(out + 2, (unsigned long long)v.cnt);
            atomicMax(out + 3, (unsigned long long)v.mx);
            atomicMax(out + 4, ~v.first);
        }
    }
}

bool has_float(const FrontendArgs &a)
{
    for (int c = 0; c < a.ncomp; ++c)
        if (a.sample_bytes[c] == 4) return true;
    return false;
}

} // namespace

void launch_compare(const CompareArgs &a, hipStream_t s)
{
    if (a.width <= 0 || a.height <= 0 || a.ncomp <= 0) return;
    // about 2048 workgroups (eight per CU) whatever the shape: enough waves in flight to cover the loads, few enough that the
    // workgroups' atomics are no measurable part of the launch
    const unsigned gx = (unsigned)((a.width + kThreads * kV - 1) / (kThreads * kV));
    unsigned gy = gx >= 2048u ? 1u : 2048u / gx;
    if (gy > (unsigned)a.height) gy = (unsigned)a.height;
    const dim3 grid(gx, gy, 1);
    if (a.planes[0]) hipLaunchKernelGGL((compare_kernel<false, true>), grid, dim3(kThreads), 0, s, a);
    else if (has_float(a.src)) hipLaunchKernelGGL((compare_kernel<true, false>), grid, dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL((compare_kernel<false, false>), grid, dim3(kThreads), 0, s, a);
}

} // namespace j2k_hip
