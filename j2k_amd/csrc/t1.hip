// t1.hip -- EBCOT Tier-1 for gfx950: quantisation (A7), bit-plane context modelling and the MQ
// arithmetic coder (A8).  Replaces OpenJPEG's t1.c / mqc.c as reached from opj_encode (reference
// call site: src/common/j2k_openjpeg_codec.cpp:730).  T.800 Annex D
// (coding passes, contexts) and Annex C (MQ coder); results are byte-identical to the oracle.
//
// Integer/bit-serial work (no MFMA, no roofline claim); the whole chip's VALU issue rate is what bounds
// it:
//
//  t1_model_kernel      one 64-lane wavefront per code-block, lane = column.  A column's state lives in
//            registers as 64-bit row masks (significance, sign, refined, visited, current
//            bit-plane).  A coding pass is DECIDED for whole columns at once and only WRITTEN stripe
//            by stripe: which samples the significance pass visits and which become significant
//            is one fixed point on the row masks (the neighbourhood of a sample as the stripe scan
//            meets it = shifted copies of the own / left / right masks, "new" or "old" by position;
//            the chain down a column is a carry chain = one 64-bit addition; the chain from column
//            to column is what the iteration resolves, 2-5 rounds per pass); zero-coding contexts
//            (Table D.1), sign contexts and predictions (Tables D.2/D.3) and the run-length flags
//            of the cleanup pass are evaluated bit-sliced on 32-row halves of those masks (boolean
//            expressions of the neighbour masks, no table, no LDS).  A stripe then costs a few
//            bit-field extracts to form its decision bytes.  In the significance and cleanup passes
//            a lane's bytes of a stripe are packed in registers (v_perm, selectors from a table by
//            which rows code something) and ORed as whole words into a zeroed linear LDS stage at
//            the offset a DPP scan of the per-lane counts gives; the refinement pass does the same with
//            the <= 4 bytes of a stripe column (one v_perm, two words, two stripes per scan).  A cleanup
//            stripe in which every column is in run-length mode and holds no 1 is w identical bytes:
//            plain stores, and a half made of such stripes forms no contexts.
//            A 32-row half of a significance / cleanup pass that visits few samples (and has no
//            run-length column) is written sample by sample instead: the lanes' bytes per stripe are counted
//            on the nibbles of the masks, scanned two stripes to a register, and every lane walks its own
//            visited rows -- the cost follows the samples coded, not the stripes that hold one.
//            They leave in coalesced 1 KiB stores.  With rate control (DIST) the per-pass distortion
//            estimates are weighted population counts of (samples of the pass) & (bit-planes below the
//            current one): the nmsedec tables are piecewise linear in their index (dist_sum).
//  t1_mq2_kernel        one LANE per code-block, two waves per 64 blocks: the MQ coder is serial per
//            block, so blocks are the parallel axis; a producer wave runs the interval/probability
//            recurrence, a consumer wave the code register and byte output, joined by an LDS queue.
//            The producer's two table addresses per decision are byte permutes of the symbol word plus one
//            three-input logic instruction (ctx_word2, mq2_slot); the consumer stores its bytes through a plain
//            per-lane LDS pointer and moves the lane's remainder to the front of its stage at every flush.
//  t1_rate_fixup_kernel the reference's fix-ups of the per-pass byte counts (rate control, and behind the styled coder).
// Frames with a code-block style are coded by t1_mq_styled.hip (launch_t1_mq chooses); of this file they use the modeller,
// in its BYPASS instantiation where raw passes exist, and the fix-ups.
#include "kernels.h"
#include "t1_common.h"
#include "cblk_style.h"
#include "t1_mq_window.h"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace j2k_hip {
namespace {


constexpr int kFrac = 6;
constexpr int kFlush = 1024;                 // decisions go to HBM in coalesced 1 KiB pieces (64 lanes x 16 B)
constexpr int kStageBytes = kFlush + 64 * 10; // linear LDS stage per wave: < kFlush left over + one 64 x 10 byte burst


// issue priority of the wave (s_setprio takes an immediate): 0 leaves it alone, 1..3 set that level
__device__ __forceinline__ void set_priority(int p)
{
    if (p >= 3) __builtin_amdgcn_s_setprio(3);
    else if (p == 2) __builtin_amdgcn_s_setprio(2);
    else if (p == 1) __builtin_amdgcn_s_setprio(1);
}

// value of lane-1 / lane+1 through DPP wave shifts; lane 0 / lane 63 receive 0
__device__ __forceinline__ unsigned from_left(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x138 /*wave_shr:1*/, 0xf, 0xf, false); }
__device__ __forceinline__ unsigned from_right(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x130 /*wave_shl:1*/, 0xf, 0xf, false); }

__device__ __forceinline__ u64 from_left64(u64 v) { return (u64)from_left((unsigned)v) | ((u64)from_left((unsigned)(v >> 32)) << 32); }
__device__ __forceinline__ u64 from_right64(u64 v) { return (u64)from_right((unsigned)v) | ((u64)from_right((unsigned)(v >> 32)) << 32); }

// exclusive prefix sum over the wave of a per-lane count, plus the wave total, through a DPP scan:
// row_shr 1/2/4/8 inside the rows of 16 lanes, then row_bcast15 / row_bcast31 carry the row totals
// into the following rows (6 adds, no ballots)
__device__ __forceinline__ unsigned prefix_count_dpp(unsigned cnt, unsigned &total)
{
    int t = (int)cnt;
    t += __builtin_amdgcn_update_dpp(0, t, 0x111, 0xf, 0xf, false);
    t += __builtin_amdgcn_update_dpp(0, t, 0x112, 0xf, 0xf, false);
    t += __builtin_amdgcn_update_dpp(0, t, 0x114, 0xf, 0xf, false);
    t += __builtin_amdgcn_update_dpp(0, t, 0x118, 0xf, 0xf, false);
    t += __builtin_amdgcn_update_dpp(0, t, 0x142, 0xa, 0xf, false);
    t += __builtin_amdgcn_update_dpp(0, t, 0x143, 0xc, 0xf, false);
    total = (unsigned)__builtin_amdgcn_readlane(t, 63);
    return (unsigned)t - cnt;
}

// population counts of the eight nibbles of a word, each in its nibble
__device__ __forceinline__ unsigned nibble_counts(unsigned v)
{
    const unsigned x = v - ((v >> 1) & 0x55555555u);
    return (x & 0x33333333u) + ((x >> 2) & 0x33333333u);
}

// Sample-wise writing of a sparse pass half against its dense stripe loop, in static VALU instructions of the kernel as
// built (tools/isa.sh, <false,false>, all paths): the stripe loop costs kDenseStripe per stripe that holds a visited
// sample; the sample-wise path kSparseHead once (nibble counts, four packed scans, stripe bases) and kSparseRound per
// round, rounds = visited samples of the busiest lane.  The sample-wise path is taken when it is the cheaper one by these.
// (Stripe costs of 70 and 85 -- nearer to what a stripe executes with its skipped parts left out -- were built and
//  measured on the metric frame: the kernel's vector instructions and its time moved by less than 0.5 %.)
constexpr unsigned kDenseStripe = 103, kSparseHead = 64, kSparseRound = 44;
constexpr unsigned kBurst = 64 * 10; // room of the stage beyond what may be pending

// distortion LUTs of the oracle in closed form (index = 7 bits around the current bit-plane)
__device__ __forceinline__ int nmsedec_sig(unsigned m, int bp)
{
    const int i = (int)((m >> bp) & 127u);
    return bp > 0 ? max(0, (3 * i - 144) * 128) : ((i * i + 32) >> 6) * 128;
}
__device__ __forceinline__ int nmsedec_ref(unsigned m, int bp)
{
    const int i = (int)((m >> bp) & 127u);
    if (bp > 0) return i >= 64 ? max(0, (i - 80) * 128) : max(0, (48 - i) * 128);
    return (((i - 64) * (i - 64) + 32) >> 6) * 128;
}

// v_perm selectors that compact a stripe column's decision bytes, by presence (entry Vz | N << 4: the rows that code a
// zero-coding / a sign decision): output byte k = the k-th present one of Z0 S0 Z1 S1 Z2 S2 Z3 S3 (byte r of zsym =
// selector r, of ssym = selector 4 + r), 0x0c (a zero byte) past the last
struct PackSel {
    u64 v[256];
    constexpr PackSel() : v()
    {
        for (int e = 0; e < 256; ++e) {
            u64 sel = 0x0c0c0c0c0c0c0c0cull;
            int k = 0;
            for (int r = 0; r < 4; ++r) {
                if ((e >> r) & 1) { sel = (sel & ~(0xffull << (8 * k))) | ((u64)r << (8 * k)); ++k; }
                if ((e >> (4 + r)) & 1) { sel = (sel & ~(0xffull << (8 * k))) | ((u64)(4 + r) << (8 * k)); ++k; }
            }
            v[e] = sel;
        }
    }
};
__constant__ PackSel kPackSel = PackSel();

// Two bit-planes' row nibbles of a stripe as decision-byte bits at once: entry a | b << 4 holds bit r of a at bit 0 and bit r of
// b at bit 1 of byte r -- spread4(a) | spread4(b) << 1 without the two multiplies.  The dense stripes take their zero-coding and
// sign bytes from it two planes at a time, the refinement rounds theirs.  The plain variants of the modeller hold a copy in LDS.
struct PairTab {
    unsigned v[256];
    constexpr PairTab() : v()
    {
        for (unsigned e = 0; e < 256; ++e) {
            unsigned t = 0;
            for (unsigned r = 0; r < 4; ++r) t |= (((e >> r) & 1u) | (((e >> (4 + r)) & 1u) << 1)) << (8 * r);
            v[e] = t;
        }
    }
};
constexpr bool pair_tab_ok()
{
    const PairTab t;
    for (unsigned a = 0; a < 16; ++a)
        for (unsigned b = 0; b < 16; ++b)
            if (t.v[a | (b << 4)] != (spread4(a) | (spread4(b) << 1))) return false;
    return true;
}
static_assert(pair_tab_ok(), "PairTab: entry a | b << 4 must be spread4(a) | spread4(b) << 1 for all 256 nibble pairs");
__constant__ PairTab kPairTab = PairTab();
// The table's index bytes of one 32-row half for a plane pair (x, y): byte k of `even` is the entry number of stripe 2 k, of
// `odd` that of stripe 2 k + 1 (x's nibble below y's)
__device__ __forceinline__ void pair_index(unsigned x, unsigned y, unsigned &even, unsigned &odd)
{
    constexpr unsigned M = 0x0f0f0f0fu;
    even = (x & M) | ((y << 4) & ~M);
    odd = ((x >> 4) & M) | (y & ~M);
}

// one butterfly stage of the 32 x 32 bit-matrix transpose held in 32 registers (m[p] bit r <- m[r] bit p after the five
// stages J = 16, 8, 4, 2, 1)
template <int J, unsigned MASK>
__device__ __forceinline__ void transpose_stage(unsigned (&m)[32])
{
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        if (k & J) continue;
        const unsigned t = ((m[k] >> J) ^ m[k + J]) & MASK;
        m[k] ^= t << J;
        m[k + J] ^= t;
    }
}

// A coefficient word as the coder sees it: the magnitude of the sample scaled to kFrac fractional bits (9/7: the quotient
// by the step size, rounded once more to an integer of 1/64 steps, as the oracle's quantiser does; 5/3: the integer
// shifted up) and its sign as 0 / 1
template <bool REV>
__device__ __forceinline__ unsigned scaled_magnitude(unsigned word, float stepsize, unsigned &neg)
{
    if constexpr (REV) {
        const int c = (int)word;
        neg = (unsigned)c >> 31;
        return (unsigned)(c < 0 ? -c : c) << kFrac;
    } else {
        const int t = __float2int_rn(__fmul_rn(__fdiv_rn(__uint_as_float(word), stepsize), 64.0f));
        neg = (unsigned)t >> 31;
        return (unsigned)(t < 0 ? -t : t);
    }
}

// (7 waves per SIMD = 72 VGPRs: what the pass loops need; the one-off transposition of the magnitudes would take 98 and
//  spills a few registers instead -- outside every loop)
#ifndef J2K_MODEL_WAVES
#define J2K_MODEL_WAVES 7
#endif
// BYPASS: an instantiation of its own for frames coded with selective arithmetic-coding bypass (never with DIST: a style
// excludes rate control).  Its one difference: in a raw significance pass a sign decision carries the sample's sign, not
// sign XOR prediction -- a raw bit is the sign itself (D.6), and the prediction cannot be taken out again from the context
// number (Table D.3).  Without it the kernel compiles to the code it was before the parameter existed.
template <bool REV, bool DIST, bool BYPASS = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(J2K_MODEL_WAVES, J2K_MODEL_WAVES))) void t1_model_kernel(T1Args a)
{
    // The block's scaled magnitudes go back into its own area of the coefficient buffer (dead after Tier-1) -- as
    // transposed bit-planes, or as they are for heights other than 64 and 32 -- and each bit-plane is re-read from L2:
    // no 16 KiB of magnitudes in LDS per wave, 2.5x the occupancy.
    // DIST (rate control): the six bit-planes below the current one, which the distortion estimates of its passes
    // look at, wait in LDS (plane q of the magnitudes in slot q % 6; one new plane per bit-plane of the scan).
    __shared__ u64 win[DIST ? 6 * 64 : 1];
    __shared__ __attribute__((aligned(16))) unsigned char stage[kStageBytes];
    // the selector table kPackSel in LDS (with DIST the distortion window leaves no room for its 2 KiB at 7 waves per
    // SIMD: that variant reads it from constant memory)
    __shared__ u64 sel_tab[DIST ? 1 : 256];
    // PairTab in LDS beside it, for the same reason not with DIST: that variant keeps the multiplies.  (Read per lane from
    // constant memory the table cost more than it saved: every look-up is a gather over up to sixteen cache lines.)
    constexpr bool kPairTabs = !DIST;
    __shared__ unsigned pair_tab[kPairTabs ? 256 : 1];
    const auto pair_entry = [&](unsigned e) -> unsigned { return pair_tab[e]; };

    const int b = a.first + (int)blockIdx.x;
    const int lane = threadIdx.x;
    set_priority(a.model_prio);
    // the launch has started, so everything before it in the stream (the frame's DWT) is through
    if (a.done_word && blockIdx.x == 0 && lane == 0) __hip_atomic_store(a.done_word, a.done_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const CblkDev cb = a.blks[b];
    const int w = cb.w, h = cb.h, orient = cb.orient;
    // the stage starts zeroed and stays so beyond what is pending (decisions are ORed into it)
    for (int i = lane; i < kStageBytes / 16; i += 64) reinterpret_cast<uint4 *>(stage)[i] = make_uint4(0, 0, 0, 0);
    if constexpr (!DIST)
        for (int e = lane; e < 256; e += 64) { sel_tab[e] = kPackSel.v[e]; pair_tab[e] = kPairTab.v[e]; }

    // ---- A7: load the block (coalesced rows), scale to sign-magnitude with 6 fractional bits
    u64 chi = 0;
    unsigned mx = 0;
    // Rows are addressed as a wave-uniform row pointer (advanced by the stride on the scalar unit) plus the lane: no
    // per-row address arithmetic on the vector unit.
    unsigned *const blk0 = const_cast<unsigned *>(reinterpret_cast<const unsigned *>(a.coef)) + cb.coef_off;
    const long long stride = a.stride;
    // Blocks of 64 or 32 rows, one 32-row half at a time: the 32 rows of a column are loaded into 32 registers, scaled
    // there, a 32 x 32 bit-matrix transpose (5 butterfly stages) turns them into one word per bit-plane (bit r = that
    // plane's bit of row r), and the words of planes kFrac .. kFrac+25 go to rows 0..25 (upper half of the column) and
    // 32..57 (lower half) of the block's own area (the coefficient buffer is dead after Tier-1).  The magnitudes
    // themselves are never stored.  A bit-plane of the column is then two coalesced loads: no 16 KiB of magnitudes in
    // LDS per wave, 2.5x the occupancy.  (Every plane word depends on all 32 rows of its half, so the rows are read
    // before the first word lands on one of them; lanes beyond w hold other blocks' samples and neither load nor store.)
    // With distortion sums all 32 planes are kept (plane q in rows q and 32 + q): the estimates read the fractional bits.
    constexpr int kPlane0 = DIST ? 0 : kFrac, kPlaneRows = DIST ? 32 : 26;
    // Blocks of 32 rows (the 32 x 32 blocks of the cinema profiles) have one such half: 32 rows, 32 plane words.
    const bool planes_stored = h == 64 || h == 32;
    const int halves = h >> 5;
    if (planes_stored) {
        unsigned mxl = 0;
#pragma unroll 1
        for (int half = 0; half < halves; ++half) {
            unsigned *const half0 = blk0 + (long long)(32 * half) * stride;
            unsigned neg = 0;
            if (lane < w) {
                unsigned m[32];
                const unsigned *rp = half0;
#pragma unroll
                for (int i = 0; i < 32; ++i, rp += stride) {
                    if ((i & 7) == 0) __builtin_amdgcn_sched_barrier(0); // (the loads leave in row order, all 32 in flight)
                    m[i] = rp[lane];
                }
#pragma unroll
                for (int i = 0; i < 32; ++i) {
                    if ((i & 3) == 0) __builtin_amdgcn_sched_barrier(0); // (a row's sign is folded in before the next rows are scaled: it is not kept beside its magnitude)
                    unsigned n;
                    m[i] = scaled_magnitude<REV>(m[i], cb.stepsize, n); // (bit 31 is never used: |q| < 2^31)
                    neg |= n << i;
                    mxl = max(mxl, m[i]);
                }
                __builtin_amdgcn_sched_barrier(0);
                transpose_stage<16, 0x0000ffffu>(m);
                transpose_stage<8, 0x00ff00ffu>(m);
                transpose_stage<4, 0x0f0f0f0fu>(m);
                transpose_stage<2, 0x33333333u>(m);
                transpose_stage<1, 0x55555555u>(m);
                unsigned *wp = half0;
#pragma unroll
                for (int q = 0; q < kPlaneRows; ++q, wp += stride) {
                    if ((q & 3) == 0) __builtin_amdgcn_sched_barrier(0);
                    wp[lane] = m[q + kPlane0];
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            chi |= (u64)neg << (32 * half);
        }
        mx = mxl;
    } else { // any other height: the magnitudes are written back in place, and every bit-plane re-reads them from L2
        unsigned *rp = blk0;
        for (int y = 0; y < h; ++y, rp += stride) {
            unsigned m = 0, n = 0;
            if (lane < w) {
                m = scaled_magnitude<REV>(rp[lane], cb.stepsize, n);
                rp[lane] = m;
            }
            chi |= (u64)n << y;
            mx = max(mx, m);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, o));
    mx = (unsigned)__builtin_amdgcn_readfirstlane((int)mx); // wave-uniform: lets the pass / bit-plane control flow run on the scalar unit
    int numbps = mx ? (32 - __clz((int)mx)) - kFrac : 0;
    if (numbps < 0) numbps = 0;
    __syncthreads();

    unsigned *pass_nsym = a.pass_nsym + (size_t)b * kDevMaxPasses;
    int *pass_nmsedec = a.pass_nmsedec + (size_t)b * kDevMaxPasses;
    // gated coding: the block's coder workgroup may start once every block of its group has reported here (the release makes
    // this wave's stores -- decisions, per-pass tables, counts -- visible to a wave on any XCD that acquires after it)
    auto report = [&]() {
        if (!a.gate_group_of) return;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        if (lane == 0) __hip_atomic_fetch_add(a.gate_ready + a.gate_group_of[b], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    };
    if (numbps == 0 || 3 * numbps - 2 > kDevMaxPasses) {
        if (lane == 0) {
            a.numbps[b] = 0; a.npasses[b] = 0; a.nsym[b] = 0;
            if (numbps) a.err[0] = 1u; // more bit-planes than the pass tables hold
        }
        report();
        return;
    }

    // the block's samples of this column as a row mask.  Formed where it is used (the rows are wave-uniform, the column test is
    // one compare; the width goes through an empty asm so that the mask is not hoisted): held in a register pair through the
    // pass loops it is one 64-bit value too many there and something spills
    const u64 rows_of_block = h == 64 ? ~(u64)0 : (((u64)1 << h) - 1);
    auto rowmask_now = [&]() -> u64 {
        int wv = w;
        asm volatile("" : "+s"(wv));
        return lane < wv ? rows_of_block : 0;
    };
    const int nstripes = (h + 3) >> 2;
    u64 sigma = 0, mu = 0, pi = 0;
    unsigned fill = 0, flushed = 0; // decisions produced / already stored to HBM (wave-uniform)
    unsigned char *symout = a.sym + cb.sym_off;
    const unsigned symcap = cb.sym_cap;
    bool overflow = false;

    // Decisions are staged in a linear LDS buffer: [0, fill - flushed) is pending, always < kFlush between
    // appends.  reserve() hands every lane the stage offset of its first byte (lane order = scan order of
    // the columns), the caller scatters its bytes there, commit() accounts for them and, once kFlush bytes
    // are pending, stores them to HBM and moves the remainder to the front.
    auto reserve = [&](unsigned cnt, auto maxc, unsigned &total) -> unsigned {
        // counts of at most 4 need 3 ballot rounds, at most 8/10 need 4
        (void)maxc;
        const unsigned off = prefix_count_dpp(cnt, total);
        return (fill - flushed) + off;
    };
    auto commit = [&](unsigned total) {
        fill += total;
        if (fill - flushed >= kFlush) {
            __builtin_amdgcn_wave_barrier();
            // (the lane number through an empty asm: its multiples and the lane's address in the stream are formed here, once per
            //  flush, and not kept in four registers through every loop of the kernel)
            int ln = lane;
            asm volatile("" : "+v"(ln));
            const uint4 v = *reinterpret_cast<const uint4 *>(&stage[ln * 16]);
            const uint4 r = *reinterpret_cast<const uint4 *>(&stage[kFlush + min(ln, 39) * 16]); // 40 x 16 B cover the burst
            if (flushed + kFlush <= symcap) *reinterpret_cast<uint4 *>(symout + flushed + ln * 16) = v;
            else overflow = true;
            flushed += kFlush;
            __builtin_amdgcn_wave_barrier();
            // the remainder moves to the front, and what it leaves behind is zeroed again (the zero is made here: a
            // constant would be held in four registers through the whole pass loop)
            unsigned z;
            asm volatile("v_mov_b32 %0, 0" : "=v"(z));
            const uint4 zero = make_uint4(z, z, z, z);
            if (ln < 40) {
                *reinterpret_cast<uint4 *>(&stage[ln * 16]) = r;
                *reinterpret_cast<uint4 *>(&stage[kFlush + ln * 16]) = zero;
            } else *reinterpret_cast<uint4 *>(&stage[ln * 16]) = zero;
            __builtin_amdgcn_wave_barrier();
        }
    };
    // A lane's bytes of one stripe, cnt <= 10 of them packed in p0 | p1 << 32 | p2 << 64 and destined for stage[base ..):
    // they are ORed into the zeroed stage as aligned words (v_alignbyte by the byte offset inside the word), only the
    // words that hold some of them.  Lanes sharing a word combine by OR, in any order.
    auto emit = [&](unsigned base, unsigned cnt, unsigned p0, unsigned p1, unsigned p2) {
        const unsigned t = 0u - base; // (v_alignbyte reads t & 3 = 4 - (base & 3), or 0)
        const unsigned al = (base + 3u) & ~3u; // the first word boundary at or after base
        unsigned *const wp = reinterpret_cast<unsigned *>(stage + al);
        const int e = (int)(base + cnt) - (int)al; // bytes of the lane from there on
        if (cnt != 0 && al != base) __hip_atomic_fetch_or(wp - 1, __builtin_amdgcn_alignbyte(p0, 0u, t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        if (e > 0) __hip_atomic_fetch_or(wp, __builtin_amdgcn_alignbyte(p1, p0, t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        if (e > 4) __hip_atomic_fetch_or(wp + 1, __builtin_amdgcn_alignbyte(p2, p1, t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        if (e > 8) __hip_atomic_fetch_or(wp + 2, __builtin_amdgcn_alignbyte(0u, p2, t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    };

    // the two-word form: cnt <= 4 bytes packed in p0 (zero bytes past the last)
    auto emit4 = [&](unsigned base, unsigned cnt, unsigned p0) {
        const unsigned t = 0u - base;
        const unsigned al = (base + 3u) & ~3u;
        unsigned *const wp = reinterpret_cast<unsigned *>(stage + al);
        const int e = (int)(base + cnt) - (int)al;
        if (cnt != 0 && al != base) __hip_atomic_fetch_or(wp - 1, __builtin_amdgcn_alignbyte(p0, 0u, t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        if (e > 0) __hip_atomic_fetch_or(wp, __builtin_amdgcn_alignbyte(0u, p0, t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    };

#ifdef J2K_T1_COUNTERS
    unsigned long long dc[kT1Counters] = {};
#define DCNT(i) (++dc[i])
#define DADD(i, n) (dc[i] += (n))
#else
#define DCNT(i) ((void)0)
#define DADD(i, n) ((void)0)
#endif
    // plane q of the magnitudes of this column (stored planes only): two coalesced loads
    auto plane_word = [&](int q) -> u64 {
        if (lane >= w) return 0;
        const unsigned *const rp = blk0 + (long long)(q - kPlane0) * stride; // (wave-uniform: the lane is the load's offset)
        const unsigned lo = rp[lane];
        const unsigned hi = halves == 2 ? (rp + 32 * stride)[lane] : 0u;
        return (u64)lo | ((u64)hi << 32);
    };
    if constexpr (DIST) {
        if (planes_stored)
            for (int q = numbps; q < numbps + 5; ++q) win[(q % 6) * 64 + lane] = plane_word(q); // (the top plane's own slot is filled in its round)
    }
    // Distortion estimates of a pass (OpenJPEG's nmsedec tables in closed form, see nmsedec_sig / nmsedec_ref) summed
    // over the samples in `set`.  For all planes but the last the tables are piecewise linear in the 7-bit index
    // (current bit b6, the six bits f below it), so a sum over samples is a weighted sum of population counts of
    // set & plane -- no per-sample work; the last plane's tables have a quadratic term (f * f + 32) >> 6 per sample.
    auto dist_sum = [&](u64 set, u64 cur, int bp, bool refinement) -> int {
        if (!set) return 0;
        if (!planes_stored) { // partial blocks: per sample from the magnitudes in place
            int sum = 0;
            for (u64 rest = set; rest; rest &= rest - 1) {
                const unsigned m = blk0[(long long)__builtin_ctzll(rest) * stride + lane];
                sum += refinement ? nmsedec_ref(m, bp) : nmsedec_sig(m, bp);
            }
            return sum;
        }
        u64 W[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) W[k] = win[((bp + k) % 6) * 64 + lane];
        auto weighted = [&](u64 sel) { // sum of f over the samples in sel
            int t = 0;
#pragma unroll
            for (int k = 0; k < 6; ++k) t += __popcll(sel & W[k]) << k;
            return t;
        };
        int sum;
        if (bp > 0) {
            if (!refinement) sum = 48 * __popcll(set) + 3 * weighted(set);           // 3 i - 144, i = 64 + f
            else {
                const u64 up = set & cur & (W[5] | W[4]), down = set & ~cur & ~(W[5] & W[4]);
                sum = weighted(up) - 16 * __popcll(up) + 48 * __popcll(down) - weighted(down); // max(0, i - 80) | max(0, 48 - i)
            }
        } else {
            // (i * i + 32) >> 6 with i = 64 + f, resp. ((i - 64)^2 + 32) >> 6: 64 +- 2 f + ((f * f + 32) >> 6), the +- part only for b6 = 0
            if (!refinement) sum = 64 * __popcll(set) + 2 * weighted(set);
            else { const u64 down = set & ~cur; sum = 64 * __popcll(down) - 2 * weighted(down); }
            for (u64 rest = set; rest; rest &= rest - 1) {
                const int r = __builtin_ctzll(rest);
                int f = 0;
#pragma unroll
                for (int k = 0; k < 6; ++k) f |= (int)((W[k] >> r) & 1u) << k;
                sum += (f * f + 32) >> 6;
            }
        }
        return sum * 128;
    };
    int pass = 0;
    for (int bp = numbps - 1; bp >= 0; --bp) {
        DCNT(6);
        // current bit-plane of this column as a row mask
        u64 bits = 0;
        const int sb = bp + kFrac;
        if (planes_stored) {
            bits = plane_word(sb);
            if constexpr (DIST) win[(bp % 6) * 64 + lane] = plane_word(bp); // joins the window: planes bp .. bp+5 of the magnitudes
        } else if (lane < w) {
            // (row pointers formed from the wave-uniform row number: a scalar multiply, and nothing for the optimiser to
            //  turn into per-lane pointers that it would keep across the bit-plane loop)
            int y = 0;
            for (; y + 8 <= h; y += 8) { // 8 row loads in flight
                const unsigned *rp = blk0 + (long long)y * stride;
                unsigned t[8];
#pragma unroll
                for (int i = 0; i < 8; ++i, rp += stride) t[i] = rp[lane];
#pragma unroll
                for (int i = 0; i < 8; ++i) bits |= (u64)((t[i] >> sb) & 1u) << (y + i);
            }
            for (; y < h; ++y) bits |= (u64)(((blk0 + (long long)y * stride)[lane] >> sb) & 1u) << y;
        }

        for (int pt = (bp == numbps - 1 ? 2 : 0); pt < 3; ++pt) {
            int nm = 0;
            // whole-pass early-out: SPP/CUP code only insignificant samples, MRP only significant ones
            // (the cleanup pass only codes what the significance-propagation pass of this bit-plane left unvisited)
            const u64 rowmask = rowmask_now();
            const u64 todo = pt == 1 ? sigma : (pt == 0 ? rowmask & ~sigma : rowmask & ~sigma & ~pi);
            const bool pass_work = todo != 0;
            const int ns_eff = __any(pass_work) ? nstripes : 0;
            if (pt == 1) {
                // ---- magnitude refinement pass: no dependency between samples, so the four rows of a
                // stripe are handled with bit-parallel arithmetic on the 4-bit row nibbles
                // (model_wc: which rows are refined and which of them have a significant neighbour -- left / right columns
                //  rows r-1..r+1, own column r-1, r+1 -- for the whole column at once)
                // (a later refinement has context 16 whatever its neighbours: the neighbour flag is cleared there once per pass, and
                //  the decision byte of a row is 0x1c + 2 * flag + 4 * later + bit -- 14 + flag or 16, << 1, | bit -- by additions alone)
                u64 ref64 = 0, nb64 = 0;
                if (ns_eff) {
                    const u64 LR = from_left64(sigma) | from_right64(sigma);
                    nb64 = ((sigma << 1) | (sigma >> 1) | LR | (LR << 1) | (LR >> 1)) & ~mu;
                    ref64 = sigma & ~pi;
                }
                if constexpr (DIST) nm = dist_sum(ref64, bits, bp, true);
                // two stripes per round: their per-lane byte counts share one prefix scan (16-bit halves of one register).  The
                // rounds run on one 32-row half of the masks at a time: a stripe's rows are 4-bit fields of single registers
#pragma unroll 1
                for (int half = 0; 8 * half < ns_eff; ++half) {
                    auto hf = [&](u64 m) { return half ? (unsigned)(m >> 32) : (unsigned)m; };
                    const unsigned refh = hf(ref64), nbh = hf(nb64), muh = hf(mu), bitsh = hf(bits);
                    const int rows = min(4 * ns_eff - 32 * half, 32);
                    // a round's two stripes are an even and an odd one: byte sl / 8 of the two index words
                    unsigned bn[2] = {0, 0};
                    if constexpr (kPairTabs) pair_index(bitsh, nbh, bn[0], bn[1]);
                    for (int sl = 0; sl < rows; sl += 8) {
                        const unsigned ref8 = __builtin_amdgcn_ubfe(refh, (unsigned)sl, 8u); // rows of both stripes refined in this pass
                        if (!__any(ref8 != 0)) { DCNT(5); continue; }
                        unsigned pk[2], cnt[2];
#pragma unroll
                        for (int k = 0; k < 2; ++k) {
                            // a stripe's four decision bytes are compacted in registers: one v_perm with the low word of the selector
                            // table's entry (Vz = ref4, N = 0): "the present rows' bytes in order", zero bytes past the last
                            const unsigned ref4 = k ? ref8 >> 4 : ref8 & 0xfu;
                            const unsigned at = (unsigned)(sl + 4 * k);
                            const unsigned sel = (unsigned)(DIST ? kPackSel.v[ref4] : sel_tab[ref4]);
                            unsigned W;
                            if constexpr (kPairTabs)
                                W = 0x1c1c1c1cu + pair_entry(__builtin_amdgcn_ubfe(bn[k], (unsigned)sl, 8u)) + (pair_entry(__builtin_amdgcn_ubfe(muh, at, 4u)) << 2);
                            else
                                W = 0x1c1c1c1cu + (spread4(__builtin_amdgcn_ubfe(nbh, at, 4u)) << 1) + (spread4(__builtin_amdgcn_ubfe(muh, at, 4u)) << 2) +
                                    spread4(__builtin_amdgcn_ubfe(bitsh, at, 4u));
                            pk[k] = __builtin_amdgcn_perm(0u, W, sel);
                            cnt[k] = (unsigned)__builtin_popcount(ref4);
                        }
                        DCNT(4);
                        unsigned totals;
                        const unsigned offs = prefix_count_dpp(cnt[0] | (cnt[1] << 16), totals); // (sums < 65536: no carry between the halves)
                        const unsigned total0 = totals & 0xffffu, total1 = totals >> 16;
                        const unsigned pend = fill - flushed;
                        emit4(pend + (offs & 0xffffu), cnt[0], pk[0]);
                        emit4(pend + total0 + (offs >> 16), cnt[1], pk[1]);
                        DCNT(total0 + total1 < 64 ? 50 : (total0 + total1 < 448 ? 51 : (total0 + total1 < 512 ? 52 : 53)));
                        DADD(16, total0 + total1);
                        commit(total0 + total1);
                    }
                }
                mu |= ref64; // every row refined in this pass
            } else if (ns_eff) {
            {
            // ---- significance propagation (pt 0) / cleanup (pt 2), decided for whole columns at once on 64-bit row masks.
            // Which samples a pass visits (V) and which become significant (N) is known before any stripe is emitted;
            // the stripes then only form contexts and write decisions.  Timing of a sample's neighbourhood in the
            // stripe scan: the row above and the left column count with what this pass has made significant so far,
            // the row below and the right column as they were -- except across stripe boundaries: the left column's
            // row below the stripe (r = 3 mod 4) is still old, the right column's row above the stripe (r = 0 mod 4)
            // is already new.
            constexpr u64 M0 = 0x1111111111111111ull, M3 = 0x8888888888888888ull;
            const u64 O = sigma;
            const u64 LO = from_left64(O), RO = from_right64(O);
            u64 N64, V64;
            if (pt == 0) {
                // A sample is visited when that neighbourhood holds a significant sample; it becomes significant when its
                // bit is 1.  Fixed point over the columns; the chain down a column (N_r |= pb_r & N_(r-1)) is a carry
                // chain: one 64-bit addition.
                const u64 cand = rowmask & ~O, pb = cand & bits;
                const u64 Hc = (O >> 1) | (LO >> 1) | (RO << 1) | RO | (RO >> 1); // the part that does not move
                u64 H = 0;
                N64 = 0;
                for (;;) {
                    DCNT(1);
                    const u64 A_ = O | N64;
                    const u64 LA_ = from_left64(A_), RA_ = from_right64(A_);
                    H = Hc | (A_ << 1) | (LA_ << 1) | LA_ | ((LA_ >> 1) & ~M3) | ((RA_ << 1) & M0);
                    const u64 G = pb & H;
                    const u64 Nn = (pb & ~(pb + G)) | G;
                    const bool changed = Nn != N64;
                    N64 = Nn;
                    if (!__any(changed)) break;
                }
                V64 = cand & H;
            } else { // cleanup: everything not yet coded in this plane; a 1 bit makes it significant
                V64 = rowmask & ~O & ~pi;
                N64 = V64 & bits;
            }
            if constexpr (DIST) nm = dist_sum(N64, bits, bp, false);
            const u64 A = O | N64;
            const u64 LA = from_left64(A), RA = from_right64(A);
            // (here, not behind the halves, and pinned here: V64 need not outlive them -- sunk to the end of the pass it is
            //  spilled across the stripe loops)
            if (pt == 0) pi |= V64;
            asm volatile("" : "+v"(pi));
            // stripes with anything to code (wave-wide OR of the per-lane nibble occupancy)
            u64 occ = V64 | (V64 >> 1);
            occ = (occ | (occ >> 2)) & M0;
            unsigned olo = (unsigned)occ, ohi = (unsigned)(occ >> 32);
#define J2K_OR_STEP(ctrl, rmask)                                                                   \
            olo |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)olo, ctrl, rmask, 0xf, false);    \
            ohi |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)ohi, ctrl, rmask, 0xf, false);
            J2K_OR_STEP(0x111, 0xf) J2K_OR_STEP(0x112, 0xf) J2K_OR_STEP(0x114, 0xf) J2K_OR_STEP(0x118, 0xf)
            J2K_OR_STEP(0x142, 0xa) J2K_OR_STEP(0x143, 0xc)
#undef J2K_OR_STEP
            const unsigned act[2] = {(unsigned)__builtin_amdgcn_readlane((int)olo, 63), (unsigned)__builtin_amdgcn_readlane((int)ohi, 63)};
            const bool any_n = __any(N64 != 0);
#ifdef J2K_T1_COUNTERS
            { // passes by the busiest lane's visited samples, with the stripes that hold one
                unsigned busiest = (unsigned)__popcll(V64);
                for (int o = 32; o > 0; o >>= 1) busiest = max(busiest, (unsigned)__shfl_xor((int)busiest, o));
                const int bucket = busiest == 0 ? 0 : (busiest <= 2 ? 1 : 32 - __clz((int)busiest - 1));
                const int t0 = pt == 0 ? 20 : 34;
                DCNT(pt == 0 ? 10 : 11);
                DCNT(t0 + bucket);
                DADD(t0 + 7 + bucket, __builtin_popcount(act[0]) + __builtin_popcount(act[1]));
            }
#endif
            // The contexts of the pass are formed for 32 rows at a time (rows 0..31, then 32..63): every mask below is the
            // half of a 64-bit row mask, so the bit-sliced tables run on single registers and only one half's planes are alive
            // while its eight stripes are written.
#pragma unroll 1
            for (int half = 0; half < 2; ++half) {
                unsigned active = act[half];
                if (!active) continue;
                auto hf = [&](u64 m) { return half ? (unsigned)(m >> 32) : (unsigned)m; };
                // ---- cleanup pass, run-length mode: a full stripe column with nothing significant in its 3 x 6 neighbourhood
                // when the scan arrives (flag at the bit of the stripe's first row)
                unsigned rl = 0;
                if (pt != 0) {
                    const u64 in = O | LA | RO; // rows of the stripe: own old, left new, right old
                    u64 busy = in | (in >> 1);
                    busy |= busy >> 2;
                    busy |= ((A | LA | RA) << 1) | ((O | LO | RO) >> 4); // row above the stripe (new), row below it (old)
                    u64 full = V64 & (V64 >> 1);
                    full &= full >> 2;
                    rl = hf(full & ~busy & M0);
                }
                const unsigned bitsh = hf(bits), Nh = hf(A) & ~hf(O), Vh = hf(V64); // (N64 = A & ~O: one 64-bit mask less alive through the halves)
                // ---- run-length fills: a cleanup stripe in which every column of the block is in run-length mode and holds no 1
                // is w bytes CTX_RL << 1, whatever the contexts say.  Columns that are not of that kind raise the flag at the
                // stripe's first row; the flags are ORed over the wave as act[] is (once per half), what stays clear is a fill.
                const bool any_rl = __any(rl != 0);
                unsigned fills = 0;
                if (any_rl) {
                    unsigned nof = Nh | (Nh >> 1);
                    nof = (nof | (nof >> 2) | ~rl) & 0x11111111u;
                    int wv = w;
                    asm volatile("" : "+s"(wv));
                    if (lane >= wv) nof = 0; // (columns outside the block: no say)
#define J2K_OR_STEP(ctrl, rmask) nof |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)nof, ctrl, rmask, 0xf, false);
                    J2K_OR_STEP(0x111, 0xf) J2K_OR_STEP(0x112, 0xf) J2K_OR_STEP(0x114, 0xf) J2K_OR_STEP(0x118, 0xf)
                    J2K_OR_STEP(0x142, 0xa) J2K_OR_STEP(0x143, 0xc)
#undef J2K_OR_STEP
                    fills = active & ~(unsigned)__builtin_amdgcn_readlane((int)nof, 63);
                    DADD(48, __builtin_popcount(fills));
                    if (fills == active) DCNT(49);
                }
                // ---- sample-wise writing of a sparse half: no stripe loop.  Every lane's bytes per stripe are counted on the
                // nibbles of V and N, the eight stripes' counts are scanned across the wave two to a register (16-bit fields:
                // a stripe holds at most 512 bytes), the stripe totals become stripe bases on the scalar unit -- the scan order
                // is stripe, column, row, [ZC][sign] per row, as the stripe loop writes it -- and then every lane walks its own
                // visited rows: the contexts are single bits of the planes formed below, the bytes go to its place in the stage.
                // The busiest lane sets the number of rounds.  A cleanup half with a run-length column stays dense.
                bool sparse = false;
                u64 q0 = 0, q1 = 0;
                unsigned sparse_total = 0;
                if (a.sparse >= 0 && !any_rl) {
                    // (rounds = the busiest lane's visited samples: no lane may have more than the break-even allows)
                    const unsigned dense_cost = kDenseStripe * (unsigned)__builtin_popcount(active);
                    if (a.sparse > 0 || !__any(kSparseHead + kSparseRound * (unsigned)__builtin_popcount(Vh) >= dense_cost)) {
                        const unsigned c = nibble_counts(Vh) + nibble_counts(Nh); // at most 8 per nibble
                        // register k: stripes k (low half) and k + 4 (high half)
                        const unsigned c0 = c & 0x000f000fu, c1 = (c >> 4) & 0x000f000fu, c2 = (c >> 8) & 0x000f000fu, c3 = (c >> 12) & 0x000f000fu;
                        unsigned t0, t1, t2, t3;
                        const unsigned e0 = prefix_count_dpp(c0, t0), e1 = prefix_count_dpp(c1, t1), e2 = prefix_count_dpp(c2, t2), e3 = prefix_count_dpp(c3, t3);
                        // (wave-uniform: the packed totals summed over the registers -- low halves: bytes of the stripes before k,
                        //  high halves: of the stripes 4 .. 3 + k; the first four stripes together come before every high one)
                        const unsigned a1 = t0 + t1, a2 = a1 + t2, a3 = a2 + t3;
                        const unsigned total = (a3 & 0xffffu) + (a3 >> 16);
                        if (total <= kBurst) {
                            sparse = true;
                            sparse_total = total;
                            DCNT(pt == 0 ? 7 : 8);
                            DADD(pt == 0 ? 14 : 15, total);
                            // stage offsets of the lane's first byte in each stripe, four to a 64-bit word: q0 = stripes 0, 4, 1, 5,
                            // q1 = stripes 2, 6, 3, 7
                            const unsigned org = (fill - flushed) * 0x10001u + (a3 << 16);
                            q0 = (u64)(e0 + org) | ((u64)(e1 + org + t0) << 32);
                            q1 = (u64)(e2 + org + a1) | ((u64)(e3 + org + a2) << 32);
                        } else DCNT(17);
                    }
                }
                // (a half whose active stripes are all fills needs none of the context planes)
                unsigned zb0 = 0, zb1 = 0, zb2 = 0, zb3 = 0, sb0 = 0, sb1 = 0, sb2 = 0, sd = 0;
                if (fills != active) {
                    // the eight neighbour masks with the timing of the stripe scan: left column new (its row below the stripe
                    // old), right column old (its row above the stripe new), row above new, row below old
                    const unsigned Wm1 = hf(LA << 1), W0 = hf(LA), Wp1 = hf(((LA >> 1) & ~M3) | (LO >> 1));
                    const unsigned Em1 = hf((RO << 1) | ((RA << 1) & M0)), E0 = hf(RO), Ep1 = hf(RO >> 1);
                    const unsigned Up = hf(A << 1), Dn = hf(O >> 1);
                    // ---- zero-coding contexts (Table D.1), bit-sliced: counts of significant horizontal / vertical / diagonal
                    // neighbours, then the table of the block's orientation as boolean expressions -> planes of the context 0..8
                    {
                        unsigned h1 = W0 ^ E0, h2 = W0 & E0, v1 = Up ^ Dn, v2 = Up & Dn; // exactly one / both
                        if (orient == 1) { const unsigned t1 = h1, t2 = h2; h1 = v1; h2 = v2; v1 = t1; v2 = t2; } // HL: swapped
                        const unsigned p = Wm1 ^ Wp1, q = Wm1 & Wp1, r_ = Em1 ^ Ep1, t = Em1 & Ep1;
                        const unsigned dodd = p ^ r_, dge1 = p | q | r_ | t, dge2 = (p & r_) | q | t;
                        const unsigned deq1 = dodd & ~dge2;
                        const unsigned hz = ~(h1 | h2), vnz = v1 | v2;
                        if (orient == 3) { // HH: diagonal count first, then min(h + v, 2)
                            const unsigned dge3 = (q & (r_ | t)) | (t & p);
                            const unsigned deq2 = dge2 & ~dge3, deq0 = ~dge1;
                            const unsigned hv0 = hz & ~vnz, hv1 = (h1 & ~vnz) | (hz & v1), hvge2 = ~(hv0 | hv1);
                            zb3 = dge3;
                            zb2 = deq2 | (deq1 & ~hv0);
                            zb1 = deq2 | (deq1 & hv0) | (deq0 & hvge2);
                            zb0 = (deq2 & ~hv0) | (deq1 & (hv0 | hvge2)) | (deq0 & hv1);
                        } else {
                            zb3 = h2;
                            zb2 = h1 | (hz & v2);
                            zb1 = (h1 & (vnz | dge1)) | (hz & (v1 | (~vnz & dge2)));
                            zb0 = (h1 & (vnz | ~dge1)) | (hz & (v1 | (~vnz & deq1)));
                        }
                    }
                    // ---- sign symbols (Tables D.2 / D.3), bit-sliced: contributions h, v in {-1, 0, +1} as two masks each;
                    // code = context - 9 (|h| = 1: 3, +1 if v agrees, -1 if it disagrees; h = 0: 1 if v != 0 else 0), decision bit =
                    // own sign XOR (h < 0 or (h = 0 and v < 0)); the symbol byte is 18 + 2 * code + decision
                    if (any_n) {
                        const unsigned cL = hf(from_left64(chi)), cR = hf(from_right64(chi)), cU = hf(chi << 1), cD = hf(chi >> 1);
                        const unsigned Wp = W0 & ~cL, Wn = W0 & cL, Ep = E0 & ~cR, En = E0 & cR;
                        const unsigned Upp = Up & ~cU, Upn = Up & cU, Dnp = Dn & ~cD, Dnn = Dn & cD;
                        const unsigned hp = (Wp & ~En) | (Ep & ~Wn), hn = (Wn & ~Ep) | (En & ~Wp);
                        const unsigned vp = (Upp & ~Dnn) | (Dnp & ~Upn), vn = (Upn & ~Dnp) | (Dnn & ~Upp);
                        const unsigned hnz = hp | hn, vnz = vp | vn;
                        const unsigned same = (hp & vp) | (hn & vn), opp = (hp & vn) | (hn & vp);
                        sb2 = same;
                        sb1 = hnz & ~same;
                        sb0 = (hnz & ~same & ~opp) | (~hnz & vnz);
                        sd = hf(chi) ^ (hn | (~hnz & vn));
                        if constexpr (BYPASS) {
                            if (pt == 0 && pass >= 10) sd = hf(chi); // raw pass (wave-uniform): the sign as it is
                        }
                    }
                }
                if (sparse) {
                    unsigned rest = Vh, pos = 0;
                    int cur = -1; // the stripe pos belongs to
                    while (__any(rest != 0)) {
                        DCNT(9);
                        if (rest) {
                            const int r = __builtin_ctz(rest);
                            rest &= rest - 1;
                            const int st = r >> 2;
                            if (st != cur) pos = (unsigned)((r & 8 ? q1 : q0) >> (((r & 4) << 3) | (r & 16))) & 0xffffu;
                            cur = st;
                            // (context << 1) | bit, one bit of each plane: bit extracts chained by shift-and-or
                            const auto bit = [&](unsigned plane) { return __builtin_amdgcn_ubfe(plane, (unsigned)r, 1u); };
                            stage[pos] = (unsigned char)((((((((bit(zb3) << 1) | bit(zb2)) << 1) | bit(zb1)) << 1) | bit(zb0)) << 1) | bit(bitsh));
                            ++pos;
                            if (bit(Nh)) {
                                stage[pos] = (unsigned char)(0x12u + ((((((bit(sb2) << 1) | bit(sb1)) << 1) | bit(sb0)) << 1) | bit(sd)));
                                ++pos;
                            }
                        }
                    }
                    commit(sparse_total);
                    continue;
                }
                DCNT(pt == 0 ? 12 : 13);
                // PairTab's index bytes of this half for the zero-coding bytes, even and odd stripes: (bit, zb0) and (zb1, zb2).  Formed
                // here, behind the sample-wise path, and only for a half with a stripe that is no fill: neither pays for them.  (The sign
                // planes keep their form and are indexed stripe by stripe: their four index words as well are more than 72 registers
                // hold, and pi went to scratch in every pass.  With DIST the stripes keep the multiplies: see kPairTabs.)
                unsigned zi0e = 0, zi0o = 0, zi1e = 0, zi1o = 0;
                if (kPairTabs && fills != active) {
                    pair_index(bitsh, zb0, zi0e, zi0o);
                    pair_index(zb1, zb2, zi1e, zi1o);
                }
                while (active) {
                    const int sl = __builtin_ctz(active) & ~3; // first row of the stripe inside the half
                    active &= active - 1;
                    if ((fills >> sl) & 1u) { // plain stores into the zeroed stage, as the sample-wise path does
                        int wv = w;
                        asm volatile("" : "+s"(wv));
                        if (lane < wv) stage[(fill - flushed) + lane] = (unsigned char)(CTX_RL << 1);
                        DADD(15, w);
                        commit((unsigned)w);
                        continue;
                    }
                    DCNT(pt == 0 ? 0 : 2);
                    const unsigned N = (Nh >> sl) & 0xfu;
                    unsigned Vz = (Vh >> sl) & 0xfu;
                    unsigned pc = 0, rlsym = 0; // run-length prefix of this lane (cleanup): 0, 1 (RL) or 3 (RL, UNI, UNI) decisions
                    if (pt != 0) {
                        if ((rl >> sl) & 1u) { // run-length mode
                            const int runlen = N ? __ffs((int)N) - 1 : 4;
                            rlsym = (CTX_RL << 1) | (runlen != 4 ? 1u : 0u);
                            pc = 1;
                            Vz = 0;
                            if (runlen != 4) {
                                rlsym |= (((CTX_UNI << 1) | (unsigned)(runlen >> 1)) << 8) | (((CTX_UNI << 1) | (unsigned)(runlen & 1)) << 16);
                                pc = 3;
                                Vz = 0xfu & ~((2u << runlen) - 1u); // rows below the first 1 bit; that row itself: sign only
                            }
                        }
                    }
                    // (the selector look-up and the stage offsets first: their latencies hide behind the decision bytes)
                    const u64 sel = DIST ? kPackSel.v[Vz | (N << 4)] : sel_tab[Vz | (N << 4)];
                    const unsigned cnt = pc + (unsigned)__builtin_popcount(Vz) + (unsigned)__builtin_popcount(N);
                    unsigned total;
                    const unsigned base = reserve(cnt, std::integral_constant<int, 10>(), total);
                    unsigned zsym = 0, ssym = 0; // decision bytes of the four rows: zero coding / sign
                    const auto nib = [&](unsigned plane) { return __builtin_amdgcn_ubfe(plane, (unsigned)sl, 4u); };
                    if constexpr (kPairTabs) {
                        // The stripe's index byte: byte sl / 8 of the even or the odd word, picked by one v_perm whose selector is formed
                        // on the scalar unit (bytes 0..3: the second operand, 4..7: the first; 0x0c: a zero byte)
                        const unsigned pick = 0x0c0c0c00u | ((unsigned)sl >> 3) | ((unsigned)sl & 4u);
                        if (__any(Vz != 0)) // (context << 1) | bit
                            zsym = pair_entry(__builtin_amdgcn_perm(zi0o, zi0e, pick)) | (pair_entry(__builtin_amdgcn_perm(zi1o, zi1e, pick)) << 2) |
                                   (spread4(nib(zb3)) << 4);
                        if (__any(N != 0))
                            ssym = 0x12121212u + pair_entry(nib(sd) | (nib(sb0) << 4)) + (pair_entry(nib(sb1) | (nib(sb2) << 4)) << 2);
                    } else {
                        if (__any(Vz != 0))
                            zsym = (spread4(nib(zb0)) << 1) | (spread4(nib(zb1)) << 2) | (spread4(nib(zb2)) << 3) | (spread4(nib(zb3)) << 4) | spread4(nib(bitsh));
                        if (__any(N != 0))
                            ssym = 0x12121212u + (spread4(nib(sb0)) << 1) + (spread4(nib(sb1)) << 2) + (spread4(nib(sb2)) << 3) + spread4(nib(sd));
                    }
                    {
                        // The lane's bytes in coding order, [RL][UNI][UNI] then row by row [ZC][sign], packed in registers:
                        // one v_perm per output word picks the present rows' bytes out of zsym / ssym, the run-length prefix
                        // shifts them up (with a prefix of 1 there are no others; with 3 at most 7)
                        const unsigned c0 = __builtin_amdgcn_perm(ssym, zsym, (unsigned)sel), c1 = __builtin_amdgcn_perm(ssym, zsym, (unsigned)(sel >> 32));
                        const u64 d = (((u64)c1 << 32) | c0) << (8 * pc);
                        emit(base, cnt, (unsigned)d | rlsym, (unsigned)(d >> 32), __builtin_amdgcn_ubfe(c1, 8, 8 * pc));
                        DADD(pt == 0 ? 14 : 15, total);
                        commit(total);
                    }
                }
            }
            sigma = A;
            }
            }
            if (pt == 2) pi = 0;
            if constexpr (DIST) {
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) nm += __shfl_xor(nm, o);
            }
            if (lane == 0) { pass_nsym[pass] = fill; pass_nmsedec[pass] = nm; }
            ++pass;
        }
    }
    // drain the stage
    __builtin_amdgcn_wave_barrier();
    const unsigned rest = fill - flushed;
    if (lane * 16u < rest) {
        if (flushed + lane * 16u + 16u <= symcap) {
            const uint4 v = *reinterpret_cast<const uint4 *>(&stage[lane * 16]);
            *reinterpret_cast<uint4 *>(symout + flushed + lane * 16) = v;
        } else overflow = true;
    }
#ifdef J2K_T1_COUNTERS
    if (lane == 0 && a.dbg) for (int i = 0; i < kT1Counters; ++i) if (dc[i]) atomicAdd(a.dbg + i, dc[i]);
#endif
    const bool ovf = __any(overflow);
    if (ovf && lane == 0) a.err[0] = 2u; // decision stream capacity exceeded: the call fails, the coder must not run on it
    if (lane == 0) { a.numbps[b] = (unsigned)numbps; a.npasses[b] = ovf ? 0u : (unsigned)pass; a.nsym[b] = ovf ? 0u : fill; }
    report();
}

// ------------------------------------------------------------------------------------------------
// MQ coder (T.800 Annex C); Table C.2 lives in t1_common.h.
// The two-wave coder's state word: Qe in the high half (the interval register lives there too: its leading zeros are the
// renormalisation shift as they stand), below it the byte offset of the state's entry in the transition table `trans`:
// the index from bit 2, the MPS sense at bit 8 and once more at bit 9, where the decision's bit meets it.
// (state ^ bit << 9) & 0x3fc is the address of the entry to take -- one v_bitop3 -- and "less probable symbol" is its top bit:
// one compare.  (The flag at bit 2, under the index, takes an AND more per decision to test.)
constexpr unsigned mq2_slot(unsigned idx, unsigned mps, unsigned lps) { return idx | (mps << 6) | (lps << 7); } // word index in `trans`
constexpr unsigned kMq2LpsBit = 9; // of the entry's byte address
constexpr bool mq2_slots_ok()
{
    bool seen[256] = {};
    for (unsigned idx = 0; idx < 47; ++idx)
        for (unsigned mps = 0; mps < 2; ++mps)
            for (unsigned lps = 0; lps < 2; ++lps) {
                const unsigned w = mq2_slot(idx, mps, lps), addr = w * 4u;
                if (w >= 256u || seen[w] || (addr & 3u) || (addr & ~0x3fcu)) return false;
                // (what the look-up relies on: the lps flag is one bit of the address, and without it the address is the state's own field)
                if (addr != ((mq2_slot(idx, mps, 0) * 4u) ^ (lps << kMq2LpsBit))) return false;
                seen[w] = true;
            }
    return true;
}
static_assert(mq2_slots_ok(), "trans: (index, sense, lps) -> word index must be injective over 47 x 2 x 2, below 256, and a word address within 0x3fc");
__device__ __forceinline__ unsigned ctx_word2(unsigned qe, unsigned idx, unsigned mps) { return (qe << 16) | (mq2_slot(idx, mps, 0) << 2) | (mps << kMq2LpsBit); }

// ------------------------------------------------------------------------------------------------
// Two-wave MQ coder.  The coder state splits into two recurrences that only talk one way:
//   stage 1 (interval A + probability states): decision -> Qe, MPS/LPS, renormalisation shift n
//   stage 2 (code register C, counter CT, pending byte B): += addend, << n, BYTEOUTs, pass rates
// Stage 1 never needs C/CT/B, so a workgroup runs them as a producer wave and a consumer wave on
// different SIMDs, 64 blocks each (lane = block), joined by a double-buffered LDS queue of
// {addend | n << 16} words (in a plain frame: of groups of four, summed) that is handed over once per 16 decisions (one barrier).  The serial
// chain per decision is cut roughly in half.
// Staged codeword bytes per lane of the two-wave coder.  (As a ring of 256 -- the ring index a byte of the count -- it coded a
// frame alone 1 % sooner, but its 8 KiB more of LDS per workgroup cost 3 % with frames in flight (8020 against 8280 Mpixel/s
// on one box) and the DWT launches beside the coders a tenth of their rate.  The stage is no ring any more: see the consumer.)
#ifndef J2K_MQ2_RING
#define J2K_MQ2_RING 128
#endif
constexpr unsigned kRing = J2K_MQ2_RING;
// RATES: the consumer also keeps the byte count at the end of every coding pass (pass_rate: rate control, and the stage hook on
// request).  A plain frame reads none of them: without the parameter the consumer has no pass-end tests, one copy of its
// decision loop, and neither loads pass_nsym nor stores pass_rate.  Codeword, lengths, flush, errors and gates are the same.
template <bool RATES>
__global__ __launch_bounds__(128) void t1_mq2_kernel(T1Args a)
{
    __shared__ unsigned ctxs[19 * 64];
    // [mq2_slot(index, mps, lps)]: the context word after an MPS / an LPS out of state (index, mps): MPS sense and SWITCH folded in.
    // One 32-bit word per look-up -- the producer knows which of the two it wants before it asks -- instead of the pair:
    // half the LDS bytes of the gather, whose bank conflicts were a third of this kernel's LDS-active cycles (profiles/r2_t1_pmc.txt)
    __shared__ unsigned trans[256];
    // [buffer][decision / 4][lane]; without RATES the same 16 bytes per lane and group as two halves of eight, [buffer][decision / 4][half][lane]
    __shared__ uint4 queue[2][4][64];
    __shared__ __attribute__((aligned(16))) unsigned ostage[(kRing / 4 + 1) * 64]; // per lane one pad word, then kRing bytes: stride kRing + 4 B (an odd number of banks), conflict-free byte-out stores
    __shared__ unsigned finalA[64];   // the producer's interval register after the last decision (FLUSH needs it)
    const int lane = threadIdx.x & 63;
    const bool producer = threadIdx.x < 64;
    // gated: this workgroup's blocks are gate_groups[first + blockIdx]; it sleeps until the modeller has reported all of them
    __shared__ int gate_ok;
    T1Args::GateGroup gg{};
    bool gated_out = false;
    if (a.gate_groups) {
        gg = a.gate_groups[a.first + (int)blockIdx.x];
        if (threadIdx.x == 0) {
            unsigned polls = 0;
            int ok = 1;
            while (__hip_atomic_load(a.gate_ready + a.first + (int)blockIdx.x, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < gg.count) {
                __builtin_amdgcn_s_sleep(127); // ~4 us
                if (++polls > a.gate_budget || (a.gate_abort && __hip_atomic_load(a.gate_abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) { ok = 0; break; }
            }
            gate_ok = ok;
        }
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        gated_out = gate_ok == 0;
        if (gated_out && threadIdx.x == 0) a.err[0] = 4u; // the blocks were never modelled (the call failed half way, or the wait ran out)
        set_priority(a.mq_prio ? (int)gg.prio : 0);
    } else set_priority(a.mq_prio);
    const int b = a.gate_groups ? (int)gg.first + lane : a.first + (int)blockIdx.x * 64 + lane;
    if (producer) {
        if (lane < 47) {
            trans[mq2_slot(lane, 0, 0)] = ctx_word2(kQe[kNmps[lane]], kNmps[lane], 0);
            trans[mq2_slot(lane, 1, 0)] = ctx_word2(kQe[kNmps[lane]], kNmps[lane], 1);
            trans[mq2_slot(lane, 0, 1)] = ctx_word2(kQe[kNlps[lane]], kNlps[lane], kSwitch[lane]);
            trans[mq2_slot(lane, 1, 1)] = ctx_word2(kQe[kNlps[lane]], kNlps[lane], 1u ^ kSwitch[lane]);
        }
#pragma unroll
        for (int c = 0; c < 19; ++c) {
            const unsigned idx = c == CTX_UNI ? 46u : (c == CTX_RL ? 3u : (c == 0 ? 4u : 0u));
            ctxs[c * 64 + lane] = ctx_word2(kQe[idx], idx, 0);
        }
    }
    const bool live = a.gate_groups ? (lane < (int)gg.count && !gated_out) : b < a.nblks;
    CblkDev cb = {};
    unsigned nsym = 0, npasses = 0;
    if (live) { cb = a.blks[b]; nsym = a.nsym[b]; npasses = a.npasses[b]; }
    unsigned maxsym = nsym;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) maxsym = max(maxsym, (unsigned)__shfl_xor((int)maxsym, o));
    const unsigned nchunks = (unsigned)__builtin_amdgcn_readfirstlane((int)((maxsym + 15) / 16)); // wave-uniform loop bound
    __syncthreads();

    if (producer) {
        const unsigned char *sym = a.sym + cb.sym_off;
        unsigned A = 0x80000000u; // (the interval register, in the high half)
        uint4 next = make_uint4(0, 0, 0, 0);
        if (nsym) next = *reinterpret_cast<const uint4 *>(sym);
        unsigned yield_budget = 2048; // polls of ~2 us: every wave moves on whatever the word says
#ifdef J2K_MQ_TIMES
        long long tw_ = 0, tb_ = 0;
#endif
        for (unsigned c = 0; c <= nchunks; ++c) {
#ifdef J2K_MQ_TIMES
            const long long t0_ = __builtin_readcyclecounter();
#endif
            // While another frame's DWT launches are running (yield_word != 0) the coder waves step aside: the
            // bandwidth-bound DWT waves get the SIMDs' issue slots to themselves for those ~0.35 ms.  The consumer
            // wave needs no poll of its own: it sleeps at the barrier below.
            if (a.yield_word && (c & 3u) == 0) {
                while (yield_budget && __builtin_amdgcn_readfirstlane((int)__hip_atomic_load(a.yield_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
                    __builtin_amdgcn_s_sleep(64);
                    --yield_budget;
                }
            }
            if (c < nchunks) {
                const unsigned base = c * 16;
                const uint4 chunk = next;
                if (base + 16 < nsym) next = *reinterpret_cast<const uint4 *>(sym + base + 16);
                const unsigned words[4] = {chunk.x, chunk.y, chunk.z, chunk.w};
                const int rem = (int)min(nsym - min(base, nsym), 16u);
                // One decision: the context's word, the transition it may take (asked for as soon as the word is there),
                // the interval.  Both table addresses come from byte permutes of values formed once per four symbols: the
                // context word's is the context number above lane * 4 (both fit a byte), the transition entry's the state
                // word's low bits xor the decision's bit at bit 9 -- the tables' own offsets ride in the instructions.
                unsigned char *const ctx_b = reinterpret_cast<unsigned char *>(ctxs);
                const unsigned char *const trans_b = reinterpret_cast<const unsigned char *>(trans);
                const unsigned lane4 = (unsigned)lane * 4u;
                // c4: the four symbols' context numbers, one byte each; b4: the symbols (context << 1 | bit < 128) shifted up by
                // one: a symbol's byte, moved to byte 1, has its bit at bit 9 and nothing else under the mask; jj: which of the four
                // What goes to the consumer under RATES is {addend | shift << 16}, the value returned; otherwise the group
                // is summed (below) from q, the decision's addend still in the high half, and nn, its shift.
                auto decide = [&](unsigned c4, unsigned b4, auto jj_, unsigned &q, unsigned &nn) -> unsigned {
                    constexpr unsigned jj = decltype(jj_)::value;
                    unsigned *const cp = reinterpret_cast<unsigned *>(ctx_b + __builtin_amdgcn_perm(c4, lane4, 0x0c0c0400u + (jj << 8)));
                    const unsigned st = *cp;
                    const unsigned ta = (st ^ __builtin_amdgcn_perm(b4, 0u, 0x0c0c040cu + (jj << 8))) & 0x3fcu;
                    const unsigned tr = *reinterpret_cast<const unsigned *>(trans_b + ta);
                    const bool mps = ta < (1u << kMq2LpsBit); // the more probable symbol
                    const unsigned qe = st & 0xffff0000u;
                    const unsigned A1 = A - qe;
                    const bool use_a1 = (A1 >= qe) == mps; // MPS: keep A1 unless conditional exchange; LPS: the reverse
                    A = use_a1 ? A1 : qe;
                    const bool renorm = (int)A >= 0;
                    *cp = renorm ? tr : st;
                    const unsigned n = (unsigned)__builtin_clz(A);
                    A <<= n;
                    if constexpr (RATES) return __builtin_amdgcn_alignbit(n, use_a1 ? qe : 0u, 16);
                    q = use_a1 ? qe : 0u;
                    nn = n;
                    return 0u;
                };
                // Without RATES the group goes over summed (t1_mq_window.h): {G, shifts} in one 8-byte half of the lane's 16 bytes
                // -- all the consumer reads unless the group is coded again -- and the addends in the other; the halves of the
                // 64 lanes lie together, so that either is read at eight bytes a lane without a bank conflict.
                auto send = [&](const int g, const unsigned (&q)[4], const unsigned (&n)[4]) {
                    unsigned G = 0, N = 0, shifts = 0;
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        mq_group_add(G, N, q[jj] >> 16, n[jj]);
                        shifts = mq_group_add_shift(shifts, n[jj], (unsigned)jj);
                    }
                    uint2 *const half = reinterpret_cast<uint2 *>(queue) + ((c & 1) * 4 + g) * 128 + lane;
                    half[0] = make_uint2(G, shifts);
                    half[64] = make_uint2(mq_group_pack_addends_high(q[0], q[1]), mq_group_pack_addends_high(q[2], q[3]));
                };
                if (__all(rem == 16)) { // every lane has a full chunk: no per-decision test for the lane's end
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const unsigned c4 = (words[g] >> 1) & 0x1f1f1f1fu, b4 = words[g] << 1;
                        unsigned e[4], q[4], n[4];
                        e[0] = decide(c4, b4, std::integral_constant<unsigned, 0>(), q[0], n[0]);
                        e[1] = decide(c4, b4, std::integral_constant<unsigned, 1>(), q[1], n[1]);
                        e[2] = decide(c4, b4, std::integral_constant<unsigned, 2>(), q[2], n[2]);
                        e[3] = decide(c4, b4, std::integral_constant<unsigned, 3>(), q[3], n[3]);
                        if constexpr (RATES) queue[c & 1][g][lane] = make_uint4(e[0], e[1], e[2], e[3]);
                        else send(g, q, n);
                    }
                } else
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const unsigned c4 = (words[g] >> 1) & 0x1f1f1f1fu, b4 = words[g] << 1;
                    if constexpr (RATES) {
                        unsigned e[4] = {0, 0, 0, 0}, q, n;
                        if (4 * g + 0 < rem) e[0] = decide(c4, b4, std::integral_constant<unsigned, 0>(), q, n);
                        if (4 * g + 1 < rem) e[1] = decide(c4, b4, std::integral_constant<unsigned, 1>(), q, n);
                        if (4 * g + 2 < rem) e[2] = decide(c4, b4, std::integral_constant<unsigned, 2>(), q, n);
                        if (4 * g + 3 < rem) e[3] = decide(c4, b4, std::integral_constant<unsigned, 3>(), q, n);
                        queue[c & 1][g][lane] = make_uint4(e[0], e[1], e[2], e[3]);
                    } else {
                        // (the four words summed in place, each decision's share under the decision's own mask: four zeros to
                        //  start from instead of eight, and a decision past the lane's end leaves every field as it is)
                        unsigned G = 0, N = 0, shifts = 0, a[2] = {0, 0};
                        auto one = [&](auto jj_) {
                            constexpr unsigned jj = decltype(jj_)::value;
                            unsigned q, n;
                            decide(c4, b4, jj_, q, n);
                            mq_group_add(G, N, q >> 16, n);
                            shifts = mq_group_add_shift(shifts, n, jj);
                            a[jj >> 1] = (jj & 1u) ? mq_group_pack_addends(a[jj >> 1], q >> 16) : q >> 16;
                        };
                        if (4 * g + 0 < rem) one(std::integral_constant<unsigned, 0>());
                        if (4 * g + 1 < rem) one(std::integral_constant<unsigned, 1>());
                        if (4 * g + 2 < rem) one(std::integral_constant<unsigned, 2>());
                        if (4 * g + 3 < rem) one(std::integral_constant<unsigned, 3>());
                        uint2 *const half = reinterpret_cast<uint2 *>(queue) + ((c & 1) * 4 + g) * 128 + lane;
                        half[0] = make_uint2(G, shifts);
                        half[64] = make_uint2(a[0], a[1]);
                    }
                }
            } else {
                finalA[lane] = A >> 16; // last iteration: nothing left to produce
            }
#ifdef J2K_MQ_TIMES
            const long long t1_ = __builtin_readcyclecounter();
            __syncthreads();
            tw_ += t1_ - t0_; tb_ += __builtin_readcyclecounter() - t1_;
#else
            __syncthreads();
#endif
        }
#ifdef J2K_MQ_TIMES
        if (lane == 0 && a.dbg) { atomicAdd(a.dbg + 0, (unsigned long long)tw_); atomicAdd(a.dbg + 1, (unsigned long long)tb_); atomicAdd(a.dbg + 4, (unsigned long long)nchunks); atomicAdd(a.dbg + 5, 1ull); }
#endif
        return;
    }

    // ---- consumer: code register, byte output, pass rates
    unsigned char *out = a.out + cb.out_off;
    const unsigned *pass_nsym = a.pass_nsym + (size_t)(live ? b : 0) * kDevMaxPasses;
    unsigned *pass_rate = a.pass_rate + (size_t)(live ? b : 0) * kDevMaxPasses;
    unsigned char *ostage_b = reinterpret_cast<unsigned char *>(ostage);
    unsigned C = 0, CT = 12, B = 0;
    // Without RATES the state carried from group to group is the wide register of t1_mq_window.h -- (C, CT, B) as one number --
    // unless the knob mq_window says otherwise: -1 = every group per decision on (C, CT, B), as under RATES; 2 = every group
    // accumulated and peeled, then sent back and coded per decision, through both conversions; 3 = every lane reports every
    // group long: sent back before anything is peeled.  No byte depends on it.
    bool window = false, window_again = false, window_long = false;
    if constexpr (!RATES) { window = a.mq_window >= 0; window_again = a.mq_window == 2; window_long = a.mq_window == 3; }
    MqWide wide = mq_wide_from(C, CT, B);
    int flushed = 0;
    bool overflow = false;
    // The lane's stage: its data bytes start at dbase, and the byte at dbase is number `flushed` of the codeword.  `pos` is
    // where the next candidate byte goes -- an offset into ostage: the array's own address rides in the store -- and the byte
    // count is derived from it where it is needed.  Before the first byte (count -1) it points at the pad word's last byte.
    const unsigned dbase = (unsigned)lane * (kRing + 4u) + 4u;
    unsigned pos = dbase - 1u;
    auto nbytes = [&]() -> int { return (int)(pos - dbase) + flushed; };
    // BYTEOUT (Figure C.3) for the lanes in `p`, by selects.  (An explicit masked block -- `if (p) { ... }` -- was measured
    // on the same box: 5900 instead of 7050 Mpixel/s.)  Every lane stores its candidate byte at `pos` -- the next one to become valid: lanes not in `p` only
    // scribble on a slot that their next committed byte overwrites (count -1: the pad byte, never read)
    auto byteout = [&](bool p) {
        const bool was_ff = B == 0xffu;
        const unsigned Bc = B + ((C > 0x7ffffffu && !was_ff) ? 1u : 0u); // the carry goes into the byte before -- unless that is a 0xFF
        const bool stuff = Bc == 0xffu;
        const unsigned sh = stuff ? 20u : 19u, ct = 27u - sh;
        // the next byte: ct bits from `sh` up -- the carry above them has gone into Bc -- or, behind a 0xFF, eight: there the
        // carry stays with its byte
        const unsigned bw = was_ff ? 8u : ct;
        ostage_b[pos] = (unsigned char)Bc;
        B = p ? __builtin_amdgcn_ubfe(C, sh, bw) : B; C = p ? __builtin_amdgcn_ubfe(C, 0u, sh) : C; CT = p ? ct : CT; pos += p ? 1u : 0u;
        asm("" : "+v"(pos)); // (one register for the pointer: left to itself the compiler forms it a second time for the next store)
    };
    unsigned cur_pass = 0;
    unsigned next_end = 0xffffffffu;
    if constexpr (RATES) next_end = npasses ? pass_nsym[0] : 0xffffffffu;
    auto close_passes = [&](unsigned i) {
        while (cur_pass < npasses && i == next_end) {
            pass_rate[cur_pass] = (unsigned)(nbytes() + 3);
            ++cur_pass;
            next_end = cur_pass < npasses ? pass_nsym[cur_pass] : 0xffffffffu;
        }
    };
#ifdef J2K_MQ_TIMES
    long long tw_ = 0, tb_ = 0;
#endif
    for (unsigned c = 0; c <= nchunks; ++c) {
#ifdef J2K_MQ_TIMES
        const long long t0_ = __builtin_readcyclecounter();
#endif
        if (c >= 1) {
            const unsigned base = (c - 1) * 16;
            int rel = 64;
            if constexpr (RATES) rel = (int)min(next_end - base, 64u);
            // four decisions; CHECK = a coding pass of some lane ends among them (its byte count is taken then)
            auto four = [&](auto check, const unsigned (&e)[4], const int g) {
                constexpr bool ENDS = decltype(check)::value;
                {
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        const int j = 4 * g + jj;
                        // (no test for the lane's end: past it the producer queues zeros -- addend 0, shift 0: a decision that changes nothing)
                        C += e[jj] & 0xffffu;
                        unsigned n = e[jj] >> 16;
                        {
                            const bool p = n >= CT;
                            const unsigned k = p ? CT : 0u;
                            C <<= k; n -= k;
                            byteout(p);
                        }
                        // (n <= 15 and a byte takes 7 or 8 shifts: three BYTEOUTs at most, so two plain tests instead of a loop --
                        //  a loop's carried registers cost a copy each on every decision, and with the byte count's update
                        //  sunk into its header a lane mask went through every decision as well)
                        if (__any(n >= CT)) {
                            const bool p2 = n >= CT;
                            const unsigned k2 = p2 ? CT : 0u;
                            C <<= k2; n -= k2;
                            byteout(p2);
                            if (__any(n >= CT)) {
                                const bool p3 = n >= CT;
                                const unsigned k3 = p3 ? CT : 0u;
                                C <<= k3; n -= k3;
                                byteout(p3);
                            }
                        }
                        C <<= n; CT -= n;
                        if constexpr (ENDS) {
                            // (a plain divergent branch: the compiler skips an empty one by itself; an __any around it costs five instructions more)
                            if (rel == j + 1) { close_passes(base + j + 1); rel = (int)min(next_end - base, 64u); }
                        }
                    }
                }
            };
            // the sixteen decisions of the chunk.  Pass ends are looked for group by group: with 64 lanes nearly every chunk has one
            // somewhere, but four groups in five have none, and their decisions go without the test.
            // (Without RATES there is nothing to look for: one copy of the decisions, no test.)
            bool ends_here = false;
            if constexpr (RATES) ends_here = __any(rel <= 16);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if constexpr (RATES) {
                    const uint4 q = queue[(c - 1) & 1][g][lane];
                    const unsigned e[4] = {q.x, q.y, q.z, q.w};
                    if (ends_here && __any(rel > 4 * g && rel <= 4 * g + 4)) four(std::true_type(), e, g);
                    else four(std::false_type(), e, g);
                } else {
                    // The group as the producer summed it (t1_mq_window.h): V = (V << N) + G, then as many peel rounds as the
                    // busiest lane has bytes -- one BYTEOUT's worth of selects per round instead of per decision.  The wave codes
                    // the group per decision from its starting state -- the peel's bytes lie behind `pos` and are written over --
                    // if some lane reports that it is not exact that way: its shifts sum to more than 15 (G is not whole), a
                    // carry above a 0xFF, or a byte that reads 0x00 and whose top boundary a carry crossed.  Only then are the
                    // four {addend, shift} read and unpacked.
                    const uint2 *const half = reinterpret_cast<const uint2 *>(queue) + (((c - 1) & 1) * 4 + g) * 128 + lane;
                    uint2 q = half[0];
                    asm("" : "+v"(q.x), "+v"(q.y)); // (one 8-byte load: left to itself the compiler reads the two words apart, G only where it is used, and two 4-byte reads at 8 bytes a lane meet in the banks)
                    bool again = true; // (wave-uniform from here on)
                    const MqWide wide0 = wide;
                    const unsigned pos0 = pos;
                    if (window) {
                        const unsigned N = mq_group_N(q.y);
                        mq_wide_add_group(wide, q.x, N);
                        again = __any(window_long || mq_group_is_long(N) || mq_wide_has_carry(wide));
                        if (!again) {
                            const unsigned long long V_after = wide.V;
                            unsigned zpos = kMqNoZero;
                            // (a group that is not long ends below 50 bits and a round takes 7 or 8 off: three rounds at most, so
                            //  plain tests instead of a loop, whose carried registers cost a copy each on every round)
                            static_assert(kMqExactMax + kMqGroupMaxN - 3u * 7u < kMqWideDue, "three peel rounds must do");
                            auto round = [&]() {
                                const bool due = mq_wide_due(wide);
                                const unsigned byte = mq_wide_peel_mark(wide, due, zpos);
                                ostage_b[pos] = (unsigned char)byte;
                                pos += due ? 1u : 0u;
                            };
                            if (__any(mq_wide_due(wide))) {
                                round();
                                if (__any(mq_wide_due(wide))) {
                                    round();
                                    if (__any(mq_wide_due(wide))) round();
                                }
                            }
                            again = window_again;
                            if (__any(zpos != kMqNoZero)) again = __any(window_again || mq_group_rolled(V_after, wide0.V, N, zpos));
                        }
                    }
                    if (again) {
                        const uint2 r = half[64];
                        unsigned e[4];
#pragma unroll
                        for (unsigned jj = 0; jj < 4; ++jj) e[jj] = mq_group_decision(q.y, r.x, r.y, jj);
                        if (window) { pos = pos0; mq_wide_to(wide0, C, CT, B); }
                        four(std::false_type(), e, g);
                        if (window) wide = mq_wide_from(C, CT, B);
                    }
                }
            }
            // Codeword bytes leave the stage in 16-byte units, every lane's at once: when some lane has 64 waiting, all lanes send
            // the whole units they have.  (Each lane on its own -- 64 bytes whenever it had them -- ran this code in five chunks
            // out of six: with 64 lanes somebody is always due.  Together it runs once in thirty.)  Then each lane moves what is
            // left -- fewer than 16 bytes and the candidate's slot: four words -- to the front of its stage and pulls `pos` back.
            // A chunk adds fewer than 48 bytes to a lane, so fewer than 64 + 48 = 112 ever wait: the candidate's slot is at most
            // data byte 111 of the lane's kRing = 128, and the move reads no further than byte 6 * 16 + 15.
            // (Per decision: a shift of at most 15 and 7 or 8 shifts to a byte, three BYTEOUTs -- 12 a group.  On the wide
            // register a group peels at most three -- it starts below 35 bits, is peeled only if its shifts sum to 15 at most, and
            // a round takes 7 or 8 off -- and a group that is sent back starts again at the `pos` it began with: 12 bounds both,
            // 48 a chunk.)
            const int waiting = (int)(pos - dbase); // (nothing yet: -1)
            if (__any(waiting >= 64)) {
                const int units = waiting >> 4; // (-1 -> -1)
                for (int u = 0; u < 7; ++u) {
                    if (!__any(u < units)) break;
                    if (u < units) {
                        if ((unsigned)(flushed + 16) <= cb.out_cap) {
                            const unsigned *sp = reinterpret_cast<const unsigned *>(ostage_b + dbase + 16 * u);
                            *reinterpret_cast<uint4 *>(out + flushed) = make_uint4(sp[0], sp[1], sp[2], sp[3]);
                        } else overflow = true;
                        flushed += 16;
                    }
                }
                if (units > 0) {
                    const unsigned *sp = reinterpret_cast<const unsigned *>(ostage_b + dbase + 16 * units);
                    unsigned *dp = reinterpret_cast<unsigned *>(ostage_b + dbase);
                    const unsigned r0 = sp[0], r1 = sp[1], r2 = sp[2], r3 = sp[3];
                    dp[0] = r0; dp[1] = r1; dp[2] = r2; dp[3] = r3;
                    pos -= 16u * (unsigned)units;
                }
            }
        }
#ifdef J2K_MQ_TIMES
        const long long t1_ = __builtin_readcyclecounter();
        __syncthreads();
        tw_ += t1_ - t0_; tb_ += __builtin_readcyclecounter() - t1_;
#else
        __syncthreads();
#endif
    }
#ifdef J2K_MQ_TIMES
    if (lane == 0 && a.dbg) { atomicAdd(a.dbg + 2, (unsigned long long)tw_); atomicAdd(a.dbg + 3, (unsigned long long)tb_); }
#endif
    if constexpr (!RATES) {
        if (window) mq_wide_to(wide, C, CT, B); // FLUSH runs on (C, CT, B)
    }
    const bool fin = live && npasses;
    const unsigned A = finalA[lane]; // written by the producer before the last barrier
    if (fin) {
        if constexpr (RATES) close_passes(nsym);
        const unsigned tempc = C + A;
        C |= 0xffffu;
        if (C >= tempc) C -= 0x8000u;
    }
    C <<= CT; byteout(fin);
    C <<= CT; byteout(fin);
    if (fin && B != 0xffu) {
        ostage_b[pos] = (unsigned char)B;
        ++pos;
    }
    const int nb = nbytes();
    if (fin) {
        for (int o = flushed; o < nb; o += 4) {
            if ((unsigned)(o + 4) <= cb.out_cap) *reinterpret_cast<unsigned *>(out + o) = *reinterpret_cast<const unsigned *>(ostage_b + dbase + (o - flushed));
            else overflow = true;
        }
        if constexpr (RATES) pass_rate[npasses - 1] = (unsigned)nb;
        a.len[b] = (unsigned)nb;
        if (overflow) a.err[0] = 3u;
    } else if (live) {
        a.len[b] = 0;
    } else if (a.gate_groups && lane < (int)gg.count) {
        a.len[b] = 0; // (a group that was never modelled: nothing of it goes into a file -- the call fails -- but the packing must not read garbage)
    }
    if (a.gate_groups) { // the consumer wave is the workgroup's last: its codewords and lengths are out
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        if (lane == 0) __hip_atomic_fetch_add(a.gate_done + gg.stage, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The reference's fix-ups of the per-pass byte counts (OpenJPEG opj_t1_encode_cblk): an estimate never
// exceeds what follows it, and a pass never ends on 0xFF.  One thread per block, after its coder -- either coder: under a
// code-block style the rules are the same ones (a terminated pass holds its exact count and never ends on 0xFF by itself).
__global__ void t1_rate_fixup_kernel(T1Args a)
{
    const int b = a.first + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= a.nblks) return;
    const unsigned np = a.npasses[b];
    unsigned *rate = a.pass_rate + (size_t)b * kDevMaxPasses;
    const unsigned char *bytes = a.out + a.blks[b].out_off;
    unsigned last = a.len[b];
    for (unsigned p = np; p > 0;) { --p; if (rate[p] > last) rate[p] = last; else last = rate[p]; }
    for (unsigned p = 0; p < np; ++p)
        if (rate[p] > 0 && bytes[rate[p] - 1] == 0xffu) --rate[p];
}

// One sleeping wave holds a stream until *word has reached `target` (agent-scope polling) or about
// `timeout_us` microseconds have passed -- whichever comes first, so the stream always moves on.
__global__ void wait_word_kernel(const unsigned *word, unsigned target, unsigned timeout_us)
{
    for (unsigned i = 0; i < timeout_us; ++i) {
        if ((int)(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - target) >= 0) return;
        __builtin_amdgcn_s_sleep(32); // 32 x 64 clocks ~ 1 us
    }
}

// Holds a stream until *word >= target -- a stage's coder workgroups have all reported -- bounded like wait_word_kernel; gives up
// with *err = 5 (the launches behind it then work on whatever is there; the call fails on the error word).
__global__ void wait_count_kernel(const unsigned *word, unsigned target, unsigned timeout_us, const unsigned *abort, unsigned *err)
{
    for (unsigned i = 0; i < timeout_us; i += 2) {
        if (__hip_atomic_load(word, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) >= target) return;
        if (abort && __hip_atomic_load(abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
        __builtin_amdgcn_s_sleep(64); // ~2 us
    }
    if (threadIdx.x == 0) *err = 5u;
}

__global__ void set_word_kernel(unsigned *word, unsigned value, unsigned *word2, unsigned value2)
{
    if (threadIdx.x == 0) {
        if (word2) __hip_atomic_store(word2, value2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(word, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

} // namespace

void launch_wait_word(const unsigned *word, unsigned target, unsigned timeout_us, hipStream_t s)
{
    hipLaunchKernelGGL(wait_word_kernel, dim3(1), dim3(64), 0, s, word, target, timeout_us);
}

void launch_wait_count(const unsigned *word, unsigned target, unsigned timeout_us, const unsigned *abort, unsigned *err, hipStream_t s)
{
    hipLaunchKernelGGL(wait_count_kernel, dim3(1), dim3(64), 0, s, word, target, timeout_us, abort, err);
}

void launch_set_word(unsigned *word, unsigned value, hipStream_t s, unsigned *word2, unsigned value2)
{
    hipLaunchKernelGGL(set_word_kernel, dim3(1), dim3(64), 0, s, word, value, word2, value2);
}

void launch_t1_rate_fixup(const T1Args &a, hipStream_t s)
{
    const int n = a.nblks - a.first;
    if (n <= 0) return;
    hipLaunchKernelGGL(t1_rate_fixup_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, a);
}

void launch_t1_model(const T1Args &a, hipStream_t s)
{
    const int n = a.nblks - a.first;
    if (n <= 0) return;
    // want_dist: per-pass distortion sums (needed by rate control only; the no-rate-target mode the
    // reference reaches puts every pass in layer 0 and never looks at them)
    if (a.want_dist) {
        if (a.reversible) hipLaunchKernelGGL((t1_model_kernel<true, true>), dim3((unsigned)n), dim3(64), 0, s, a);
        else hipLaunchKernelGGL((t1_model_kernel<false, true>), dim3((unsigned)n), dim3(64), 0, s, a);
    } else if (a.style & kStyleBypass) {
        if (a.reversible) hipLaunchKernelGGL((t1_model_kernel<true, false, true>), dim3((unsigned)n), dim3(64), 0, s, a);
        else hipLaunchKernelGGL((t1_model_kernel<false, false, true>), dim3((unsigned)n), dim3(64), 0, s, a);
    } else {
        if (a.reversible) hipLaunchKernelGGL((t1_model_kernel<true, false>), dim3((unsigned)n), dim3(64), 0, s, a);
        else hipLaunchKernelGGL((t1_model_kernel<false, false>), dim3((unsigned)n), dim3(64), 0, s, a);
    }
}

void launch_t1_mq_gated(const T1Args &a, int group_first, int group_count, hipStream_t s)
{
    if (group_count <= 0 || !a.gate_groups) return;
    T1Args g = a;
    g.first = group_first; // (gated: `first` is the first workgroup's index into gate_groups / gate_ready)
    if (g.want_rates) hipLaunchKernelGGL(t1_mq2_kernel<true>, dim3((unsigned)group_count), dim3(128), 0, s, g);
    else hipLaunchKernelGGL(t1_mq2_kernel<false>, dim3((unsigned)group_count), dim3(128), 0, s, g);
}

void launch_t1_mq(const T1Args &a, hipStream_t s)
{
    const int n = a.nblks - a.first;
    if (n <= 0) return;
    if (a.style) { launch_t1_mq_styled(a, s); return; } // (a termination at a pass boundary needs interval and code register together)
    // want_rates: per-pass byte counts (rate control, the stage hook on request); a plain frame's consumer keeps none
    if (a.want_rates) hipLaunchKernelGGL(t1_mq2_kernel<true>, dim3((unsigned)((n + 63) / 64)), dim3(128), 0, s, a);
    else hipLaunchKernelGGL(t1_mq2_kernel<false>, dim3((unsigned)((n + 63) / 64)), dim3(128), 0, s, a);
}

} // namespace j2k_hip
