// t1_mq_styled.hip -- the coder of code-blocks under a code-block style (bypass, reset, termall, pterm, segsym; T.800 D.4 - D.7).
//
//  t1_mq_styled_kernel  one LANE per code-block, 64 blocks per wave, blocks are the parallel axis as in t1_mq2_kernel -- but the
//            interval register and the code register run in the SAME lane: a termination at a pass boundary (FLUSH, the
//            predictable form, the padding of a raw segment) needs both, and the two-wave coder's producer never sees the
//            code register.  The recurrence itself is t1_mq_styled.h (StyledCoder), shared with the host; this file gives it
//            its tables (LDS), its context states (LDS, a column per lane) and its byte sink: a per-lane LDS stage from
//            which the codeword leaves in 16-byte vector stores.  Pass ends and pass kinds come from pass_nsym and the pass
//            index; which passes are raw and which terminate follows from the style (cblk_style.h), on the host as here.
//            pass_rate receives libopenjp2's byte count per pass; t1_rate_fixup_kernel runs behind it.
#include "kernels.h"
#include "t1_common.h"
#include "t1_mq_styled.h"

namespace j2k_hip {
namespace {

// Staged codeword bytes per lane: a pad word (read as "the byte before the first", never part of the codeword), then kStage
// bytes.  A lane's stage is drained when 64 bytes wait, down to 16..31 (a termination looks at and takes back up to two
// bytes behind the end: they must still be there); between two drains lie at most 16 decisions (3 bytes each at most)
// and one pass end (four segmentation symbols and a termination: under 20 bytes), so under 64 + 48 + 20 = 132 bytes ever
// wait.  Stride 41 words: odd, so the lanes' byte stores spread over the banks.
constexpr unsigned kStage = 160, kStride = kStage + 4;

struct LdsTab {
    const unsigned *mps, *lps;
    __device__ __forceinline__ unsigned mps_entry(unsigned st) const { return mps[st]; }
    __device__ __forceinline__ unsigned lps_next(unsigned st) const { return lps[st]; }
};
struct LdsCtx {
    unsigned *col; // the lane's column: context c at col[c * 64]
    __device__ __forceinline__ unsigned get(unsigned c) const { return col[c * 64]; }
    __device__ __forceinline__ void set(unsigned c, unsigned st) { col[c * 64] = st; }
};
struct LdsSink {
    unsigned char *stage; // the lane's first data byte
    unsigned pos = 0;     // bytes staged
    unsigned flushed = 0; // bytes of the codeword already in HBM (a multiple of 16)
    // (the clamp never acts while the bound above holds; if it ever did not, the bytes would stay inside the lane's stage and
    //  the drain reports the block as overflowed)
    __device__ __forceinline__ void put(unsigned b) { stage[min(pos, kStage - 1u)] = (unsigned char)b; ++pos; }
    __device__ __forceinline__ void drop(unsigned n) { pos -= n; }
    __device__ __forceinline__ unsigned peek(unsigned k) const { return stage[(int)pos - 1 - (int)k]; } // (before the first byte: the pad word, zero)
    __device__ __forceinline__ unsigned size() const { return flushed + pos; }
};

__global__ __launch_bounds__(64) void t1_mq_styled_kernel(T1Args a)
{
    __shared__ unsigned ctxs[19 * 64];
    __shared__ unsigned tab_mps[94], tab_lps[94]; // [Table C.2 index << 1 | MPS]
    __shared__ __attribute__((aligned(16))) unsigned ostage[kStride / 4 * 64];
    const int lane = threadIdx.x;
    if (a.mq_prio >= 3) __builtin_amdgcn_s_setprio(3);
    else if (a.mq_prio == 2) __builtin_amdgcn_s_setprio(2);
    else if (a.mq_prio == 1) __builtin_amdgcn_s_setprio(1);
    if (lane < 47)
        for (unsigned mps = 0; mps < 2; ++mps) {
            tab_mps[lane * 2 + mps] = ((unsigned)kQe[lane] << 16) | ((unsigned)kNmps[lane] << 1) | mps;
            tab_lps[lane * 2 + mps] = ((unsigned)kNlps[lane] << 1) | (mps ^ kSwitch[lane]);
        }
    for (int i = lane; i < (int)(kStride / 4 * 64); i += 64) ostage[i] = 0;
    const int b = a.first + (int)blockIdx.x * 64 + lane;
    const bool live = b < a.nblks;
    CblkDev cb = {};
    unsigned nsym = 0, npasses = 0;
    if (live) { cb = a.blks[b]; nsym = a.nsym[b]; npasses = a.npasses[b]; }
    unsigned maxsym = nsym;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) maxsym = max(maxsym, (unsigned)__shfl_xor((int)maxsym, o));
    const unsigned nchunks = (unsigned)__builtin_amdgcn_readfirstlane((int)((maxsym + 15) / 16)); // wave-uniform loop bound
    __syncthreads();

    LdsTab tab{tab_mps, tab_lps};
    LdsCtx ctx{ctxs + lane};
    LdsSink sink{reinterpret_cast<unsigned char *>(ostage) + (unsigned)lane * kStride + 4u};
    StyledCoder<LdsTab, LdsCtx, LdsSink> coder(tab, ctx, sink, a.style);
    coder.begin_block();

    const unsigned char *sym = a.sym + cb.sym_off;
    unsigned char *out = a.out + cb.out_off;
    const unsigned *pass_nsym = a.pass_nsym + (size_t)(live ? b : 0) * kDevMaxPasses;
    unsigned *pass_rate = a.pass_rate + (size_t)(live ? b : 0) * kDevMaxPasses;
    bool overflow = false;
    // whole 16-byte units leave the lane's stage once 64 bytes wait; 16..31 bytes stay and move to the front
    auto drain = [&]() {
        if (sink.pos < 64u) return;
        if (sink.pos > kStage) { overflow = true; sink.pos = kStage; }
        const unsigned units = (sink.pos >> 4) - 1u;
        for (unsigned u = 0; u < units; ++u) {
            if (sink.flushed + 16u <= cb.out_cap) {
                const unsigned *sp = reinterpret_cast<const unsigned *>(sink.stage + 16u * u);
                *reinterpret_cast<uint4 *>(out + sink.flushed) = make_uint4(sp[0], sp[1], sp[2], sp[3]);
            } else overflow = true;
            sink.flushed += 16u;
        }
        const unsigned rest = sink.pos - 16u * units; // 16 .. 31
        const unsigned *sp = reinterpret_cast<const unsigned *>(sink.stage + 16u * units);
        unsigned *dp = reinterpret_cast<unsigned *>(sink.stage);
        for (unsigned k = 0; 4u * k < rest; ++k) dp[k] = sp[k]; // (forwards: the source lies at least 48 bytes further on)
        sink.pos = rest;
    };
    unsigned cur_pass = 0;
    unsigned next_end = npasses ? pass_nsym[0] : 0xffffffffu;
    // the passes that end in front of decision i (an empty pass ends where the one before it did)
    auto close_passes = [&](unsigned i) {
        while (cur_pass < npasses && i == next_end) {
            pass_rate[cur_pass] = coder.end_pass(cur_pass, npasses);
            ++cur_pass;
            next_end = cur_pass < npasses ? pass_nsym[cur_pass] : 0xffffffffu;
            drain();
        }
    };
    unsigned yield_budget = 2048; // polls of ~2 us: every wave moves on whatever the word says
    for (unsigned c = 0; c < nchunks; ++c) {
        // while another frame's DWT launches are running (yield_word != 0) the coder waves step aside, as the two-wave coder's do
        if (a.yield_word && (c & 3u) == 0) {
            while (yield_budget && __builtin_amdgcn_readfirstlane((int)__hip_atomic_load(a.yield_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
                __builtin_amdgcn_s_sleep(64);
                --yield_budget;
            }
        }
        const unsigned base = c * 16;
        if (base < nsym) { // (the stream's capacity is a multiple of 1 KiB: the 16 bytes are the block's own)
            const uint4 chunk = *reinterpret_cast<const uint4 *>(sym + base);
            const unsigned rem = min(nsym - base, 16u);
#pragma unroll 1
            for (unsigned g = 0; 4u * g < rem; ++g) {
                unsigned w = g == 0 ? chunk.x : (g == 1 ? chunk.y : (g == 2 ? chunk.z : chunk.w));
                const unsigned n4 = min(rem - 4u * g, 4u);
#pragma unroll 1
                for (unsigned j = 0; j < n4; ++j, w >>= 8) {
                    const unsigned i = base + 4u * g + j;
                    if (i == next_end) close_passes(i);
                    coder.decision(w & 0xffu);
                }
            }
            drain();
        }
    }
    const bool fin = live && npasses;
    if (fin) {
        close_passes(nsym); // the passes that end with the stream, the last one among them: it terminates
        const unsigned nb = sink.size();
        for (unsigned o = sink.flushed; o < nb; o += 4) {
            if (o + 4u <= cb.out_cap) *reinterpret_cast<unsigned *>(out + o) = *reinterpret_cast<const unsigned *>(sink.stage + (o - sink.flushed));
            else overflow = true;
        }
        a.len[b] = nb;
        if (overflow) a.err[0] = 3u;
    } else if (live) a.len[b] = 0;
}

} // namespace

void launch_t1_mq_styled(const T1Args &a, hipStream_t s)
{
    const int n = a.nblks - a.first;
    if (n <= 0) return;
    hipLaunchKernelGGL(t1_mq_styled_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, a);
}

} // namespace j2k_hip
