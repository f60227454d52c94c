// cblk_style.h -- the code-block styles of the write side (COD SPcod, T.800 Table A.19) and what follows from a style and a
// pass index alone: which coding passes go out as raw bits and which ones end a codeword segment.  The styled coder kernel
// (t1_mq_styled.hip) and the packet headers (tier2.cpp) both derive a block's segments from these two functions: one rule
// on both sides, no per-pass flags travel.
#pragma once

#include <cstdint>

namespace j2k_hip {

enum : uint32_t {
    kStyleBypass = 1, kStyleReset = 2, kStyleTermall = 4, kStyleVcausal = 8, kStylePterm = 16, kStyleSegsym = 32,
    kStylesEncoded = kStyleBypass | kStyleReset | kStyleTermall | kStylePterm | kStyleSegsym
};

// Pass p of a block (0 = the cleanup pass of its top bit-plane, then significance, refinement, cleanup per plane):
// its kind, 0 significance / 1 refinement / 2 cleanup
constexpr uint32_t cblk_pass_kind(uint32_t p) { return (p + 2u) % 3u; }

// Selective arithmetic-coding bypass (D.6): significance and refinement passes from the fifth bit-plane of the block on
// (pass 10 is the fifth plane's significance pass) are raw bits
constexpr bool cblk_pass_raw(uint32_t style, uint32_t p) { return (style & kStyleBypass) && p >= 10u && cblk_pass_kind(p) != 2u; }

// Does pass p of np end a codeword segment?  The last pass always; every pass under TERMALL; under BYPASS the cleanup pass
// of the fourth plane (pass 9: the last one before the raw passes) and below it every refinement pass (it closes the raw
// pair) and every cleanup pass (an MQ segment of its own).
constexpr bool cblk_pass_terminates(uint32_t style, uint32_t p, uint32_t np)
{
    return p + 1u == np || (style & kStyleTermall) || ((style & kStyleBypass) && (p == 9u || (p >= 10u && cblk_pass_kind(p) != 0u)));
}

} // namespace j2k_hip
