// t1_mq_window.h -- the code register of the MQ coder (T.800 Annex C) as one wide number, so that a group of decisions needs no
// byte-out test between them.  Between two BYTEOUTs the coder holds the pending byte B, 27 - CT live bits of C and the carry
// above them; they are one number
//
//     V = (B << (27 - CT)) + C        of width w = 8 + 27 - CT
//
// in which the carry adds into B by itself.  A decision {addend, shift n} is V = (V + addend) << n, w += n: no test, no select.
// After a group of decisions bytes are peeled off the top: while w - 8 >= 27 the top eight bits are a finished byte; they go
// out, and w drops by 8 -- by 7 behind a 0xFF, whose lowest bit position then stays on top of the next byte as the zero slot
// of Figure C.3.
//
// The wide number differs from Annex C in one situation only: a carry that arrives after a byte was frozen as 0xFF.  Annex C
// parks it in the stuffed bit; here it ripples through: the 0xFF reads 0x00 and the byte above grows by one.  (A finished byte
// takes at most one carry from below, so a rolled byte reads 0x00 and nothing else.)  A group is exact unless
//   carry   V >> w != 0: the pending byte was 0xFF -- from the start, or by a carry of this group -- and took a carry;
//   rolled  a byte that became the pending one during the peel reads 0x00 (conservative: it may be a true zero);
//   wide    w passed 63: V may have lost bits (from an exact state, w <= 34, that takes shifts of more than 29 in the group).
// A group that reports one of them is run again from its starting state by the per-decision coder; the states convert both ways.
// The group form further down is what the kernel runs: the group summed into one number by the side that knows the decisions,
// `wide` replaced by `long`, and `rolled` by the exact test, which does not report a true zero.
//
// No LDS and no lane logic here: the consumer of t1_mq2_kernel (t1.hip) and a host program (tests/native/t1_mq_window_host.cpp)
// run this text.
#pragma once

#if defined(__HIPCC__)
#define J2K_WIN_HD __host__ __device__ __forceinline__
#else
#define J2K_WIN_HD inline
#endif

namespace j2k_hip {

struct MqWide {
    unsigned long long V;
    unsigned w;
};

constexpr unsigned kMqWideDue = 8u + 27u;  // from this width on the top byte is finished
constexpr unsigned kMqWideMax = 63u;       // widest state whose V is whole and whose carry bit V >> w can be read

// (C, CT, B) of an exact state, 1 <= CT <= 12, C below 2^(28 - CT): a carry still in C lands in B, where BYTEOUT would put
// it -- or above a B of 0xFF, where only this form shows it.
J2K_WIN_HD MqWide mq_wide_from(unsigned C, unsigned CT, unsigned B)
{
    MqWide s;
    s.V = ((unsigned long long)B << (27u - CT)) + C;
    s.w = kMqWideDue - CT;
    return s;
}
// ... and back, 23 <= w <= 34.  A carry above the pending byte can only stand above a 0xFF: it returns to C, where Annex C keeps it.
J2K_WIN_HD void mq_wide_to(const MqWide &s, unsigned &C, unsigned &CT, unsigned &B)
{
    const unsigned k = s.w - 8u;
    const unsigned top = (unsigned)(s.V >> k), over = top >> 8;
    CT = kMqWideDue - s.w;
    B = top - over; // 0x100 -> 0xFF
    C = ((unsigned)s.V & ((1u << k) - 1u)) | (over << k);
}

// one decision as the producer queues it: addend in the low half, shift above
J2K_WIN_HD void mq_wide_add(MqWide &s, unsigned e)
{
    const unsigned n = e >> 16;
    s.V = (s.V + (e & 0xffffu)) << n;
    s.w += n;
}

// after the group's decisions, before any byte is peeled
J2K_WIN_HD bool mq_wide_is_wide(const MqWide &s) { return s.w > kMqWideMax; }
J2K_WIN_HD bool mq_wide_has_carry(const MqWide &s) { return (s.V >> (s.w & 63u)) != 0; } // (meaningful while !mq_wide_is_wide)

J2K_WIN_HD bool mq_wide_due(const MqWide &s) { return s.w >= kMqWideDue; }
// One peel round, in select form: every lane gets its top byte back -- the byte to store at the lane's next position; a lane
// that is not due stores its pending byte there, where its next finished byte overwrites it -- and the lanes in `p` (those due)
// drop it and report in `rolled` whether the byte that is pending now reads 0x00.
J2K_WIN_HD unsigned mq_wide_peel(MqWide &s, bool p, bool &rolled)
{
    const unsigned k = s.w - 8u;
    const unsigned byte = (unsigned)(s.V >> k);
    const unsigned long long rest = s.V - ((unsigned long long)byte << k);
    const unsigned w1 = s.w - (byte == 0xffu ? 7u : 8u);
    const bool zero = (rest >> (w1 - 8u)) == 0;
    s.V = p ? rest : s.V;
    s.w = p ? w1 : s.w;
    rolled = rolled || (p && zero);
    return byte;
}

// ---- The group form.  Four decisions act on V as one number: with N = n0 + n1 + n2 + n3
//
//     V' = (V << N) + G,      G = ((((a0 << n0) + a1) << n1) + a2) << n2 ... << n3
//
// and the side that knows the decisions (the producer wave) forms G by one (G + a) << n per decision in 32 bits.  An addend is
// 0 or a Qe of Table C.2, at most 0x5601, so G <= 4 * 0x5601 << N, which 32 bits hold while N <= 15.  A group with a larger N is
//   long    its G is not to be used: the group is coded again from its addends and shifts, which travel beside G.
// From an exact state (w <= 34) a group that is not long ends at w <= 49: `wide` cannot occur on this path.
constexpr unsigned kMqAddendMax = 0x5601u; // the largest Qe of Table C.2
constexpr unsigned kMqGroupMaxN = 15u;
constexpr unsigned kMqExactMax = kMqWideDue - 1u; // the widest exact state: CT = 1
static_assert(((4ull * kMqAddendMax) << kMqGroupMaxN) < (1ull << 32), "G of a group that is not long must fit 32 bits");
static_assert(((4ull * kMqAddendMax) << (kMqGroupMaxN + 1u)) >= (1ull << 32), "(and one shift more does not: the bound is tight)");
static_assert(kMqExactMax + kMqGroupMaxN <= kMqWideMax, "a group that is not long cannot be wide");

J2K_WIN_HD void mq_group_add(unsigned &G, unsigned &N, unsigned addend, unsigned n)
{
    G = (G + addend) << n;
    N += n;
}
J2K_WIN_HD bool mq_group_is_long(unsigned N) { return N > kMqGroupMaxN; }
// (a long group's V is garbage -- N < 64 all the same: four shifts of at most 15 -- and is never read)
J2K_WIN_HD void mq_wide_add_group(MqWide &s, unsigned G, unsigned N)
{
    s.V = (s.V << N) + G;
    s.w += N;
}

// The queue words of a group: {G, shifts} is what the common path reads, {a01, a23} what a group that is coded again reads too.
//   shifts   n0 | n1 << 4 | n2 << 8 | n3 << 12 | N << 16         a01, a23   the addends as 16-bit halves, the earlier one below
// Decisions past a lane's end are zeros in every field.
J2K_WIN_HD unsigned mq_group_pack_shifts(unsigned n0, unsigned n1, unsigned n2, unsigned n3, unsigned N)
{
    return n0 | (n1 << 4) | (n2 << 8) | (n3 << 12) | (N << 16);
}
// (the same word built decision by decision: shift n of decision jj goes into its nibble and into the sum in one multiply-add,
//  n * (1 << 4 * jj | 1 << 16); the nibbles stay below bit 16 and N <= 60, so nothing meets)
J2K_WIN_HD unsigned mq_group_add_shift(unsigned shifts, unsigned n, unsigned jj)
{
    const unsigned k = (1u << (4u * jj)) | 0x10000u;
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(n, k) + shifts;
#else
    return n * k + shifts;
#endif
}
J2K_WIN_HD unsigned mq_group_pack_addends(unsigned first, unsigned second) { return first | (second << 16); }
// (the same word from addends that sit in the high halves of their words, as the producer wave holds them: one byte permute)
J2K_WIN_HD unsigned mq_group_pack_addends_high(unsigned first, unsigned second)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(second, first, 0x07060302u);
#else
    return (first >> 16) | (second & 0xffff0000u);
#endif
}
J2K_WIN_HD unsigned mq_group_N(unsigned shifts) { return shifts >> 16; }
// decision jj of the group as {addend | n << 16}, the form mq_wide_add and the per-decision coder take
J2K_WIN_HD unsigned mq_group_decision(unsigned shifts, unsigned a01, unsigned a23, unsigned jj)
{
    const unsigned pair = jj < 2u ? a01 : a23;
    const unsigned addend = (jj & 1u) ? pair >> 16 : pair & 0xffffu;
    return addend | (((shifts >> (4u * jj)) & 15u) << 16);
}

// The peel round of mq_wide_peel that records instead of reporting: where a byte that became the pending one reads 0x00, the
// lane keeps the bit position of that byte's top boundary (positions in V do not move while bytes are peeled off the top).
// The boundary is the lowest bit of the byte just peeled, k -- also behind a 0xFF, where the new byte's window begins one bit
// higher, on the zero slot: a carry that made a 0xFE above into that 0xFF changed bit k and nothing above it.
// Later rounds are lower, and the lowest is the most conservative one: it is the one kept.
constexpr unsigned kMqNoZero = 63u; // no such byte: above every bit of a V that is not wide, the test below reads nothing there
J2K_WIN_HD unsigned mq_wide_peel_mark(MqWide &s, bool p, unsigned &zpos)
{
    const unsigned k = s.w - 8u;
    const unsigned byte = (unsigned)(s.V >> k);
    const unsigned long long rest = s.V - ((unsigned long long)byte << k);
    const unsigned w1 = s.w - (byte == 0xffu ? 7u : 8u);
    const bool zero = (rest >> (w1 - 8u)) == 0;
    s.V = p ? rest : s.V;
    s.w = p ? w1 : s.w;
    zpos = (p && zero) ? k : zpos;
    return byte;
}
// The exact form of `rolled`.  A byte that reads 0x00 has rolled over only if a carry left its top boundary, bit zpos, during the
// group.  The group's partial sums, all taken at the final scale, only grow from V_start << N to V_after, so floor(. / 2^zpos)
// never falls: if the bits from zpos up are the same in both, no carry crossed, and the byte is a true zero.  Taken on the
// value before any byte is peeled.  (Still conservative: a carry that crossed before the byte was finished is reported too.)
J2K_WIN_HD bool mq_group_rolled(unsigned long long V_after, unsigned long long V_start, unsigned N, unsigned zpos)
{
    return zpos != kMqNoZero && ((V_after ^ (V_start << N)) >> zpos) != 0;
}

} // namespace j2k_hip
