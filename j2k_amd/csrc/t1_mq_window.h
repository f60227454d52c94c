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

} // namespace j2k_hip
