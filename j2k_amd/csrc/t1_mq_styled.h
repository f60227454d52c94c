// t1_mq_styled.h -- the coder of a code-block under a code-block style (T.800 D.4 - D.7, Annex C): MQ segments with restarts,
// plain and predictable termination, raw segments of the selective bypass, context resets and segmentation symbols -- one
// block's whole recurrence (interval, code register, byte output) in one place, written against three small interfaces so
// that the kernel (t1_mq_styled.hip: a lane per block, bytes staged in LDS) and a host program run the very same text:
//
//   Tab   unsigned mps_entry(state)   Qe << 16 | the state after a more probable symbol   (state = Table C.2 index << 1 | MPS)
//         unsigned lps_next(state)    the state after a less probable symbol (SWITCH folded in)
//   Ctx   unsigned get(c), void set(c, state)   the 19 context states of the block
//   Sink  void put(byte), void drop(n), unsigned peek(k), unsigned size()
//         the block's codeword so far: append, take the last n bytes back, read the byte k before the end, count
//
// The byte counts it reports per pass are libopenjp2's (opj_t1_encode_cblk): the exact length at a terminated pass, an
// estimate at any other; the fix-ups of t1_rate_fixup_kernel then apply as they do for rate control.
#pragma once

#include "cblk_style.h"

#if defined(__HIPCC__)
#define J2K_HD __host__ __device__ __forceinline__
#else
#define J2K_HD inline
#endif

namespace j2k_hip {

constexpr unsigned kCtxUni = 18, kCtxRl = 17;
// initial states (D.7): UNI 46, run-length 3, context 0 -> 4, every other one 0; MPS 0
constexpr unsigned cblk_ctx_initial(unsigned c) { return (c == kCtxUni ? 46u : (c == kCtxRl ? 3u : (c == 0u ? 4u : 0u))) << 1; }

template <class Tab, class Ctx, class Sink>
struct StyledCoder {
    Tab &tab;
    Ctx &ctx;
    Sink &out;
    unsigned style;
    // MQ: interval A, code register C, counter CT, the byte B that a carry may still reach (have_b: there is one -- not before
    // the first byte of the block, not while a segment is closed).  Raw: C collects the bits of the open byte, CT counts its free ones.
    unsigned A = 0x8000u, C = 0, CT = 12, B = 0;
    bool have_b = false, raw = false;
    static constexpr unsigned kRawIdle = 99; // raw segment without a bit yet (no 0xFF 0x7F trimming then)

    J2K_HD StyledCoder(Tab &t, Ctx &c, Sink &o, unsigned s) : tab(t), ctx(c), out(o), style(s) {}

    J2K_HD void reset_contexts() { for (unsigned c = 0; c < 19; ++c) ctx.set(c, cblk_ctx_initial(c)); }

    J2K_HD void emit_b() { if (have_b) out.put(B); have_b = true; }
    // BYTEOUT (Figure C.3)
    J2K_HD void byteout()
    {
        if (B == 0xffu) { emit_b(); B = (C >> 20) & 0xffu; C &= 0xfffffu; CT = 7; return; }
        if (C & 0x8000000u) {
            ++B;
            if (B == 0xffu) { C &= 0x7ffffffu; emit_b(); B = (C >> 20) & 0xffu; C &= 0xfffffu; CT = 7; return; }
        }
        emit_b(); B = (C >> 19) & 0xffu; C &= 0x7ffffu; CT = 8;
    }
    // ENCODE (Figures C.4 - C.8) of bit d in context c
    J2K_HD void encode(unsigned c, unsigned d)
    {
        const unsigned st = ctx.get(c), e = tab.mps_entry(st), qe = e >> 16;
        A -= qe;
        if (d == (st & 1u)) {
            if (A & 0x8000u) { C += qe; return; }
            if (A < qe) A = qe; else C += qe;
            ctx.set(c, e & 0xffffu);
        } else {
            if (A < qe) C += qe; else A = qe;
            ctx.set(c, tab.lps_next(st));
        }
        unsigned n = (unsigned)__builtin_clz(A) - 16u; // renormalisation shift: A < 0x8000 here
        A <<= n;
        while (n >= CT) { C <<= CT; n -= CT; byteout(); }
        C <<= n; CT -= n;
    }
    // bytes of the block so far as libopenjp2 counts them while an MQ segment is open (the pending byte is not in)
    J2K_HD int mq_bytes() const { return (int)out.size() - (have_b ? 0 : 1); }

    // FLUSH (C.2.9): set bits, two byte-outs, a trailing 0xFF is dropped
    J2K_HD void flush()
    {
        const unsigned tempc = C + A;
        C |= 0xffffu;
        if (C >= tempc) C -= 0x8000u;
        C <<= CT; byteout();
        C <<= CT; byteout();
        if (B != 0xffu) out.put(B);
        have_b = false;
    }
    // predictable termination (D.4.2)
    J2K_HD void erterm()
    {
        int k = 12 - (int)CT;
        while (k > 0) { C <<= CT; CT = 0; byteout(); k -= (int)CT; }
        if (B != 0xffu) emit_b();
        have_b = false;
    }
    // the next MQ segment: INITENC with the segment's last byte as the byte before
    J2K_HD void restart()
    {
        A = 0x8000u; C = 0; CT = 12;
        B = out.peek(0); out.drop(1); have_b = true;
        if (B == 0xffu) CT = 13;
        raw = false;
    }
    J2K_HD void raw_init() { C = 0; CT = kRawIdle; have_b = false; raw = true; }
    J2K_HD void raw_bit(unsigned d)
    {
        if (CT == kRawIdle) CT = 8;
        --CT;
        C += d << CT;
        if (CT == 0) { out.put(C); CT = C == 0xffu ? 7 : 8; C = 0; } // after a 0xFF the next byte takes seven bits
    }
    J2K_HD bool raw_open_byte(bool pterm) const { return CT < 7 || (CT == 7 && (pterm || out.peek(0) != 0xffu)); }
    J2K_HD void raw_flush(bool pterm)
    {
        if (raw_open_byte(pterm)) { // the open byte goes out padded with 0, 1, 0, 1 ...
            unsigned bit = 0;
            while (CT > 0) { --CT; C += bit << CT; bit ^= 1u; }
            out.put(C);
        } else if (CT == 7 && out.peek(0) == 0xffu) out.drop(1);                                   // a trailing 0xFF
        else if (CT == 8 && !pterm && out.peek(0) == 0x7fu && out.peek(1) == 0xffu) out.drop(2);     // 0xFF 0x7F: the decoder reads ones past the end anyway
    }

    J2K_HD void begin_block() { A = 0x8000u; C = 0; CT = 12; B = 0; have_b = false; raw = false; reset_contexts(); }
    J2K_HD void decision(unsigned byte) // (context << 1) | bit as the modeller writes it
    {
        if (raw) raw_bit(byte & 1u); else encode(byte >> 1, byte & 1u);
    }
    // Pass p of np is through: segmentation symbol, termination, byte count, context reset, and the next segment opened.
    J2K_HD unsigned end_pass(unsigned p, unsigned np)
    {
        if ((style & kStyleSegsym) && cblk_pass_kind(p) == 2u) { encode(kCtxUni, 1); encode(kCtxUni, 0); encode(kCtxUni, 1); encode(kCtxUni, 0); }
        const bool pterm = (style & kStylePterm) != 0;
        unsigned rate;
        if (cblk_pass_terminates(style, p, np)) {
            if (raw) raw_flush(pterm); else if (pterm) erterm(); else flush();
            rate = out.size();
            if (p + 1u < np) { if (cblk_pass_raw(style, p + 1u)) raw_init(); else restart(); }
        } else rate = raw ? out.size() + (raw_open_byte(pterm) ? 1u : 0u) : (unsigned)(mq_bytes() + 3);
        if (style & kStyleReset) reset_contexts();
        return rate;
    }
};

} // namespace j2k_hip
