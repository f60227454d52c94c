// t1_mq_window_host.cpp -- the host program of t1_mq_window.h: the MQ coder's code register as one wide number, accumulated
// over groups of four decisions and peeled byte by byte, held to a plain transcription of T.800 Figure C.3 (bit-by-bit
// RENORME, BYTEOUT as drawn).  tests/test_t1_mq_window_host.py builds this with the address and undefined-behaviour
// sanitizers and reads its report.
//
//   t1_mq_window_host [streams [decisions [seed]]]          (defaults 2000, 4000, 1)
//
// Generated streams: an interval register A driven through ENCODE (Figures C.4 - C.8), which yields per decision what the
// producer wave of t1_mq2_kernel queues: {addend, shift}.  Even streams use the state of Qe = 0x5601 alone with fair bits,
// odd ones walk Table C.2 in eight contexts whose bits are skewed differently.  Crafted groups start from a given (C, CT, B)
// and force each report of the header: a pending 0xFF that takes a late carry, a finished 0xFF that rolls over, four shifts
// of 15, a true 0x00 byte, the block's first byte.  A group that reports is run again from its starting state by a word-wise
// per-decision coder (the form of the kernel's `four`), through both state conversions; the option of the kernel's knob
// mq_window = 2 -- every group that way -- is run as well.
//
// Every stream must give the reference's bytes and its final state, every crafted group the report it is named for, and the
// generated streams may send at most 1 % of their groups back (printed as "rerun share").  Exit status 0 / 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "t1_mq_window.h"

namespace {

using j2k_hip::MqWide;

const uint16_t kQeTab[47] = {0x5601, 0x3401, 0x1801, 0x0AC1, 0x0521, 0x0221, 0x5601, 0x5401, 0x4801, 0x3801, 0x3001, 0x2401,
                             0x1C01, 0x1601, 0x5601, 0x5401, 0x5101, 0x4801, 0x3801, 0x3401, 0x3001, 0x2801, 0x2401, 0x2201,
                             0x1C01, 0x1801, 0x1601, 0x1401, 0x1201, 0x1101, 0x0AC1, 0x09C1, 0x08A1, 0x0521, 0x0441, 0x02A1,
                             0x0221, 0x0141, 0x0111, 0x0085, 0x0049, 0x0025, 0x0015, 0x0009, 0x0005, 0x0001, 0x5601};
const uint8_t kNmpsTab[47] = {1, 2, 3, 4, 5, 38, 7, 8, 9, 10, 11, 12, 13, 29, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24,
                              25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 45, 46};
const uint8_t kNlpsTab[47] = {1, 6, 9, 12, 29, 33, 6, 14, 14, 14, 17, 18, 20, 21, 14, 14, 15, 16, 17, 18, 19, 19, 20, 21,
                              22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 46};

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x1234567ull) {}
    uint32_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 16); }
    double unit() { return (next() & 0xffffffu) / 16777216.0; }
};

struct State { unsigned C, CT, B; };
constexpr State kInit = {0, 12, 0};

// ---- the reference: Figure C.3 and the shift loop of RENORME, one bit at a time.  Every BYTEOUT appends B -- the first one
// the pad byte before the codeword, as the kernel's stage has it.
struct Plain {
    unsigned C, CT, B;
    std::vector<uint8_t> out;
    explicit Plain(State s) : C(s.C), CT(s.CT), B(s.B) {}
    void byteout()
    {
        if (B == 0xffu) { out.push_back((uint8_t)B); B = C >> 20; C &= 0xfffffu; CT = 7; return; }
        if (C >= 0x8000000u) {
            ++B;
            if (B == 0xffu) { C &= 0x7ffffffu; out.push_back((uint8_t)B); B = C >> 20; C &= 0xfffffu; CT = 7; return; }
            C &= 0x7ffffffu;
        }
        out.push_back((uint8_t)B); B = C >> 19; C &= 0x7ffffu; CT = 8;
    }
    void decision(unsigned e)
    {
        C += e & 0xffffu;
        for (unsigned n = e >> 16; n; --n) { C <<= 1; if (--CT == 0) byteout(); }
    }
};

// ---- the per-decision coder a reported group falls back to: word-wise shifts, BYTEOUT with the carry left in place
struct Words {
    unsigned C, CT, B;
    std::vector<uint8_t> *out;
    void byteout()
    {
        const bool was_ff = B == 0xffu;
        const unsigned Bc = B + ((C > 0x7ffffffu && !was_ff) ? 1u : 0u);
        const unsigned sh = Bc == 0xffu ? 20u : 19u;
        out->push_back((uint8_t)Bc);
        B = (C >> sh) & (was_ff ? 0xffu : (1u << (27u - sh)) - 1u);
        C &= (1u << sh) - 1u;
        CT = 27u - sh;
    }
    void decision(unsigned e)
    {
        C += e & 0xffffu;
        unsigned n = e >> 16;
        while (n >= CT) { C <<= CT; n -= CT; byteout(); }
        C <<= n; CT -= n;
    }
};

enum { kCarry = 1, kRolled = 2, kWide = 4 };

// ---- the coder under test: groups of four through the header.  `always`: every group takes the fallback.
struct Windowed {
    MqWide s;
    std::vector<uint8_t> out;
    unsigned long long groups = 0, reruns = 0, peeled = 0;
    explicit Windowed(State st) : s(j2k_hip::mq_wide_from(st.C, st.CT, st.B)) {}
    int group(const unsigned (&e)[4], bool always)
    {
        const MqWide s0 = s;
        const size_t n0 = out.size();
        for (unsigned e1 : e) j2k_hip::mq_wide_add(s, e1);
        int report = 0;
        if (j2k_hip::mq_wide_is_wide(s)) report |= kWide;
        else if (j2k_hip::mq_wide_has_carry(s)) report |= kCarry;
        if (!report) {
            bool rolled = false;
            while (j2k_hip::mq_wide_due(s)) { out.push_back((uint8_t)j2k_hip::mq_wide_peel(s, true, rolled)); ++peeled; }
            if (rolled) report |= kRolled;
        }
        ++groups;
        if (report) ++reruns;
        if (report || always) {
            out.resize(n0);
            Words w{0, 0, 0, &out};
            j2k_hip::mq_wide_to(s0, w.C, w.CT, w.B);
            for (unsigned e1 : e) w.decision(e1);
            s = j2k_hip::mq_wide_from(w.C, w.CT, w.B);
        }
        return report;
    }
};

// ---- decisions
struct Interval {
    unsigned A = 0x8000u;
    unsigned encode(unsigned qe, bool mps) // {addend | shift << 16}
    {
        unsigned add = 0;
        A -= qe;
        if (mps) {
            if (A & 0x8000u) return qe;
            if (A < qe) A = qe; else add = qe;
        } else {
            if (A < qe) add = qe; else A = qe;
        }
        unsigned n = 0;
        while (!(A & 0x8000u)) { A <<= 1; ++n; }
        return add | (n << 16);
    }
};

std::vector<unsigned> generate(Rng &rng, size_t count, bool mixed)
{
    std::vector<unsigned> e(count);
    Interval iv;
    unsigned idx[8] = {0, 0, 0, 0, 3, 4, 46, 0};
    double p_lps[8];
    for (double &p : p_lps) p = mixed ? 0.002 + 0.45 * rng.unit() * rng.unit() : 0.5;
    for (size_t i = 0; i < count; ++i) {
        if (!mixed) { e[i] = iv.encode(0x5601u, (rng.next() & 1u) != 0); continue; }
        const unsigned c = rng.next() & 7u;
        const bool mps = rng.unit() >= p_lps[c];
        const unsigned qe = kQeTab[idx[c]];
        const unsigned a_before = iv.A;
        e[i] = iv.encode(qe, mps);
        const bool renorm = !(mps && ((a_before - qe) & 0x8000u));
        if (renorm) idx[c] = mps ? kNmpsTab[idx[c]] : kNlpsTab[idx[c]];
    }
    return e;
}

int g_failed = 0;

// One stream from `start` through the reference and the windowed coder; the report of the first group goes to *first.
bool run_stream(const char *name, long id, State start, const std::vector<unsigned> &dec, bool always, Windowed *stats, int *first)
{
    Plain ref(start);
    for (unsigned e : dec) ref.decision(e);
    Windowed win(start);
    for (size_t i = 0; i < dec.size(); i += 4) {
        unsigned e[4] = {0, 0, 0, 0}; // (past the end: decisions that change nothing, as the producer queues them)
        for (size_t j = 0; j < 4 && i + j < dec.size(); ++j) e[j] = dec[i + j];
        const int report = win.group(e, always);
        if (i == 0 && first) *first = report;
    }
    if (stats) { stats->groups += win.groups; stats->reruns += win.reruns; stats->peeled += win.peeled; }
    bool ok = true;
    if (win.out.size() != ref.out.size()) { std::printf("%s %ld: %zu bytes, the reference has %zu\n", name, id, win.out.size(), ref.out.size()); ok = false; }
    for (size_t i = 0; ok && i < ref.out.size(); ++i)
        if (win.out[i] != ref.out[i]) { std::printf("%s %ld: byte %zu is %02x, the reference has %02x\n", name, id, i, win.out[i], ref.out[i]); ok = false; }
    const MqWide want = j2k_hip::mq_wide_from(ref.C, ref.CT, ref.B);
    if (ok && (win.s.V != want.V || win.s.w != want.w)) {
        std::printf("%s %ld: final state (%llx, %u), the reference has (%llx, %u)\n", name, id, win.s.V, win.s.w, want.V, want.w);
        ok = false;
    }
    if (!ok) ++g_failed;
    return ok;
}

struct Crafted { const char *name; State start; unsigned e[4]; int report; };
constexpr unsigned dec(unsigned addend, unsigned n) { return addend | (n << 16); }
const Crafted kCrafted[] = {
    // B = 0xFF pending behind 20 set bits of C; the last decision's addend carries out of them: Annex C parks the carry in the
    // next byte's top bit, the wide number would make the byte 0x100
    {"pending 0xFF, late carry", {0xfffffu, 7, 0xff}, {dec(0, 0), dec(0, 0), dec(0, 0), dec(1, 0)}, kCarry},
    // a pending 0xFE that a carry of this group makes 0xFF before it goes out: no report, and the byte behind it takes seven bits
    {"pending 0xFE becomes 0xFF", {0x7ffffu, 8, 0xfe}, {dec(1, 1), dec(0x5601, 7), dec(0, 0), dec(0, 0)}, 0},
    // eight shifts finish a byte of 0xFF, then a carry reaches it: 0xFF -> 0x00, the byte above 0x12 -> 0x13
    {"finished 0xFF rolls", {0x7ffffu, 8, 0x12}, {dec(0, 8), dec(0x100, 0), dec(0, 0), dec(0, 0)}, kRolled},
    // four shifts of 15 from the widest exact state
    {"four shifts of 15", {0x155u, 1, 0x34}, {dec(0x5601, 15), dec(0x0001, 15), dec(0x2201, 15), dec(0x0005, 15)}, kWide},
    {"four shifts of 15, narrow start", {0, 12, 0}, {dec(0x5601, 15), dec(0x0001, 15), dec(0x2201, 15), dec(0x0005, 15)}, kWide},
    // a byte that is zero by itself: reported (the test cannot tell it from a rolled one), and coded the same either way
    {"true 0x00 byte", {0x00055u, 8, 0x12}, {dec(0, 8), dec(0x55, 0), dec(0, 0), dec(0, 0)}, kRolled},
    // the block's first byte: CT = 12, the pad byte goes out, the byte behind it is not zero
    {"first byte", {0, 12, 0}, {dec(0x1601, 1), dec(0x0AC1, 2), dec(0x0521, 4), dec(0x0221, 6)}, 0},
    {"first byte, not yet out", {0, 12, 0}, {dec(0x1601, 1), dec(0x0AC1, 2), dec(0, 0), dec(0, 0)}, 0},
};

} // namespace

int main(int argc, char **argv)
{
    const long streams = argc > 1 ? std::atol(argv[1]) : 2000;
    const long count = argc > 2 ? std::atol(argv[2]) : 4000;
    const long seed = argc > 3 ? std::atol(argv[3]) : 1;
    Rng rng((uint64_t)seed);

    int named = 0;
    for (const Crafted &c : kCrafted) {
        std::vector<unsigned> d(c.e, c.e + 4);
        const std::vector<unsigned> tail = generate(rng, 60, true); // what follows pushes the group's bytes out
        d.insert(d.end(), tail.begin(), tail.end());
        int first = -1;
        bool ok = run_stream(c.name, 0, c.start, d, false, nullptr, &first);
        ok = run_stream(c.name, 1, c.start, d, true, nullptr, nullptr) && ok;
        if (first != c.report) { std::printf("%s: reported %d, expected %d\n", c.name, first, c.report); ++g_failed; ok = false; }
        if (ok) { std::printf("crafted: %s: report %d\n", c.name, first); ++named; }
    }

    Windowed stats(kInit);
    long long decisions = 0;
    for (long i = 0; i < streams; ++i) {
        const std::vector<unsigned> d = generate(rng, (size_t)count, (i & 1) != 0);
        run_stream("stream", i, kInit, d, false, &stats, nullptr);
        if (i % 16 == 0) run_stream("stream (every group again)", i, kInit, d, true, nullptr, nullptr);
        decisions += count;
    }
    const double share = stats.groups ? (double)stats.reruns / (double)stats.groups : 0.0;
    std::printf("%ld streams, %lld decisions, %llu groups, %llu again, %.4f bytes peeled per group\n", streams, decisions, stats.groups,
                stats.reruns, stats.groups ? (double)stats.peeled / (double)stats.groups : 0.0);
    std::printf("rerun share %.6f\n", share);
    if (share > 0.01) { std::printf("more than 1 %% of the groups ran again\n"); ++g_failed; }
    std::printf("%d of %zu crafted groups as named, %d failures\n", named, sizeof(kCrafted) / sizeof(kCrafted[0]), g_failed);
    return g_failed ? 1 : 0;
}
