// t1_mq_group_host.cpp -- the host program of the group form of t1_mq_window.h: the producer's side sums a group of four
// decisions into {G, N} (mq_group_add) and packs the queue words, the consumer's side takes the group in one step
// (mq_wide_add_group), peels with the recording round (mq_wide_peel_mark) and reports a zero byte only if a carry crossed its top
// boundary (mq_group_rolled).  Held to a plain transcription of T.800 Figure C.3 (bit-by-bit RENORME, BYTEOUT as drawn), like
// t1_mq_window_host.cpp, whose generator this is.  tests/test_t1_mq_group_host.py builds it with the address and
// undefined-behaviour sanitizers and reads its report.
//
//   t1_mq_group_host [streams [decisions [seed]]]          (defaults 2000, 4000, 1)
//
// Generated streams: even ones use the state of Qe = 0x5601 alone with fair bits, odd ones walk Table C.2 in eight contexts
// whose bits are skewed differently; then streams of every length from 1 to 23 and of lengths 4000 + 1, 2, 3 (a lane's end inside
// a group: the decisions past it are zeros in every field of the queue words).  Every sixteenth stream runs twice more: with every
// group reported long (the kernel's knob mq_window = 3) and with every group sent back (mq_window = 2).  30 000 short streams
// start from states one addend away from a carry into a 0xFF under a 0xFE or 0xFF (hard starts).  Crafted groups start from
// a given (C, CT, B) and are named for the report they must give.  A group that reports is coded again from its starting state
// by a word-wise per-decision coder (the form of the kernel's `four`) from the decisions unpacked out of the queue words.
//
// Every stream must give the reference's bytes and its final state, every crafted group its report, pack and unpack must round
// trip, at most 0.1 % of the generated (lane, group) pairs may be coded again and at most 0.01 % may be long.  Exit status 0 / 1.
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

enum { kCarry = 1, kRolled = 2, kLong = 8 };
enum Mode { kAsShipped, kEveryLong, kEveryAgain };

int g_failed = 0;

// ---- the coder under test: groups of four through the group form of the header
struct Grouped {
    MqWide s;
    std::vector<uint8_t> out;
    unsigned long long groups = 0, reruns = 0, longs = 0, zeros = 0, peeled = 0, rounds[4] = {0, 0, 0, 0};
    explicit Grouped(State st) : s(j2k_hip::mq_wide_from(st.C, st.CT, st.B)) {}
    int group(const unsigned (&e)[4], Mode mode)
    {
        // the producer's side: {G, N} by one step per decision, and the four queue words
        unsigned G = 0, N = 0;
        for (unsigned e1 : e) j2k_hip::mq_group_add(G, N, e1 & 0xffffu, e1 >> 16);
        const unsigned words[4] = {G, j2k_hip::mq_group_pack_shifts(e[0] >> 16, e[1] >> 16, e[2] >> 16, e[3] >> 16, N),
                                   j2k_hip::mq_group_pack_addends(e[0] & 0xffffu, e[1] & 0xffffu),
                                   j2k_hip::mq_group_pack_addends(e[2] & 0xffffu, e[3] & 0xffffu)};
        // the consumer's side reads the words and nothing else
        const MqWide s0 = s;
        const size_t n0 = out.size();
        const unsigned Nq = j2k_hip::mq_group_N(words[1]);
        int report = 0;
        if (j2k_hip::mq_group_is_long(Nq)) { report |= kLong; ++longs; }
        else if (mode == kEveryLong) report |= kLong; // (the knob: the long protocol at every group, no peel)
        if (!j2k_hip::mq_group_is_long(Nq)) {
            // (the bound the header proves: G is the exact 64-bit sum)
            unsigned long long G64 = 0;
            for (unsigned e1 : e) G64 = (G64 + (e1 & 0xffffu)) << (e1 >> 16);
            if (G64 != words[0]) { std::printf("G %x is not the exact sum %llx at N = %u\n", words[0], G64, Nq); ++g_failed; }
        }
        j2k_hip::mq_wide_add_group(s, words[0], Nq);
        if (!report) {
            if (j2k_hip::mq_wide_is_wide(s)) { std::printf("a group that is not long is wide: w = %u\n", s.w); ++g_failed; }
            if (j2k_hip::mq_wide_has_carry(s)) report |= kCarry;
        }
        if (!report) {
            const unsigned long long V_after = s.V;
            unsigned zpos = j2k_hip::kMqNoZero, r = 0;
            while (j2k_hip::mq_wide_due(s)) { out.push_back((uint8_t)j2k_hip::mq_wide_peel_mark(s, true, zpos)); ++peeled; ++r; }
            ++rounds[r < 3 ? r : 3];
            if (zpos != j2k_hip::kMqNoZero) ++zeros;
            if (j2k_hip::mq_group_rolled(V_after, s0.V, Nq, zpos)) report |= kRolled;
        }
        ++groups;
        if (report) ++reruns;
        if (report || mode != kAsShipped) {
            out.resize(n0);
            Words w{0, 0, 0, &out};
            j2k_hip::mq_wide_to(s0, w.C, w.CT, w.B);
            for (unsigned jj = 0; jj < 4; ++jj) {
                const unsigned d = j2k_hip::mq_group_decision(words[1], words[2], words[3], jj);
                if (d != e[jj]) { std::printf("decision %u unpacked as %x, queued as %x\n", jj, d, e[jj]); ++g_failed; }
                w.decision(d);
            }
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

// One stream from `start` through the reference and the grouped coder; the report of the first group goes to *first.
bool run_stream(const char *name, long id, State start, const std::vector<unsigned> &dec, Mode mode, Grouped *stats, int *first)
{
    Plain ref(start);
    for (unsigned e : dec) ref.decision(e);
    Grouped grp(start);
    for (size_t i = 0; i < dec.size(); i += 4) {
        unsigned e[4] = {0, 0, 0, 0}; // (past the end: decisions that change nothing, as the producer queues them)
        for (size_t j = 0; j < 4 && i + j < dec.size(); ++j) e[j] = dec[i + j];
        const int report = grp.group(e, mode);
        if (i == 0 && first) *first = report;
    }
    if (stats) {
        stats->groups += grp.groups; stats->reruns += grp.reruns; stats->longs += grp.longs; stats->zeros += grp.zeros;
        stats->peeled += grp.peeled;
        for (int r = 0; r < 4; ++r) stats->rounds[r] += grp.rounds[r];
    }
    bool ok = true;
    if (grp.out.size() != ref.out.size()) { std::printf("%s %ld: %zu bytes, the reference has %zu\n", name, id, grp.out.size(), ref.out.size()); ok = false; }
    for (size_t i = 0; ok && i < ref.out.size(); ++i)
        if (grp.out[i] != ref.out[i]) { std::printf("%s %ld: byte %zu is %02x, the reference has %02x\n", name, id, i, grp.out[i], ref.out[i]); ok = false; }
    const MqWide want = j2k_hip::mq_wide_from(ref.C, ref.CT, ref.B);
    if (ok && (grp.s.V != want.V || grp.s.w != want.w)) {
        std::printf("%s %ld: final state (%llx, %u), the reference has (%llx, %u)\n", name, id, grp.s.V, grp.s.w, want.V, want.w);
        ok = false;
    }
    if (!ok) ++g_failed;
    return ok;
}

bool run_all_modes(const char *name, long id, State start, const std::vector<unsigned> &dec)
{
    bool ok = run_stream(name, id, start, dec, kAsShipped, nullptr, nullptr);
    ok = run_stream(name, id, start, dec, kEveryLong, nullptr, nullptr) && ok;
    return run_stream(name, id, start, dec, kEveryAgain, nullptr, nullptr) && ok;
}

struct Crafted { const char *name; State start; unsigned e[4]; int report; };
constexpr unsigned dec(unsigned addend, unsigned n) { return addend | (n << 16); }
const Crafted kCrafted[] = {
    // eight shifts finish a byte of 0xFF, then a carry reaches it: 0xFF -> 0x00, the byte above 0x12 -> 0x13
    {"finished 0xFF rolls", {0x7ffffu, 8, 0x12}, {dec(0, 8), dec(0x100, 0), dec(0, 0), dec(0, 0)}, kRolled},
    // the same under a 0xFE: the carry makes it 0xFF and goes no further, so nothing changes above the lowest bit of the byte
    // above the zero -- and behind the 0xFF the zero's own window begins one bit higher, on the zero slot
    {"finished 0xFF rolls under a 0xFE", {0x7ffffu, 8, 0xfe}, {dec(0, 8), dec(0x100, 0), dec(0, 0), dec(0, 0)}, kRolled},
    // a byte that is zero by itself, well above the addends: no carry leaves its top, nothing to report
    {"true 0x00 byte", {0x00055u, 8, 0x12}, {dec(0, 8), dec(0x55, 0), dec(0, 0), dec(0, 0)}, 0},
    // the carry crosses the byte's top boundary while the byte is still part of C and leaves it 0x00: the test cannot tell
    // that from a byte frozen as 0xFF, and reports
    {"0x00 byte, a carry crossed its top", {0x7ffffu, 8, 0x12}, {dec(1, 0), dec(0, 8), dec(0, 0), dec(0, 0)}, kRolled},
    // B = 0xFF pending behind 20 set bits of C; the last decision's addend carries out of them
    {"pending 0xFF, late carry", {0xfffffu, 7, 0xff}, {dec(0, 0), dec(0, 0), dec(0, 0), dec(1, 0)}, kCarry},
    // a pending 0xFE that a carry of this group makes 0xFF before it goes out: no report, the byte behind it takes seven bits
    {"pending 0xFE becomes 0xFF", {0x7ffffu, 8, 0xfe}, {dec(1, 1), dec(0x5601, 7), dec(0, 0), dec(0, 0)}, 0},
    // the edge of the bound: the largest G that is not long -- every addend 0x5601, all fifteen shifts behind the last one.
    // (No interval register yields these four in a row, and from CT = 12 they would carry twice into one byte, which Figure C.3
    // cannot hold: the starts are such that C stays within its 28 bits.)
    {"N = 15, G at its bound", {0, 5, 0x34}, {dec(0x5601, 0), dec(0x5601, 0), dec(0x5601, 0), dec(0x5601, 15)}, 0},
    {"N = 15, G at its bound, widest start", {0x155u, 1, 0x34}, {dec(0x5601, 0), dec(0x5601, 0), dec(0x5601, 0), dec(0x5601, 15)}, 0},
    {"N = 16", {0, 12, 0}, {dec(0x5601, 1), dec(0x5601, 0), dec(0x5601, 0), dec(0x5601, 15)}, kLong},
    {"four shifts of 15", {0x155u, 1, 0x34}, {dec(0x5601, 15), dec(0x0001, 15), dec(0x2201, 15), dec(0x0005, 15)}, kLong},
    // the block's first byte: CT = 12, the pad byte goes out, the byte behind it is not zero
    {"first byte", {0, 12, 0}, {dec(0x1601, 1), dec(0x0AC1, 2), dec(0x0521, 4), dec(0x0221, 6)}, 0},
};

// every shift in every slot with every Qe of Table C.2 beside it, through pack and unpack
long pack_round_trips()
{
    long checked = 0;
    for (unsigned slot = 0; slot < 4; ++slot)
        for (unsigned n = 0; n < 16; ++n)
            for (unsigned q = 0; q < 47; ++q) {
                unsigned e[4];
                for (unsigned jj = 0; jj < 4; ++jj) e[jj] = dec(kQeTab[(q + 11u * jj) % 47u], (n + 5u * jj + slot) & 15u);
                e[slot] = dec(kQeTab[q], n);
                for (unsigned zero_addend = 0; zero_addend < 2; ++zero_addend) {
                    if (zero_addend) e[slot] = dec(0, n);
                    unsigned G = 0, N = 0;
                    for (unsigned e1 : e) j2k_hip::mq_group_add(G, N, e1 & 0xffffu, e1 >> 16);
                    const unsigned shifts = j2k_hip::mq_group_pack_shifts(e[0] >> 16, e[1] >> 16, e[2] >> 16, e[3] >> 16, N);
                    const unsigned a01 = j2k_hip::mq_group_pack_addends(e[0] & 0xffffu, e[1] & 0xffffu);
                    const unsigned a23 = j2k_hip::mq_group_pack_addends(e[2] & 0xffffu, e[3] & 0xffffu);
                    unsigned stepwise = 0;
                    for (unsigned jj = 0; jj < 4; ++jj) stepwise = j2k_hip::mq_group_add_shift(stepwise, e[jj] >> 16, jj);
                    const bool high = stepwise == shifts &&
j2k_hip::mq_group_pack_addends_high(e[0] << 16, e[1] << 16) == a01 &&
                                      j2k_hip::mq_group_pack_addends_high(e[2] << 16, e[3] << 16) == a23;
                    bool ok = high && j2k_hip::mq_group_N(shifts) ==(e[0] >> 16) + (e[1] >> 16) + (e[2] >> 16) + (e[3] >> 16);
                    for (unsigned jj = 0; jj < 4; ++jj) ok = ok && j2k_hip::mq_group_decision(shifts, a01, a23, jj) == e[jj];
                    if (!ok) { std::printf("pack: slot %u shift %u Qe %04x does not round trip\n", slot, n, kQeTab[q]); ++g_failed; }
                    ++checked;
                }
            }
    return checked;
}

} // namespace

int main(int argc, char **argv)
{
    const long streams = argc > 1 ? std::atol(argv[1]) : 2000;
    const long count = argc > 2 ? std::atol(argv[2]) : 4000;
    const long seed = argc > 3 ? std::atol(argv[3]) : 1;

    // the generated streams first: they are the generator's own for this seed
    Rng rng((uint64_t)seed);
    Grouped stats(kInit);
    long long decisions = 0;
    for (long i = 0; i < streams; ++i) {
        const std::vector<unsigned> d = generate(rng, (size_t)count, (i & 1) != 0);
        run_stream("stream", i, kInit, d, kAsShipped, &stats, nullptr);
        if (i % 16 == 0) {
            run_stream("stream (every group long)", i, kInit, d, kEveryLong, nullptr, nullptr);
            run_stream("stream (every group again)", i, kInit, d, kEveryAgain, nullptr, nullptr);
        }
        decisions += count;
    }

    Rng rng2((uint64_t)seed + 77u);
    long odd = 0;
    for (long len = 1; len <= 23; ++len)
        for (int mixed = 0; mixed < 2; ++mixed) { run_all_modes("short stream", len, kInit, generate(rng2, (size_t)len, mixed != 0)); ++odd; }
    for (long extra = 1; extra <= 3; ++extra)
        for (int k = 0; k < 8; ++k) { run_all_modes("odd stream", count + extra, kInit, generate(rng2, (size_t)(count + extra), (k & 1) != 0)); ++odd; }

    // Hard starts: the generated streams seldom put a 0xFF under a 0xFE and a carry behind both -- what the frames of a real
    // sequence do every few million decisions.  Short streams from states that are one addend away from it: the pending byte
    // 0xFD..0xFF, the live bits of C all ones but for a few low ones, every CT.
    long hard = 0;
    for (long i = 0; i < 30000; ++i) {
        const unsigned CT = 1u + rng2.next() % 8u, live = 27u - CT;
        State st;
        st.CT = CT;
        st.B = 0xfdu + rng2.next() % 3u;
        st.C = ((1u << live) - 1u) - (rng2.next() & 0xfffu & ((1u << live) - 1u));
        if (rng2.next() & 1u) st.C &= ~(0xffu << (live > 12u ? live - 12u : 0u)) | (rng2.next() << 8); // (holes below the top byte)
        st.C &= (1u << live) - 1u;
        const std::vector<unsigned> d = generate(rng2, 24, (i & 1) != 0);
        run_stream("hard start", i, st, d, kAsShipped, nullptr, nullptr);
        if (i % 8 == 0) { run_stream("hard start", i, st, d, kEveryLong, nullptr, nullptr); run_stream("hard start", i, st, d, kEveryAgain, nullptr, nullptr); }
        ++hard;
    }
    std::printf("%ld hard starts\n", hard);

    int named = 0;
    for (const Crafted &c : kCrafted) {
        std::vector<unsigned> d(c.e, c.e + 4);
        const std::vector<unsigned> tail = generate(rng2, 60, true); // what follows pushes the group's bytes out
        d.insert(d.end(), tail.begin(), tail.end());
        int first = -1;
        bool ok = run_stream(c.name, 0, c.start, d, kAsShipped, nullptr, &first);
        ok = run_stream(c.name, 1, c.start, d, kEveryLong, nullptr, nullptr) && ok;
        ok = run_stream(c.name, 2, c.start, d, kEveryAgain, nullptr, nullptr) && ok;
        if (first != c.report) { std::printf("%s: reported %d, expected %d\n", c.name, first, c.report); ++g_failed; ok = false; }
        if (ok) { std::printf("crafted: %s: report %d\n", c.name, first); ++named; }
    }

    const long packed = pack_round_trips();
    std::printf("pack: %ld groups round trip\n", packed);

    const double g = stats.groups ? (double)stats.groups : 1.0;
    std::printf("%ld streams, %lld decisions, %llu groups, %llu again, %llu long, %llu with a zero byte, %.4f bytes peeled per group\n",
                streams, decisions, stats.groups, stats.reruns, stats.longs, stats.zeros, (double)stats.peeled / g);
    std::printf("peel rounds per group: 0 in %.4f, 1 in %.4f, 2 in %.4f, more in %.4f\n", stats.rounds[0] / g, stats.rounds[1] / g,
                stats.rounds[2] / g, stats.rounds[3] / g);
    std::printf("%ld streams whose length is no multiple of four or below a chunk\n", odd);
    std::printf("rerun share %.6f\n", stats.reruns / g);
    std::printf("long share %.6f\n", stats.longs / g);
    std::printf("zero share %.6f\n", stats.zeros / g);
    if (stats.reruns == 0) { std::printf("no group ran again\n"); ++g_failed; }
    if (stats.reruns / g > 0.001) { std::printf("more than 0.1 %% of the groups ran again\n"); ++g_failed; }
    if (stats.longs / g > 0.0001) { std::printf("more than 0.01 %% of the groups were long\n"); ++g_failed; }
    std::printf("%d of %zu crafted groups as named, %d failures\n", named, sizeof(kCrafted) / sizeof(kCrafted[0]), g_failed);
    return g_failed ? 1 : 0;
}
