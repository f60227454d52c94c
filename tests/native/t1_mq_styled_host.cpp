// t1_mq_styled_host.cpp -- the host program of t1_mq_styled.h: StyledCoder, the recurrence the styled coder kernel runs, with
// plain-array tables, a 19-word context array and a std::vector as its byte sink, driven over the decision streams of a case
// file and held to the codewords and segment ends recorded there (tests/test_t1_mq_styled_host.py writes the file from the
// CPU oracle and builds this with the address and undefined-behaviour sanitizers).
//
//   t1_mq_styled_host <case file>
//
// Case file, little-endian 32-bit words and bytes:
//   "T1SC", nstreams, then per stream: nsym, nsym decision bytes ((context << 1) | bit, as the modeller writes them)
//   ncases, then per case: block id, style, stream index, npasses, pass_nsym[npasses] (decisions up to the end of each pass),
//     seg_end[npasses] (the byte count where the pass ends a codeword segment, 0xffffffff where it does not), ncw, ncw bytes
// Prints the first mismatch of every case that has one; exit status 1 if any, 2 for a file it cannot read.
//
// Every case runs three times: into the vector; into StageSink, a model of the kernel's byte stage (t1_mq_styled.hip: a zero
// pad word, bytes staged behind it, whole 16-byte units leave once 64 wait -- after every pass end and after every 16
// decisions -- and 16..31 stay), which must give the same codeword; and into a StageSink that keeps 0..15 bytes instead.
// The third is a deliberately wrong stage: where a termination looks back at bytes that such a drain has already let go,
// its codeword differs, and the program names the case ("tells the stages apart").  A case that does so on the host holds
// the kernel's drain to its 16..31 bytes on the GPU; the test asks for such cases by name.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "t1_mq_styled.h"

namespace {

// T.800 Table C.2: Qe, NMPS, NLPS, SWITCH
const uint16_t kQeTab[47] = {0x5601, 0x3401, 0x1801, 0x0AC1, 0x0521, 0x0221, 0x5601, 0x5401, 0x4801, 0x3801, 0x3001, 0x2401,
                             0x1C01, 0x1601, 0x5601, 0x5401, 0x5101, 0x4801, 0x3801, 0x3401, 0x3001, 0x2801, 0x2401, 0x2201,
                             0x1C01, 0x1801, 0x1601, 0x1401, 0x1201, 0x1101, 0x0AC1, 0x09C1, 0x08A1, 0x0521, 0x0441, 0x02A1,
                             0x0221, 0x0141, 0x0111, 0x0085, 0x0049, 0x0025, 0x0015, 0x0009, 0x0005, 0x0001, 0x5601};
const uint8_t kNmpsTab[47] = {1, 2, 3, 4, 5, 38, 7, 8, 9, 10, 11, 12, 13, 29, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24,
                              25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 45, 46};
const uint8_t kNlpsTab[47] = {1, 6, 9, 12, 29, 33, 6, 14, 14, 14, 17, 18, 20, 21, 14, 14, 15, 16, 17, 18, 19, 19, 20, 21,
                              22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 46};
const uint8_t kSwitchTab[47] = {1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1};

struct ArrayTab {
    unsigned mps[94], lps[94]; // [Table C.2 index << 1 | MPS]
    ArrayTab()
    {
        for (unsigned i = 0; i < 47; ++i)
            for (unsigned m = 0; m < 2; ++m) {
                mps[i * 2 + m] = ((unsigned)kQeTab[i] << 16) | ((unsigned)kNmpsTab[i] << 1) | m;
                lps[i * 2 + m] = ((unsigned)kNlpsTab[i] << 1) | (m ^ kSwitchTab[i]);
            }
    }
    unsigned mps_entry(unsigned st) const { return mps[st]; }
    unsigned lps_next(unsigned st) const { return lps[st]; }
};
struct ArrayCtx {
    unsigned st[19];
    unsigned get(unsigned c) const { return st[c]; }
    void set(unsigned c, unsigned s) { st[c] = s; }
};
struct VectorSink {
    std::vector<uint8_t> v;
    void put(unsigned b) { v.push_back((uint8_t)b); }
    void drop(unsigned n) { v.resize(v.size() - n); } // (more than there is: the sanitizers report it)
    unsigned peek(unsigned k) const { return k < v.size() ? v[v.size() - 1 - k] : 0u; } // before the first byte: zero
    unsigned size() const { return (unsigned)v.size(); }
};

// the kernel's LDS stage of one lane (kStage = 160 bytes behind a pad word of zeros; the drain's rule as in the kernel)
struct StageSink {
    static constexpr unsigned kPad = 4, kStage = 160;
    std::vector<uint8_t> hbm; // the whole 16-byte units that have left
    uint8_t buf[kPad + kStage] = {};
    unsigned pos = 0;
    bool keeps_a_unit; // true: the kernel's drain, 16..31 bytes stay; false: 0..15 stay
    bool lost = false; // a look or a take-back went in front of the pad word, or the stage overflowed
    explicit StageSink(bool keep) : keeps_a_unit(keep) {}
    void put(unsigned b) { buf[kPad + (pos < kStage ? pos : kStage - 1)] = (uint8_t)b; ++pos; }
    void drop(unsigned n) { if (n > pos) { lost = true; pos = 0; } else pos -= n; }
    unsigned peek(unsigned k) const { return k < pos + kPad ? buf[kPad + pos - 1 - k] : 0u; }
    unsigned size() const { return (unsigned)hbm.size() + pos; }
    void drain()
    {
        if (pos < 64) return;
        if (pos > kStage) { lost = true; pos = kStage; }
        const unsigned units = (pos >> 4) - (keeps_a_unit ? 1u : 0u);
        hbm.insert(hbm.end(), buf + kPad, buf + kPad + 16 * units);
        std::memmove(buf + kPad, buf + kPad + 16 * units, pos - 16 * units);
        pos -= 16 * units;
    }
    std::vector<uint8_t> all() const
    {
        std::vector<uint8_t> v = hbm;
        v.insert(v.end(), buf + kPad, buf + kPad + (pos < kStage ? pos : kStage));
        return v;
    }
};
inline void drain(VectorSink &) {}
inline void drain(StageSink &s) { s.drain(); }

struct Stream { const uint8_t *sym; uint32_t nsym; };

// One block through StyledCoder in the kernel's order: the passes that end in front of decision i are closed before it is
// coded, the stage drains behind every pass end and behind every 16 decisions.  Returns the passes closed.
template <class Sink>
uint32_t code_block(const ArrayTab &tab, Sink &sink, uint32_t style, const Stream &s, const std::vector<uint32_t> &pass_nsym, std::vector<uint32_t> &rate)
{
    ArrayTab t = tab;
    ArrayCtx ctx{};
    j2k_hip::StyledCoder<ArrayTab, ArrayCtx, Sink> coder(t, ctx, sink, style);
    coder.begin_block();
    const uint32_t np = (uint32_t)pass_nsym.size();
    uint32_t p = 0;
    for (uint32_t i = 0; i <= s.nsym; ++i) {
        while (p < np && pass_nsym[p] == i) { rate[p] = coder.end_pass(p, np); ++p; drain(sink); }
        if (i < s.nsym) coder.decision(s.sym[i]);
        if (i % 16 == 15 || i + 1 == s.nsym) drain(sink);
    }
    return p;
}

struct Reader {
    std::vector<uint8_t> buf;
    size_t pos = 0;
    bool ok = true;
    uint32_t u32()
    {
        if (pos + 4 > buf.size()) { ok = false; return 0; }
        const uint32_t x = buf[pos] | (buf[pos + 1] << 8) | (buf[pos + 2] << 16) | ((uint32_t)buf[pos + 3] << 24);
        pos += 4;
        return x;
    }
    const uint8_t *bytes(size_t n)
    {
        if (n > buf.size() - pos) { ok = false; return nullptr; }
        const uint8_t *p = buf.data() + pos;
        pos += n;
        return p;
    }
};

} // namespace

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s <case file>\n", argv[0]); return 2; }
    Reader in;
    {
        FILE *f = std::fopen(argv[1], "rb");
        if (!f) { std::perror(argv[1]); return 2; }
        uint8_t chunk[1 << 16];
        for (size_t n; (n = std::fread(chunk, 1, sizeof chunk, f)) > 0;) in.buf.insert(in.buf.end(), chunk, chunk + n);
        std::fclose(f);
    }
    const uint8_t *magic = in.bytes(4);
    if (!magic || magic[0] != 'T' || magic[1] != '1' || magic[2] != 'S' || magic[3] != 'C') { std::fprintf(stderr, "not a case file\n"); return 2; }
    std::vector<Stream> streams(in.u32());
    for (Stream &s : streams) { s.nsym = in.u32(); s.sym = in.bytes(s.nsym); }
    const uint32_t ncases = in.u32();
    if (!in.ok) { std::fprintf(stderr, "truncated case file\n"); return 2; }

    const ArrayTab tab;
    unsigned bad = 0, apart = 0;
    for (uint32_t k = 0; k < ncases; ++k) {
        const uint32_t block = in.u32(), style = in.u32(), si = in.u32(), np = in.u32();
        std::vector<uint32_t> pass_nsym(np), seg_end(np);
        for (uint32_t &x : pass_nsym) x = in.u32();
        for (uint32_t &x : seg_end) x = in.u32();
        const uint32_t ncw = in.u32();
        const uint8_t *cw = in.bytes(ncw);
        if (!in.ok || si >= streams.size() || (np && pass_nsym[np - 1] != streams[si].nsym)) { std::fprintf(stderr, "bad case %u\n", k); return 2; }

        VectorSink sink;
        std::vector<uint32_t> rate(np);
        const Stream &s = streams[si];
        const uint32_t p = code_block(tab, sink, style, s, pass_nsym, rate);
        bool failed = false;
        auto fail = [&](const char *what, long at, long got, long want) {
            if (!failed) std::printf("block %u style %u: %s at %ld: got %ld, want %ld\n", block, style, what, at, got, want);
            failed = true;
        };
        if (p != np) fail("passes closed", 0, p, np);
        for (uint32_t q = 0; q < np; ++q)
            if (seg_end[q] != 0xffffffffu && rate[q] != seg_end[q]) fail("segment end of pass", q, rate[q], seg_end[q]);
        const uint32_t got = np ? sink.size() : 0;
        if (got != ncw) fail("codeword length", 0, got, ncw);
        for (uint32_t i = 0; i < ncw && i < got; ++i)
            if (sink.v[i] != cw[i]) { fail("codeword byte", i, sink.v[i], cw[i]); break; }
        if (np) {
            StageSink staged(true), narrow(false);
            std::vector<uint32_t> srate(np), nrate(np);
            code_block(tab, staged, style, s, pass_nsym, srate);
            if (staged.lost || staged.all() != sink.v || srate != rate) fail("the staged codeword: bytes", 0, (long)staged.size(), got);
            code_block(tab, narrow, style, s, pass_nsym, nrate);
            if (narrow.lost || narrow.all() != sink.v || nrate != rate) {
                std::printf("block %u style %u tells the stages apart\n", block, style);
                ++apart;
            }
        }
        bad += failed;
    }
    std::printf("%u cases tell a stage that keeps 0..15 bytes from the kernel's\n", apart);
    std::printf("%u cases, %u with a mismatch\n", ncases, bad);
    return bad ? 1 : 0;
}
