// The lane-per-block Tier-1 decoder (j2k_amd/csrc/t1_dec_lane.h) under code-block styles, as a stand-alone host program with
// ONE lane: the per-lane state machine is the HIP kernel's own source.  tests/test_t1_lane_styled_host.py builds this file
// with the address and undefined-behaviour sanitizers, writes a case file and runs it; nothing is loaded into Python.
//
// Case file (little endian): "T1LD", u32 cases; per case u32 style, reversible, w, h, orient, numbps, npasses, roishift, half_step
// (float bits), cw_len, nsegs, then nsegs x (u32 bytes, u32 passes), cw_len codeword bytes, u32 has_words, and when that is 1 the
// w x h 32-bit words a decode must leave in the block's rectangle (int32, or float32 bit patterns).  A block that holds
// nothing (no pass, no bit-plane) has no words and is not decoded: the rule of a file decode (decode_plan.h: t1dec_passes).
// The codeword lies in an arena of its own with the product's padding rule (cw_arena_next, cw_arena_bytes), zeros behind its
// last byte, allocated to the byte: a read past what the kernel may read is the sanitizer's to report.  Segment words are
// the plan's (cwseg_have, cwseg_word).  Exit status 1 and the first mismatch on stdout when a case differs.
#include "../../j2k_amd/csrc/decode_plan.h"
#include "../../j2k_amd/csrc/t1_dec_lane.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace j2k_hip::t1lane;

namespace {

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
        static uint8_t chunk[1 << 16];
        for (size_t n; (n = std::fread(chunk, 1, sizeof chunk, f)) > 0;) in.buf.insert(in.buf.end(), chunk, chunk + n);
        std::fclose(f);
    }
    const uint8_t *magic = in.bytes(4);
    if (!magic || std::memcmp(magic, "T1LD", 4) != 0) { std::fprintf(stderr, "not a case file\n"); return 2; }
    const uint32_t ncases = in.u32();
    static Shared<1> sh;
    unsigned bad = 0, decoded = 0;
    for (uint32_t k = 0; k < ncases; ++k) {
        const uint32_t style = in.u32(), rev = in.u32(), w = in.u32(), h = in.u32(), orient = in.u32(), numbps = in.u32(), npasses = in.u32();
        const uint32_t roishift = in.u32(), hs_bits = in.u32(), cw_len = in.u32(), nsegs = in.u32();
        std::vector<uint32_t> pairs(2 * (size_t)nsegs);
        for (uint32_t &x : pairs) x = in.u32();
        const uint8_t *cw = in.bytes(cw_len);
        const uint32_t has_words = in.u32();
        const uint8_t *wantp = has_words ? in.bytes((size_t)w * h * 4) : nullptr;
        if (!in.ok || w < 1 || h < 1 || w > 64 || h > 64 || orient > 3 || numbps > 30 || roishift > 30 || style > 63 || has_words > 1) {
            std::fprintf(stderr, "bad case %u\n", k);
            return 2;
        }
        const uint32_t np = j2k_hip::t1dec_passes(numbps, npasses);
        if (!np) {
            if (has_words) { std::printf("case %u: a block that holds nothing came with expected words\n", k); ++bad; }
            continue;
        }
        const bool multiseg = (style & 5u) != 0;
        if (!has_words || (multiseg && !nsegs) || (!multiseg && nsegs)) { std::fprintf(stderr, "bad case %u\n", k); return 2; }
        std::vector<uint32_t> words;
        uint64_t at = 0;
        for (uint32_t i = 0; i < nsegs; ++i) {
            if (pairs[2 * i] > j2k_hip::kCwSegMaxBytes || pairs[2 * i + 1] > j2k_hip::kCwSegMaxPasses) { std::fprintf(stderr, "bad case %u\n", k); return 2; }
            words.push_back(j2k_hip::cwseg_word(j2k_hip::cwseg_have(pairs[2 * i], at, cw_len), pairs[2 * i + 1]));
            at += pairs[2 * i];
        }
        const size_t arena = (size_t)j2k_hip::cw_arena_bytes(j2k_hip::cw_arena_next(cw_len));
        uint8_t *base = static_cast<uint8_t *>(std::aligned_alloc(16, arena));
        if (!base) return 2;
        std::memset(base, 0, arena);
        if (cw_len) std::memcpy(base, cw, cw_len);
        Block b{base, cw_len, (int)w, (int)h, (int)orient, (int)np, multiseg ? words.data() : nullptr, multiseg ? nsegs : 0u};
        init_shared<1>(sh, 0);
        std::vector<uint32_t> state(kGroupWords, 0), planes((size_t)(numbps + 1) * 16 * 8, 0);
        decode_lane<1>(sh, 0, b, true, (int)np, (int)(h + 3) >> 2, state.data(), planes.data(), style);
        std::free(base);
        ++decoded;
        float half_step;
        std::memcpy(&half_step, &hs_bits, 4);
        const int last = (int)np - 1, kf = last == 0 ? 0 : 1 + (last - 1) / 3;
        bool failed = false;
        for (uint32_t y = 0; y < h && !failed; ++y)
            for (uint32_t x = 0; x < w; ++x) {
                const uint32_t s = y >> 2, r = y & 3;
                uint32_t acc = 0;
                for (int p = 0; p <= kf; ++p)
                    acc |= ((planes[((size_t)p * 16 + s) * 8 + (x >> 3)] >> (4 * (x & 7) + r)) & 1u) << (numbps - (uint32_t)p);
                const bool neg = (state[(size_t)s * 64 + x] >> (W_SGN + 1 + r)) & 1u;
                const int v = roi_unshift(sample_value(acc, neg, (int)numbps, (int)np), (int)roishift);
                uint32_t got, want;
                if (rev) got = (uint32_t)(v / 2);
                else { const float f = (float)v * half_step; std::memcpy(&got, &f, 4); }
                std::memcpy(&want, wantp + 4 * ((size_t)y * w + x), 4);
                if (got != want) {
                    std::printf("case %u (style %u, %u x %u, orient %u, numbps %u, npasses %u, %u bytes, %u segments): sample (y, x) = (%u, %u): got %#x, want %#x\n",
                                k, style, w, h, orient, numbps, np, cw_len, nsegs, y, x, got, want);
                    failed = true;
                    break;
                }
            }
        bad += failed;
    }
    if (!in.ok || in.pos != in.buf.size()) { std::fprintf(stderr, "truncated case file or bytes left over\n"); return 2; }
    std::printf("%u cases, %u decoded, %u with a mismatch\n", ncases, decoded, bad);
    return bad ? 1 : 0;
}
