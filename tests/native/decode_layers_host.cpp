// decode_layers_host.cpp -- the layer limit of the Tier-2 planner (decode_plan.cpp: plan_decode's max_layers) as a stand-alone
// program for ASan / UBSan (tests/test_decode_layers_refs.py builds and runs it; no HIP, no device).
//
// The manifest named on the command line has one line per file: `layers file strip_1 ... strip_layers`, strip_L being the
// same file cut down to its first L layers by the tests' Python helper (tests/layers_cases.py: packets removed, COD's layer
// count set, Psot fixed).  For every file and every L, at reduce 0 and 1, for the whole image and for a window:
// plan_decode(file, ..., L) must equal plan_decode(strip_L, ...) block for block -- identity, bit-planes, coding passes, the
// codeword bytes gathered from each file's own pieces, the codeword segment table.  L = 0, L = layers and L = layers + 7 must
// give the file's own plan.  Then 200 seeded mutations of every file at L = 1: each must plan soundly or end in an Error.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>

#include "../../j2k_amd/csrc/decode_plan.h"

using namespace j2k_hip;

static uint32_t lcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return s >> 8; }

static std::vector<uint8_t> slurp(const std::string &path)
{
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

// what the device code takes on trust from a plan (as tests/native/decode_sanitize.cpp states it)
static const char *plan_fault(const DecodePlan &P, size_t file_len)
{
    for (const DecSeg &s : P.segs)
        if (s.src + s.len > file_len || s.dst + s.len > P.arena_bytes) return "segment out of range";
    for (const DecBlock &b : P.blocks) {
        if (b.cw_off + b.cw_len > P.arena_bytes) return "block segment outside the arena";
        if (b.numbps == 0 || b.numbps > 30) return "bit-plane count outside 1..30";
        if (b.npasses == 0 || b.npasses > 3u * b.numbps - 2u) return "more coding passes than the block's bit-planes allow";
        if (b.cblk >= P.geo.cblks.size()) return "block index outside the geometry";
        if ((size_t)b.seg_first + b.nsegs > P.cwsegs.size()) return "codeword segments outside their table";
        uint64_t bytes = 0, passes = 0;
        for (uint32_t k = 0; k < b.nsegs; ++k) { bytes += P.cwsegs[b.seg_first + k] & kCwSegMaxBytes; passes += P.cwsegs[b.seg_first + k] >> 24; }
        // (a file cut short inside a packet: its header's passes are in the table, the bodies that did not arrive are not in npasses)
        if (b.nsegs && (bytes > b.cw_len || passes < b.npasses)) return "codeword segments that do not cover the block";
    }
    return nullptr;
}

// the codeword arena as the gather kernel fills it
static std::vector<uint8_t> arena_of(const DecodePlan &P, const std::vector<uint8_t> &file)
{
    std::vector<uint8_t> a(P.arena_bytes, 0);
    for (const DecSeg &s : P.segs) std::memcpy(a.data() + s.dst, file.data() + s.src, s.len);
    return a;
}

// "" when the two plans hand Tier-1 the same work
static std::string differ(const DecodePlan &A, const std::vector<uint8_t> &fa, const DecodePlan &B, const std::vector<uint8_t> &fb)
{
    if (A.blocks.size() != B.blocks.size()) return "blocks: " + std::to_string(A.blocks.size()) + " against " + std::to_string(B.blocks.size());
    if (A.arena_bytes != B.arena_bytes) return "arena size";
    if (A.geo.cblks.size() != B.geo.cblks.size()) return "geometry";
    const std::vector<uint8_t> aa = arena_of(A, fa), ab = arena_of(B, fb);
    for (size_t i = 0; i < A.blocks.size(); ++i) {
        const DecBlock &a = A.blocks[i], &b = B.blocks[i];
        const Cblk &ca = A.geo.cblks[a.cblk], &cb = B.geo.cblks[b.cblk];
        const std::string at = " of block " + std::to_string(i);
        if (a.cblk != b.cblk || ca.tile != cb.tile || ca.comp != cb.comp || ca.res != cb.res || ca.band != cb.band || ca.px != cb.px || ca.py != cb.py ||
            ca.w != cb.w || ca.h != cb.h)
            return "identity" + at;
        if (a.numbps != b.numbps) return "bit-planes" + at;
        if (a.npasses != b.npasses) return "passes" + at + ": " + std::to_string(a.npasses) + " against " + std::to_string(b.npasses);
        if (a.roishift != b.roishift) return "region-of-interest shift" + at;
        if (a.cw_len != b.cw_len || a.cw_off != b.cw_off) return "codeword length or place" + at;
        if (std::memcmp(aa.data() + a.cw_off, ab.data() + b.cw_off, a.cw_len) != 0) return "codeword bytes" + at;
        if (a.nsegs != b.nsegs) return "segment count" + at + ": " + std::to_string(a.nsegs) + " against " + std::to_string(b.nsegs);
        for (uint32_t k = 0; k < a.nsegs; ++k)
            if (A.cwsegs[a.seg_first + k] != B.cwsegs[b.seg_first + k]) return "segment " + std::to_string(k) + at;
    }
    return std::string();
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: decode_layers_host manifest\n"); return 2; }
    const char *env_seed = std::getenv("J2K_FUZZ_SEED");
    const uint32_t seed0 = env_seed ? (uint32_t)std::strtoul(env_seed, nullptr, 10) : 24680u;
    std::ifstream mf(argv[1]);
    std::string line;
    size_t compared = 0, files = 0, cut_blocks = 0, partial_raw = 0, mutated_ok = 0, rejected = 0;
    while (std::getline(mf, line)) {
        std::istringstream ls(line);
        uint32_t layers = 0;
        std::string path;
        if (!(ls >> layers >> path) || !layers) continue;
        const std::vector<uint8_t> file = slurp(path);
        if (file.empty()) { std::fprintf(stderr, "FAIL: cannot read %s\n", path.c_str()); return 1; }
        std::vector<std::vector<uint8_t>> strips(layers);
        for (uint32_t l = 0; l < layers; ++l) {
            std::string sp;
            if (!(ls >> sp) || (strips[l] = slurp(sp)).empty()) { std::fprintf(stderr, "FAIL: no strip %u of %s\n", l + 1, path.c_str()); return 1; }
        }
        const FileHeader H = parse_headers(file.data(), file.size());
        if (H.cod.layers != layers) { std::fprintf(stderr, "FAIL: %s has %u layers, not %u\n", path.c_str(), H.cod.layers, layers); return 1; }
        ++files;
        for (uint32_t reduce = 0; reduce < 2 && reduce < H.cod.numres; ++reduce) {
            int ow, oh;
            reduced_size(H.cod, reduce, ow, oh);
            const uint32_t W = (uint32_t)ow, Hh = (uint32_t)oh;
            const uint32_t win[4] = {W / 3, Hh / 3, (W + 2) / 3, (Hh + 2) / 3};
            for (int windowed = 0; windowed < 2; ++windowed) {
                const uint32_t *w = windowed ? win : nullptr;
                const DecodePlan own = plan_decode(file.data(), file.size(), reduce, w);
                for (uint32_t L : {0u, layers, layers + 7u}) {
                    const DecodePlan P = plan_decode(file.data(), file.size(), reduce, w, L);
                    const std::string why = differ(P, file, own, file);
                    if (!why.empty() || P.segs.size() != own.segs.size() || P.cwsegs != own.cwsegs) {
                        std::fprintf(stderr, "FAIL: %s, limit %u is not the file's own plan: %s\n", path.c_str(), L, why.c_str());
                        return 1;
                    }
                }
                for (uint32_t L = 1; L <= layers; ++L) {
                    const DecodePlan P = plan_decode(file.data(), file.size(), reduce, w, L);
                    const DecodePlan R = plan_decode(strips[L - 1].data(), strips[L - 1].size(), reduce, w);
                    if (R.hdr.cod.layers != L) { std::fprintf(stderr, "FAIL: strip %u of %s has %u layers\n", L, path.c_str(), R.hdr.cod.layers); return 1; }
                    if (const char *f = plan_fault(P, file.size())) { std::fprintf(stderr, "FAIL: %s, limit %u: %s\n", path.c_str(), L, f); return 1; }
                    const std::string why = differ(P, file, R, strips[L - 1]);
                    if (!why.empty()) {
                        std::fprintf(stderr, "FAIL: %s, limit %u, reduce %u, %s: %s\n", path.c_str(), L, reduce, windowed ? "window" : "whole", why.c_str());
                        return 1;
                    }
                    ++compared;
                    if (L < layers) cut_blocks += own.blocks.size() - P.blocks.size();
                    if (H.cblk_style == 1) // bypass: did a block end inside a raw segment (its significance pass without the refinement pass)?
                        for (const DecBlock &b : P.blocks)
                            if (b.nsegs && b.npasses > 10 && (b.npasses - 10) % 3 == 1 && (P.cwsegs[b.seg_first + b.nsegs - 1] >> 24) == 1) ++partial_raw;
                }
            }
        }
        uint32_t seed = seed0 + 131u * (uint32_t)files;
        for (int t = 0; t < 200; ++t) {
            std::vector<uint8_t> m = file;
            if (t % 4 == 0) m.resize(1 + lcg(seed) % file.size());
            else for (int k = 0; k < 1 + t % 4; ++k) m[lcg(seed) % m.size()] ^= (uint8_t)(1u << (lcg(seed) & 7));
            std::vector<uint8_t> exact(m.begin(), m.end()); // exact-size heap block: any over-read trips ASan
            try {
                const DecodePlan P = plan_decode(exact.data(), exact.size(), 0, nullptr, 1);
                if (const char *f = plan_fault(P, exact.size())) {
                    std::fprintf(stderr, "FAIL: %s (mutated %s, case %d, J2K_FUZZ_SEED=%u)\n", f, path.c_str(), t, seed0);
                    return 1;
                }
                ++mutated_ok;
            } catch (const Error &) { ++rejected; }
        }
    }
    if (!files || !cut_blocks || !partial_raw) {
        std::fprintf(stderr, "FAIL: the files prove nothing: %zu files, %zu blocks dropped by a limit, %zu blocks ending inside a raw segment\n", files, cut_blocks, partial_raw);
        return 1;
    }
    std::printf("compared %zu plans of %zu files, %zu blocks dropped, %zu blocks ending inside a raw segment, mutated ok %zu, rejected %zu\n", compared, files,
                cut_blocks, partial_raw, mutated_ok, rejected);
    return 0;
}
