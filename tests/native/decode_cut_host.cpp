// decode_cut_host.cpp -- the Tier-2 planner (decode_plan.cpp: plan_decode) on files cut short, as a stand-alone program for
// ASan / UBSan (tests/test_decode_cut_refs.py builds and runs it; no HIP, no device).
//
// The manifest named on the command line has one line per case: `id file end eoc` -- the first `end` bytes of `file`, with an
// EOC marker appended when `eoc` is 1 (tests/cut_cases.py makes the cases).  Every case is planned at reduce 0 and 1 from an
// exact-size heap copy, so that a read past the cut trips ASan.  Per case and reduce one line
//     case <id> <reduce> err <code>            the planner refused: the Error's code
//     case <id> <reduce> ok <blocks>           followed by one line per DecBlock:
//     b <tile> <comp> <res> <orient> <x> <y> <w> <h> <numbps> <npasses> <codeword bytes, hex, or -> <len:passes,... or ->
// (x, y: the block's place in its tile-component's plane) goes to stdout, where the test compares it with the oracle's list of
// the same cut.  A plan the device code could not take on trust (tests/native/decode_sanitize.cpp states what it does) ends the run.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>

#include "../../j2k_amd/csrc/decode_plan.h"

using namespace j2k_hip;

static std::vector<uint8_t> slurp(const std::string &path)
{
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

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
        if (b.nsegs && (bytes > b.cw_len || passes < b.npasses)) return "codeword segments that do not cover the block";
    }
    return nullptr;
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: decode_cut_host manifest\n"); return 2; }
    std::ifstream mf(argv[1]);
    std::string line, last_path;
    std::vector<uint8_t> file;
    size_t ncases = 0;
    while (std::getline(mf, line)) {
        std::istringstream ls(line);
        std::string id, path;
        size_t end = 0;
        int eoc = 0;
        if (!(ls >> id >> path >> end >> eoc)) continue;
        if (path != last_path) { file = slurp(path); last_path = path; }
        if (file.empty() || end > file.size()) { std::fprintf(stderr, "FAIL: %s: cannot cut %s at %zu\n", id.c_str(), path.c_str(), end); return 1; }
        std::vector<uint8_t> exact(file.begin(), file.begin() + (ptrdiff_t)end); // exact-size heap block: any over-read trips ASan
        if (eoc) { exact.push_back(0xff); exact.push_back(0xd9); }
        exact.shrink_to_fit();
        ++ncases;
        for (uint32_t reduce = 0; reduce < 2; ++reduce) {
            try {
                const DecodePlan P = plan_decode(exact.data(), exact.size(), reduce);
                if (const char *f = plan_fault(P, exact.size())) { std::fprintf(stderr, "FAIL: %s, reduce %u: %s\n", id.c_str(), reduce, f); return 1; }
                std::vector<uint8_t> arena(P.arena_bytes, 0); // the codeword arena as the gather kernel fills it
                for (const DecSeg &s : P.segs) std::memcpy(arena.data() + s.dst, exact.data() + s.src, s.len);
                std::vector<uint32_t> tile_pos(P.geo.cod.ntiles(), 0);
                for (size_t t = 0; t < P.geo.tiles.size(); ++t) tile_pos[P.geo.tiles[t].index] = (uint32_t)t;
                std::printf("case %s %u ok %zu\n", id.c_str(), reduce, P.blocks.size());
                for (const DecBlock &b : P.blocks) {
                    const Cblk &c = P.geo.cblks[b.cblk];
                    const TileComp &TC = P.geo.tiles[tile_pos[c.tile]].comps[c.comp];
                    std::printf("b %u %u %u %u %d %d %u %u %u %u ", c.tile, c.comp, c.res, (unsigned)c.orient, (int)c.px - TC.x0, (int)c.py - TC.y0, (unsigned)c.w,
                                (unsigned)c.h, b.numbps, b.npasses);
                    if (!b.cw_len) std::printf("-");
                    for (uint32_t k = 0; k < b.cw_len; ++k) std::printf("%02x", arena[b.cw_off + k]);
                    std::printf(" ");
                    if (!b.nsegs) std::printf("-");
                    for (uint32_t k = 0; k < b.nsegs; ++k)
                        std::printf("%s%u:%u", k ? "," : "", P.cwsegs[b.seg_first + k] & kCwSegMaxBytes, P.cwsegs[b.seg_first + k] >> 24);
                    std::printf("\n");
                }
            } catch (const Error &x) {
                std::printf("case %s %u err %d\n", id.c_str(), reduce, x.code);
            }
        }
    }
    if (!ncases) { std::fprintf(stderr, "FAIL: no case in the manifest\n"); return 1; }
    std::printf("done %zu\n", ncases);
    return 0;
}
