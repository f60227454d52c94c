// region_sanitize.cpp -- the window planner of a region decode (decode_plan.cpp: region_footprints, plan_decode with a
// window) as a stand-alone program for ASan / UBSan (tests/test_region_footprint.py builds and runs it; no device).
//
// For every file on the command line, at reduce 0 .. 2, for a set of windows: the plan must succeed, keep no more blocks
// than the plan of the whole image, keep exactly those for the whole-image window, and every footprint must lie inside
// its resolution and its bands -- what the windowed inverse DWT's jobs index the planes with.  Windows that leave the
// image must be refused with J2K_HIP_ERR_PARAM.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>

#include "../../j2k_amd/csrc/decode_plan.h"

using namespace j2k_hip;

static int fail(const std::string &m)
{
    std::fprintf(stderr, "FAIL: %s\n", m.c_str());
    return 1;
}

static bool inside(const IRect &a, int x0, int y0, int x1, int y1) { return a.empty() || (a.x0 >= x0 && a.y0 >= y0 && a.x1 <= x1 && a.y1 <= y1); }

int main(int argc, char **argv)
{
    size_t plans = 0;
    for (int i = 1; i < argc; ++i) {
        std::ifstream f(argv[i], std::ios::binary);
        std::vector<uint8_t> d((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        if (d.empty()) return fail(std::string("cannot read ") + argv[i]);
        FileHeader H;
        try { H = parse_headers(d.data(), d.size()); } catch (const Error &) { continue; } // (files this reader hands to the fallback)
        for (uint32_t reduce = 0; reduce < 3 && reduce < H.cod.numres; ++reduce) {
            int ow, oh;
            reduced_size(H.cod, reduce, ow, oh);
            if (ow <= 0 || oh <= 0) continue;
            const DecodePlan full = plan_decode(d.data(), d.size(), reduce);
            const uint32_t W = (uint32_t)ow, Hh = (uint32_t)oh;
            const uint32_t wins[][4] = {{0, 0, 1, 1}, {W - 1, Hh - 1, 1, 1}, {W / 3, Hh / 3, (W + 2) / 3, (Hh + 2) / 3}, {W / 2, 0, 1, Hh},
                                        {0, Hh - 1, W, 1}, {0, 0, W, Hh}};
            for (const auto &w : wins) {
                const DecodePlan P = plan_decode(d.data(), d.size(), reduce, w);
                ++plans;
                if (!P.windowed || P.windows.size() != P.geo.tiles.size() * 4) return fail("no windows in a windowed plan");
                if (P.blocks.size() > full.blocks.size()) return fail("a window keeps more blocks than the image has");
                if (w[2] == W && w[3] == Hh && (P.blocks.size() != full.blocks.size() || P.arena_bytes != full.arena_bytes))
                    return fail(std::string("the whole-image window drops blocks: ") + argv[i]);
                const uint32_t top = H.cod.numres - 1 - reduce;
                for (size_t t = 0; t < P.geo.tiles.size(); ++t)
                    for (uint32_t c = 0; c < H.cod.ncomp_out(); ++c) {
                        const std::vector<ResFootprint> &fp = P.windows[t * 4 + c];
                        if (fp.empty()) continue;
                        if (fp.size() != top + 1 || fp[top].win.empty()) return fail("footprints of the wrong depth");
                        const TileComp &TC = P.geo.tiles[t].comps[c];
                        for (uint32_t r = 0; r <= top; ++r) {
                            const Resolution &R = TC.res[r];
                            if (!inside(fp[r].win, R.x0, R.y0, R.x1, R.y1)) return fail("window outside its resolution");
                            if (r == 0 || fp[r].win.empty()) continue;
                            for (int b = 0; b < 3; ++b)
                                if (!inside(fp[r].band[b], R.bands[b].x0, R.bands[b].y0, R.bands[b].x1, R.bands[b].y1)) return fail("footprint outside its band");
                            // the rows the horizontal pass produces: inside the low (HL's rows) and high (LH's rows) halves
                            if (fp[r].ly1 > fp[r].ly0 && (fp[r].ly0 < R.bands[0].y0 || fp[r].ly1 > R.bands[0].y1)) return fail("low rows outside the band");
                            if (fp[r].hy1 > fp[r].hy0 && (fp[r].hy0 < R.bands[1].y0 || fp[r].hy1 > R.bands[1].y1)) return fail("high rows outside the band");
                            if (fp[r].ly1 - fp[r].ly0 + fp[r].hy1 - fp[r].hy0 <= 0) return fail("a window that reads no row");
                            if (!inside(fp[r - 1].win, TC.res[r - 1].x0, TC.res[r - 1].y0, TC.res[r - 1].x1, TC.res[r - 1].y1)) return fail("LL need outside the lower resolution");
                        }
                    }
            }
            const uint32_t bad[][4] = {{0, 0, 0, 1}, {0, 0, 1, 0}, {W, 0, 1, 1}, {0, Hh, 1, 1}, {1, 1, W, Hh}, {0xffffffffu, 0, 2, 1}};
            for (const auto &w : bad) {
                try {
                    (void)plan_decode(d.data(), d.size(), reduce, w);
                    return fail("a window outside the image was planned");
                } catch (const Error &e) {
                    if (e.code != J2K_HIP_ERR_PARAM || std::string(e.what()).find("region") == std::string::npos) return fail("wrong refusal of a window");
                }
            }
        }
    }
    std::printf("planned %zu windows\n", plans);
    return plans ? 0 : 1;
}
