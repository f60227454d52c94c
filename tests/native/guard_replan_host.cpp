// Host Tier-2's plan, excess, re-plan path (j2k_hip_params.guard_bits = J2K_HIP_GUARD_AUTO) under
// AddressSanitizer + UndefinedBehaviorSanitizer on the CPU.  Built and run by tests/test_guard_param_host.py; no HIP, no device:
// Tier-1 results are synthesised.  Two frames: a plain one, and a tiled one where only one of the two tiles holds a block with
// more bit-planes than its band signals.  For each: a strict count refuses (the packet writer, TilePricer and the layer
// allocation alike); under auto the plan at the floor ends in GuardExcess, guard_bits_needed finds the count, and the plan of
// with_guard_bits(geometry, count) is byte for byte the plan of a geometry built with that count fixed -- blob, segment
// tables, block destinations, length -- with the count in the QCD; so is the layer allocation.
#include "../../j2k_amd/csrc/rate_control.h"

#include <cstdio>
#include <cstdlib>

using namespace j2k_hip;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

static uint32_t lcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return s >> 8; }

static j2k_hip_params params(uint32_t w, uint32_t h, uint32_t tile, uint32_t guard_bits, const float *rates)
{
    j2k_hip_params p = {};
    p.struct_size = sizeof(p);
    p.width = w; p.height = h; p.channels = 3; p.depth = 8; p.reversible = 1; p.ycc = 1; p.num_resolutions = 2; p.tile_size = tile;
    p.comment = ""; p.guard_bits = guard_bits;
    if (rates) { p.layers = 1; p.layer_rates = rates; }
    return p;
}

// plausible results below every band's Mb (at two guard bits), then `excess` bit-planes beyond it on one block of tile `tile`
static void synth(const Geometry &g, uint32_t seed, uint32_t tile, uint32_t excess, std::vector<CblkResult> &res, std::vector<uint32_t> &rate,
                  std::vector<int32_t> &nmse)
{
    const size_t nb = g.cblks.size();
    res.assign(nb, CblkResult());
    rate.assign(nb * kMaxPasses, 0);
    nmse.assign(nb * kMaxPasses, 0);
    uint32_t s = seed;
    bool done = false;
    for (size_t i = 0; i < nb; ++i) {
        const Cblk &c = g.cblks[i];
        const uint32_t Mb2 = (uint32_t)c.Mb - g.cod.guard + 2u;
        uint32_t bps = 1 + lcg(s) % Mb2;
        if (!done && c.tile == tile && c.comp == 1) { bps = Mb2 + excess; done = true; }
        res[i].numbps = bps;
        res[i].npasses = 3 * bps - 2;
        uint32_t acc = 0;
        for (uint32_t k = 0; k < res[i].npasses; ++k) {
            acc += 1 + lcg(s) % (1 + (uint32_t)c.w * c.h / 16);
            rate[i * kMaxPasses + k] = acc;
            nmse[i * kMaxPasses + k] = (int32_t)(lcg(s) % 100000);
        }
        res[i].len = acc;
    }
    CHECK(done);
}

static bool same_plan(const Tier2Plan &a, const Tier2Plan &b)
{
    if (a.blob != b.blob || a.total_len != b.total_len || a.cblk_dst != b.cblk_dst) return false;
    if (a.hdr_segs.size() != b.hdr_segs.size() || a.body_segs.size() != b.body_segs.size()) return false;
    for (size_t i = 0; i < a.hdr_segs.size(); ++i)
        if (a.hdr_segs[i].dst != b.hdr_segs[i].dst || a.hdr_segs[i].src != b.hdr_segs[i].src || a.hdr_segs[i].len != b.hdr_segs[i].len) return false;
    for (size_t i = 0; i < a.body_segs.size(); ++i)
        if (a.body_segs[i].dst != b.body_segs[i].dst || a.body_segs[i].cblk != b.body_segs[i].cblk || a.body_segs[i].off != b.body_segs[i].off ||
            a.body_segs[i].len != b.body_segs[i].len) return false;
    return true;
}

static unsigned sqcd(const std::vector<uint8_t> &blob)
{
    for (size_t q = 2; q + 4 < blob.size(); q += 2 + (((size_t)blob[q + 2] << 8) | blob[q + 3]))
        if (blob[q] == 0xff && blob[q + 1] == 0x5c) return blob[q + 4];
    return ~0u;
}

template <typename F> static bool exceeds(F &&f)
{
    try { f(); } catch (const GuardExcess &x) { return x.code == J2K_HIP_ERR_OVERFLOW; }
    return false;
}

static void frame_case(const char *name, uint32_t w, uint32_t h, uint32_t tile, uint32_t bad_tile)
{
    static const float rates[1] = {3.0f};
    for (int rc = 0; rc < 2; ++rc) {
        const float *r = rc ? rates : nullptr;
        const j2k_hip_params pa = params(w, h, tile, J2K_HIP_GUARD_AUTO, r), p0 = params(w, h, tile, 0, r), p3 = params(w, h, tile, 3, r);
        const Coding ca = normalise(&pa), c0 = normalise(&p0), c3 = normalise(&p3);
        CHECK(ca.guard_auto && ca.guard == 2 && !c0.guard_auto && c0.guard == 2 && !c3.guard_auto && c3.guard == 3);
        const Geometry ga = build_geometry(ca, 0, ca.ntiles()), g3 = build_geometry(c3, 0, c3.ntiles());
        std::vector<CblkResult> res;
        std::vector<uint32_t> rate;
        std::vector<int32_t> nmse;
        synth(ga, 77u + w, bad_tile, 1, res, rate, nmse);
        const size_t lead = main_header(ca).size();
        auto plan = [&](const Geometry &g) {
            if (!rc) return plan_codestream(g, res, true, true);
            const LayerAlloc al = allocate_layers(g, res, rate.data(), nmse.data(), lead, 2);
            return plan_codestream(g, res, true, true, &al);
        };
        // the floor refuses: the packet writer (or, with a byte budget, the allocation's pricer) and TilePricer on the tile that holds the block
        CHECK(exceeds([&] { (void)plan(ga); }));
        for (const Tile &T : ga.tiles) CHECK(exceeds([&] { TilePricer tp(ga, T, res); }) == (T.index == bad_tile));
        // the count, the re-plan, and the same results planned at that count from the start
        CHECK(guard_bits_needed(ga, res) == 3);
        const Geometry gr = with_guard_bits(ga, 3);
        CHECK(gr.cod.guard == 3 && gr.max_Mb == g3.max_Mb && gr.cblks.size() == g3.cblks.size());
        for (size_t i = 0; i < gr.cblks.size(); ++i) CHECK(gr.cblks[i].Mb == g3.cblks[i].Mb && gr.cblks[i].Mb == ga.cblks[i].Mb + 1);
        const Tier2Plan pr = plan(gr), pf = plan(g3);
        CHECK(same_plan(pr, pf));
        CHECK(sqcd(pr.blob) == (3u << 5));
        for (const Tile &T : gr.tiles) { TilePricer tp(gr, T, res); CHECK(tp.committed() == 0); }
        CHECK(guard_bits_needed(gr, res) == 3 && guard_bits_needed(g3, res) == 3);
        // two bit-planes beyond: four guard bits; far beyond: no count holds it
        std::vector<CblkResult> r2 = res;
        for (size_t i = 0; i < r2.size(); ++i) if (r2[i].numbps > ga.cblks[i].Mb) r2[i].numbps += 1;
        CHECK(guard_bits_needed(ga, r2) == 4);
        for (size_t i = 0; i < r2.size(); ++i) if (r2[i].numbps > ga.cblks[i].Mb) r2[i].numbps += 5;
        CHECK(exceeds([&] { (void)guard_bits_needed(ga, r2); }));
        // results in range: the floor, and the plan of auto is the plan of 0
        std::vector<CblkResult> ok = res;
        for (size_t i = 0; i < ok.size(); ++i) ok[i].numbps = std::min<uint32_t>(ok[i].numbps, ga.cblks[i].Mb);
        CHECK(guard_bits_needed(ga, ok) == 2);
        if (!rc) CHECK(same_plan(plan_codestream(ga, ok, true, true), plan_codestream(build_geometry(c0, 0, c0.ntiles()), ok, true, true)));
        std::printf("ok %s%s\n", name, rc ? " under a byte budget" : "");
    }
}

int main()
{
    frame_case("plain frame", 64, 64, 0, 0);
    frame_case("two tiles, one exceeds", 128, 64, 64, 1);
    return 0;
}
