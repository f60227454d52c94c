// Layers at given slope thresholds (j2k_hip_params.layer_slopes) on the host, as a stand-alone program under the address and
// undefined-behaviour sanitizers (tests/test_slopes_host.py builds and runs it; no HIP, no device).
//
// Without arguments: read-back and replay.  On synthetic Tier-1 tables -- empty blocks, byte-less runs, blocks without one
// byte, tables that step backwards -- of frames of 1 to several thousand blocks, in one tile and in several, for 1, 3 and 100
// layers, the plain procedure (allocate_layers_plain: OpenJPEG's bisection with nothing left out) lays the layers out and
// reports the thresholds it ended at; the slopes allocation at those thresholds must be the same allocation.  One tile:
// allocate_layers_slopes, the encoder's host path.  Several tiles end at thresholds of their own: the per-block routine
// (rate_block_layers) tile by tile with each tile's thresholds, then layers_from_counts, the encoder's device path behind the
// kernel.  The product bisection (allocate_layers) must report the plain procedure's thresholds.
//
// With a case file (tests/slopes_model.py writes it): the per-block routine on the file's tables for every threshold list of
// the file, one line per list and block: "P <list> <block> <passes per layer ...> | <bytes per layer ...>".
#include "../../j2k_amd/csrc/rate_block.h"
#include "../../j2k_amd/csrc/rate_control.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace j2k_hip;

static uint32_t lcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return s >> 8; }

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

// synthetic Tier-1 results (the families of host_sanitize.cpp); spoil: every ninth block has a byte count that steps backwards
// or a negative distortion sum
static void synth_tables(const Geometry &g, uint32_t seed, bool spoil, std::vector<CblkResult> &res, std::vector<uint32_t> &rate, std::vector<int32_t> &nmse)
{
    const size_t nb = g.cblks.size();
    res.assign(nb, CblkResult());
    rate.assign(nb * kMaxPasses, 0);
    nmse.assign(nb * kMaxPasses, 0);
    uint32_t s = seed;
    for (size_t i = 0; i < nb; ++i) {
        const Cblk &c = g.cblks[i];
        const uint32_t bps = i % 7 == 3 ? c.Mb : lcg(s) % (c.Mb + 1u);
        res[i].numbps = bps;
        res[i].npasses = bps ? 3 * bps - 2 : 0;
        uint32_t acc = 0;
        for (uint32_t k = 0; k < res[i].npasses; ++k) {
            const uint32_t more = lcg(s) % (1 + (uint32_t)c.w * c.h / 8);
            if (!(i % 11 == 5 || (i % 5 == 2 && k % 8 < 5))) acc += more;
            rate[i * kMaxPasses + k] = acc;
            nmse[i * kMaxPasses + k] = (int32_t)(lcg(s) % 100000);
        }
        if (spoil && i % 9 == 4 && res[i].npasses >= 3) {
            const uint32_t k = 1 + lcg(s) % (res[i].npasses - 1);
            if (i % 2 == 0 && rate[i * kMaxPasses + k - 1] > 0) rate[i * kMaxPasses + k] = rate[i * kMaxPasses + k - 1] - 1;
            else nmse[i * kMaxPasses + k] = -(int32_t)(1 + lcg(s) % 5000);
        }
        res[i].len = res[i].npasses ? acc : 0;
    }
}

static bool same(const LayerAlloc &a, const LayerAlloc &b) { return a.layers == b.layers && a.np == b.np && a.len == b.len && a.off == b.off; }

static void replay_case(uint32_t w, uint32_t h, uint32_t nc, bool rev, uint32_t numres, uint32_t tile, uint32_t cb, std::vector<float> targets, bool psnr,
                        bool spoil, uint32_t seed)
{
    j2k_hip_params p = {};
    p.struct_size = sizeof(p);
    p.width = w; p.height = h; p.channels = nc; p.depth = 8; p.reversible = rev; p.ycc = nc >= 3;
    p.num_resolutions = numres; p.tile_size = tile; p.cblk_w = cb; p.cblk_h = cb;
    p.layers = (uint32_t)targets.size();
    if (psnr) p.layer_psnr = targets.data();
    else p.layer_rates = targets.data();
    p.comment = "sanitize";
    const Coding cod = normalise(&p);
    const Geometry g = build_geometry(cod, 0, cod.ntiles());
    const size_t nb = g.cblks.size(), nt = g.tiles.size();
    const uint32_t L = cod.layers;
    CHECK(nb > 0 && cod.rate_control());
    std::vector<CblkResult> res;
    std::vector<uint32_t> rate;
    std::vector<int32_t> nmse;
    synth_tables(g, seed, spoil, res, rate, nmse);
    const size_t lead = main_header(cod).size();
    const LayerAlloc want = allocate_layers_plain(g, res, rate.data(), nmse.data(), lead);
    CHECK(want.slopes.size() == nt * L);
    size_t positive = 0;
    for (double v : want.slopes) { CHECK(std::isfinite(v)); positive += v > 0; }
    if (!spoil) { // the product bisection ends where the plain one ends (on tables it is claimed for)
        const LayerAlloc fast = allocate_layers(g, res, rate.data(), nmse.data(), lead);
        CHECK(same(fast, want) && fast.slopes == want.slopes);
    }
    // the same frame under layer_slopes: the parameters name the thresholds, nothing else differs
    j2k_hip_params q = p;
    q.layer_rates = nullptr; q.layer_psnr = nullptr;
    q.layer_slopes = want.slopes.data(); // (the first tile's)
    const Coding cod2 = normalise(&q);
    CHECK(cod2.rate_control() && cod2.slopes.size() == L && main_header(cod2) == main_header(cod));
    const Geometry g2 = build_geometry(cod2, 0, cod2.ntiles());
    const std::vector<double> weight = rate_block_weights(g2);
    if (nt == 1) {
        const LayerAlloc got = allocate_layers_slopes(g2, res, rate.data(), nmse.data(), cod2.slopes.data());
        CHECK(same(got, want) && got.slopes == want.slopes);
    }
    // tile by tile with each tile's thresholds: the per-block routine, then the allocation of its counts
    std::vector<uint8_t> passes(nb * L);
    std::vector<uint32_t> bytes(nb * L);
    for (size_t t = 0; t < nt; ++t) {
        const Tile &T = g2.tiles[t];
        for (size_t id = T.first_cblk; id < (size_t)T.first_cblk + T.num_cblks; ++id)
            rate_block_layers(weight[id], res[id].numbps, res[id].npasses, rate.data() + id * kMaxPasses, nmse.data() + id * kMaxPasses,
                              want.slopes.data() + t * L, L, passes.data() + id * L, bytes.data() + id * L);
    }
    const LayerAlloc got = layers_from_counts(g2, passes.data(), bytes.data(), want.slopes.data());
    CHECK(same(got, want));
    for (size_t id = 0; id < nb; ++id) // pass counts are cumulative and never pass the block's
        for (uint32_t l = 0; l < L; ++l) CHECK(passes[id * L + l] <= res[id].npasses && (!l || passes[id * L + l] >= passes[id * L + l - 1]));
    std::printf("ok replay %ux%u c%u %s res%u tile%u cb%u layers%u %s%s: %zu blocks in %zu tiles, %zu of %zu thresholds positive\n", w, h, nc, rev ? "5/3" : "9/7",
                numres, tile, cb, L, psnr ? "psnr" : "rates", spoil ? " spoiled" : "", nb, nt, positive, want.slopes.size());
}

static int file_case(const char *path)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 2; }
    auto rd = [&](void *dst, size_t n) { if (n && std::fread(dst, 1, n, f) != n) { std::fprintf(stderr, "short case file\n"); std::exit(2); } };
    char magic[4];
    uint32_t n = 0;
    rd(magic, 4); rd(&n, 4);
    if (std::memcmp(magic, "RLH1", 4) != 0) { std::fprintf(stderr, "not a case file\n"); return 2; }
    std::vector<double> weight(n);
    std::vector<uint32_t> numbps(n), np(n), rate((size_t)n * kRatePasses, 0);
    std::vector<int32_t> dist((size_t)n * kRatePasses, 0);
    for (uint32_t b = 0; b < n; ++b) {
        rd(&weight[b], 8); rd(&numbps[b], 4); rd(&np[b], 4);
        if (np[b] > (uint32_t)kRatePasses) { std::fprintf(stderr, "too many passes\n"); return 2; }
        rd(&rate[(size_t)b * kRatePasses], 4 * np[b]); rd(&dist[(size_t)b * kRatePasses], 4 * np[b]);
    }
    uint32_t nlists = 0;
    rd(&nlists, 4);
    for (uint32_t k = 0; k < nlists; ++k) {
        uint32_t L = 0;
        rd(&L, 4);
        std::vector<double> slopes(L);
        rd(slopes.data(), 8 * (size_t)L);
        std::vector<uint8_t> passes(L);
        std::vector<uint32_t> bytes(L);
        for (uint32_t b = 0; b < n; ++b) {
            rate_block_layers(weight[b], numbps[b], np[b], &rate[(size_t)b * kRatePasses], &dist[(size_t)b * kRatePasses], slopes.data(), L, passes.data(), bytes.data());
            std::printf("P %u %u", k, b);
            for (uint32_t l = 0; l < L; ++l) std::printf(" %u", passes[l]);
            std::printf(" |");
            for (uint32_t l = 0; l < L; ++l) std::printf(" %u", bytes[l]);
            std::printf("\n");
        }
    }
    std::fclose(f);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1) return file_case(argv[1]);
    std::vector<float> hundred(100);
    for (int i = 0; i < 100; ++i) hundred[(size_t)i] = 400.0f - 3.9f * (float)i; // strictly decreasing ratios, the last 13.9
    // one block; a few; hundreds; several thousand -- one tile
    replay_case(8, 8, 1, true, 1, 0, 8, {4}, false, false, 1);
    replay_case(8, 8, 1, true, 1, 0, 8, {8, 4, 1}, false, false, 2);
    replay_case(64, 64, 1, true, 3, 0, 16, {20}, false, false, 3);
    replay_case(64, 64, 1, false, 3, 0, 16, {40, 20, 5}, false, false, 4);
    replay_case(64, 64, 3, true, 3, 0, 16, hundred, false, false, 5);
    replay_case(64, 64, 1, false, 3, 0, 16, hundred, false, true, 6);
    replay_case(200, 150, 3, false, 4, 0, 32, {50, 20, 1}, false, false, 7);
    replay_case(200, 150, 3, true, 4, 0, 32, {50, 20, 8}, false, true, 8);
    replay_case(256, 256, 1, false, 4, 0, 8, {30, 10, 4}, false, false, 9);
    replay_case(256, 256, 3, true, 4, 0, 8, {12}, false, true, 10);
    // fixed quality: the other bisection's thresholds
    replay_case(128, 128, 1, false, 4, 0, 32, {25, 32, 40}, true, false, 11);
    replay_case(128, 128, 3, true, 4, 0, 16, {30, 0}, true, false, 12);
    // several tiles, each ending at thresholds of its own
    replay_case(300, 200, 3, false, 4, 128, 32, {50, 25}, false, false, 13);
    replay_case(256, 256, 1, true, 4, 64, 8, {30, 10, 4}, false, true, 14);
    replay_case(128, 128, 1, false, 3, 64, 16, hundred, false, false, 15);
    replay_case(192, 192, 1, false, 3, 64, 16, {28, 36}, true, false, 16);
    return 0;
}
