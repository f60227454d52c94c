// Host-side logic of the sub-sampled write side (normalise, the partition on the components' own grids, the packet orders,
// SIZ, the layer allocation and the Tier-2 planner over components of unlike sizes) under AddressSanitizer +
// UndefinedBehaviorSanitizer on the CPU.  Built and run by tests/test_subsample_sanitize.py; no HIP, no device: Tier-1
// results are synthesised, as in host_sanitize.cpp.
#include "../../j2k_amd/csrc/rate_control.h"
#include "../../j2k_amd/csrc/jp2.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

using namespace j2k_hip;

static uint32_t lcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return s >> 8; }

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

static void one_case(uint32_t w, uint32_t h, uint32_t nc, const uint32_t (*sub)[2], uint32_t numres, uint32_t tile, uint32_t prog,
                     std::vector<float> rates, bool sycc, uint32_t seed)
{
    j2k_hip_params p = {};
    p.struct_size = sizeof(p);
    p.width = w; p.height = h; p.channels = nc; p.depth = 8; p.reversible = rates.empty();
    p.num_resolutions = numres; p.tile_size = tile; p.progression = prog; p.comment = "";
    p.layers = rates.empty() ? 1 : (uint32_t)rates.size();
    p.layer_rates = rates.empty() ? nullptr : rates.data();
    for (uint32_t c = 0; c < nc; ++c) { p.comp_sub_x[c] = sub[c][0]; p.comp_sub_y[c] = sub[c][1]; }
    p.rgb_to_sycc = sycc;
    if (sycc) { p.file_format = J2K_HIP_FMT_JP2; p.color_space = J2K_HIP_CS_SYCC; p.alpha = nc == 4 ? 4 : 0; }
    const Coding cod = normalise(&p);
    CHECK(cod.subsampled() && cod.rgb_to_sycc == sycc);
    for (uint32_t c = 0; c < nc; ++c) CHECK(cod.cdx[c] == sub[c][0] && cod.cdy[c] == sub[c][1]);
    const std::vector<uint8_t> mh = main_header(cod);
    for (uint32_t c = 0; c < nc; ++c) CHECK(mh[42 + 3 * c] == 7 && mh[43 + 3 * c] == sub[c][0] && mh[44 + 3 * c] == sub[c][1]); // Ssiz, XRsiz, YRsiz
    const Geometry g = build_geometry(cod, 0, cod.ntiles());
    const size_t nb = g.cblks.size();
    CHECK(nb > 0);
    // every packet of every tile once, whatever the progression; every block inside its component's own plane
    for (const Tile &T : g.tiles) {
        size_t want = 0;
        for (const TileComp &TC : T.comps) for (const Resolution &R : TC.res) want += (size_t)R.pw * R.ph * cod.layers;
        CHECK(packet_order(cod, T, cod.layers).size() == want);
    }
    for (const Cblk &c : g.cblks) {
        const uint32_t cw = (w + sub[c.comp][0] - 1) / sub[c.comp][0], ch = (h + sub[c.comp][1] - 1) / sub[c.comp][1];
        CHECK(c.w > 0 && c.h > 0 && c.px + c.w <= cw && c.py + c.h <= ch);
    }
    // synthetic Tier-1 results, then the allocation (fast path against the plain procedure) and the planner
    std::vector<CblkResult> res(nb);
    std::vector<uint32_t> rate(nb * kMaxPasses, 0);
    std::vector<int32_t> nmse(nb * kMaxPasses, 0);
    uint32_t s = seed;
    for (size_t i = 0; i < nb; ++i) {
        const Cblk &c = g.cblks[i];
        const uint32_t bps = lcg(s) % (c.Mb + 1u);
        res[i].numbps = bps;
        res[i].npasses = bps ? 3 * bps - 2 : 0;
        uint32_t acc = 0;
        for (uint32_t k = 0; k < res[i].npasses; ++k) {
            acc += lcg(s) % (1 + (uint32_t)c.w * c.h / 8);
            rate[i * kMaxPasses + k] = acc;
            nmse[i * kMaxPasses + k] = (int32_t)(lcg(s) % 100000);
        }
        res[i].len = res[i].npasses ? acc : 0;
    }
    LayerAlloc al;
    const bool rc = cod.rate_control();
    const size_t lead = mh.size() + jp2_file_header(cod, 0).size();
    if (rc) {
        al = allocate_layers(g, res, rate.data(), nmse.data(), lead);
        const LayerAlloc want = allocate_layers_plain(g, res, rate.data(), nmse.data(), lead);
        CHECK(al.layers == want.layers && al.np == want.np && al.len == want.len && al.off == want.off);
    }
    const Tier2Plan plan = plan_codestream(g, res, true, true, rc ? &al : nullptr);
    // the pieces tile the output exactly: no gap, no overlap
    std::vector<std::pair<uint64_t, uint64_t>> iv;
    for (const HeaderSeg &hs : plan.hdr_segs) { CHECK((size_t)hs.src + hs.len <= plan.blob.size()); iv.push_back({hs.dst, hs.len}); }
    if (rc) for (const BodySeg &b : plan.body_segs) { CHECK(b.cblk < nb && b.off + b.len <= res[b.cblk].len); iv.push_back({b.dst, b.len}); }
    else for (size_t i = 0; i < nb; ++i) if (res[i].len) iv.push_back({plan.cblk_dst[i], res[i].len});
    std::sort(iv.begin(), iv.end());
    uint64_t pos = 0;
    for (auto &x : iv) { if (!x.second) continue; CHECK(x.first == pos); pos += x.second; }
    CHECK(pos == plan.total_len);
    std::printf("ok %ux%u nc %u prog %u tile %u blocks %zu bytes %llu\n", w, h, nc, prog, tile, nb, (unsigned long long)plan.total_len);
}

static void refused(const j2k_hip_params &p, const char *word)
{
    try { normalise(&p); CHECK(false); }
    catch (const Error &e) { CHECK(e.code == J2K_HIP_ERR_PARAM && std::string(e.what()).find(word) != std::string::npos); }
}

int main()
{
    static const uint32_t s422[4][2] = {{1, 1}, {2, 1}, {2, 1}, {1, 1}}, s420[4][2] = {{1, 1}, {2, 2}, {2, 2}, {1, 1}};
    static const uint32_t s411[4][2] = {{1, 1}, {4, 1}, {4, 1}, {1, 1}}, mixed[4][2] = {{1, 1}, {2, 1}, {1, 2}, {4, 4}};
    for (uint32_t prog = J2K_HIP_LRCP; prog <= J2K_HIP_CPRL; ++prog) {
        one_case(150, 131, 3, s411, 3, 50, prog, {}, false, 1 + prog);       // tiles that are no multiple of the factor
        one_case(131, 67, 4, s420, 3, 0, prog, {}, true, 11 + prog);         // alpha behind sub-sampled chroma, JP2 sYCC
        one_case(200, 150, 3, s420, 4, 128, prog, {80.f, 30.f, 12.f}, false, 21 + prog); // byte budgets over unlike components
        one_case(130, 70, 4, mixed, 3, 64, prog, {30.f, 0.f}, false, 31 + prog);
    }
    one_case(1, 1, 3, s420, 1, 0, J2K_HIP_RPCL, {}, true, 41);               // one sample in every plane
    one_case(3, 3, 3, s420, 1, 0, J2K_HIP_PCRL, {}, false, 42);
    one_case(1, 37, 3, s422, 1, 0, J2K_HIP_CPRL, {}, true, 43);
    one_case(17, 9, 3, s420, 2, 0, J2K_HIP_LRCP, {}, false, 44);             // a chroma plane narrower than a code-block
    // what is refused, each naming its field
    j2k_hip_params b = {};
    b.struct_size = sizeof(b); b.width = 64; b.height = 64; b.channels = 3; b.depth = 8; b.num_resolutions = 3;
    j2k_hip_params q = b; q.comp_sub_x[1] = 3; refused(q, "comp_sub");
    q = b; q.comp_sub_x[0] = 2; refused(q, "component 0");
    q = b; q.comp_sub_x[1] = 2; q.ycc = 1; refused(q, "ycc");
    q = b; q.rgb_to_sycc = 1; q.ycc = 1; refused(q, "rgb_to_sycc");
    q = b; q.rgb_to_sycc = 1; q.comp_sub_x[1] = 4; q.comp_sub_x[2] = 4; refused(q, "rgb_to_sycc");
    q = b; q.rgb_to_sycc = 1; q.channels = 2; refused(q, "rgb_to_sycc");
    const float psnr[1] = {35.f};
    q = b; q.comp_sub_y[2] = 2; q.layer_psnr = psnr; refused(q, "layer_psnr");
    std::printf("ok refusals\n");
    return 0;
}
