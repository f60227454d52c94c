// Host-side code of the cinema colour front end (rgb_to_xyz: the tables of xyz_tables.cpp, the threshold search that defines a
// code, normalise's acceptance and refusals) under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU.  Built and run by
// tests/test_xyz_sanitize.py from xyz_tables.cpp and geometry.cpp; no HIP, no device.
#include "../../j2k_amd/csrc/common.h"
#include "../../j2k_amd/csrc/xyz_tables.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

using namespace j2k_hip;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

// the definition, counted one threshold at a time
static uint32_t count_le(const std::vector<float> &thr, float x)
{
    uint32_t n = 0;
    for (float t : thr) n += t <= x;
    return n;
}

static void tables(uint32_t source, uint32_t sd, uint32_t dd)
{
    CHECK(xyz_tables_valid(source, sd, dd));
    const std::vector<float> lin = xyz_lin_table(source, sd), thr = xyz_thr_table(dd);
    CHECK(lin.size() == (size_t)1 << sd && thr.size() == ((size_t)1 << dd) - 1);
    CHECK(lin.front() == 0.0f && lin.back() == 1.0f);
    for (size_t i = 1; i < lin.size(); ++i) CHECK(lin[i] > lin[i - 1]);
    for (size_t i = 1; i < thr.size(); ++i) CHECK(thr[i] > thr[i - 1]);
    CHECK(thr.front() > 0.0f && thr.back() < 1.0f);
    // the search over the edge values: below, at and just above every threshold near both ends and the middle, and the specials
    const uint32_t n = (uint32_t)thr.size();
    const float inf = std::numeric_limits<float>::infinity();
    for (float x : {0.0f, -0.0f, 1.0f, 2.0f, inf, std::numeric_limits<float>::denorm_min()}) CHECK(xyz_code(thr.data(), n, x) == count_le(thr, x));
    CHECK(xyz_code(thr.data(), n, 0.0f) == 0 && xyz_code(thr.data(), n, 1.0f) == n && xyz_code(thr.data(), 0, 0.5f) == 0);
    const uint32_t picks[] = {0, 1, 2, n / 2, n - 2, n - 1};
    for (uint32_t k : picks) {
        if (k >= n) continue;
        const float t = thr[k];
        CHECK(xyz_code(thr.data(), n, t) == k + 1);
        CHECK(xyz_code(thr.data(), n, std::nextafter(t, 0.0f)) == k);
        CHECK(xyz_code(thr.data(), n, std::nextafter(t, 2.0f)) == (k + 1 < n && thr[k + 1] <= std::nextafter(t, 2.0f) ? k + 2 : k + 1));
    }
    // white: every channel at its top through the matrix, as the kernel forms it
    float M[9];
    xyz_matrix(M);
    for (int i = 0; i < 3; ++i) {
        const float x = (M[3 * i] * lin.back() + M[3 * i + 1] * lin.back()) + M[3 * i + 2] * lin.back();
        CHECK(x > 0.0f && x < 1.0f && xyz_code(thr.data(), n, x) <= n);
    }
    std::printf("ok tables source %u depths %u -> %u\n", source, sd, dd);
}

static j2k_hip_params base()
{
    j2k_hip_params p = {};
    p.struct_size = sizeof(p);
    p.width = 64; p.height = 48; p.channels = 3; p.depth = 12; p.num_resolutions = 3; p.comment = "";
    return p;
}

static void refused(const j2k_hip_params &p, const char *word)
{
    try { normalise(&p); CHECK(false); }
    catch (const Error &e) { CHECK(e.code == J2K_HIP_ERR_PARAM && std::string(e.what()).find(word) != std::string::npos); }
}

int main()
{
    for (uint32_t source = 1; source <= 3; ++source)
        for (uint32_t sd : {8u, 12u, 16u})
            for (uint32_t dd : {8u, 12u, 16u}) tables(source, sd, dd);
    tables(1, 1, 1); // the smallest tables: two linear values, one threshold
    CHECK(!xyz_tables_valid(0, 8, 8) && !xyz_tables_valid(4, 8, 8) && !xyz_tables_valid(1, 0, 8) && !xyz_tables_valid(1, 17, 8) &&
          !xyz_tables_valid(1, 8, 0) && !xyz_tables_valid(1, 8, 17));
    std::printf("ok argument checks\n");

    // accepted: alone and with everything it combines with
    const float rates[2] = {20.f, 5.f}, psnr[1] = {40.f};
    for (uint32_t v = 1; v <= 3; ++v) { j2k_hip_params p = base(); p.rgb_to_xyz = v; CHECK(normalise(&p).rgb_to_xyz == v); }
    { j2k_hip_params p = base(); CHECK(normalise(&p).rgb_to_xyz == 0); }
    { j2k_hip_params p = base(); p.rgb_to_xyz = 1; p.width = 512; p.height = 270; p.dci_profile = 3; const Coding c = normalise(&p); CHECK(c.dci == 3 && c.mct && c.rgb_to_xyz == 1); }
    { j2k_hip_params p = base(); p.rgb_to_xyz = 1; p.layers = 2; p.layer_rates = rates; CHECK(normalise(&p).rate_control()); }
    { j2k_hip_params p = base(); p.rgb_to_xyz = 2; p.layer_psnr = psnr; CHECK(normalise(&p).rate_control()); }
    { j2k_hip_params p = base(); p.rgb_to_xyz = 3; p.ycc = 1; p.reversible = 1; p.cblk_style = J2K_HIP_CBLK_BYPASS; p.tile_size = 32; CHECK(normalise(&p).ntiles() == 4); }
    { j2k_hip_params p = base(); p.rgb_to_xyz = 1; p.channels = 4; p.alpha = 4; p.file_format = J2K_HIP_FMT_JP2; p.promote_ae16 = 1; CHECK(normalise(&p).jp2); }
    std::printf("ok accepted\n");

    // refused, the text naming the field; the tile-sharded entry points' refusal too
    { j2k_hip_params p = base(); p.rgb_to_xyz = 4; refused(p, "rgb_to_xyz"); }
    { j2k_hip_params p = base(); p.rgb_to_xyz = 1; p.channels = 2; refused(p, "rgb_to_xyz"); }
    { j2k_hip_params p = base(); p.rgb_to_xyz = 1; p.channels = 1; refused(p, "rgb_to_xyz"); }
    { j2k_hip_params p = base(); p.rgb_to_xyz = 1; p.rgb_to_sycc = 1; refused(p, "rgb_to_xyz"); }
    { j2k_hip_params p = base(); p.rgb_to_xyz = 1; p.comp_sub_x[1] = 2; p.comp_sub_x[2] = 2; refused(p, "rgb_to_xyz"); }
    { j2k_hip_params p = base(); p.rgb_to_xyz = 1; p.channels = 4; p.comp_sub_y[3] = 2; refused(p, "rgb_to_xyz"); }
    {
        j2k_hip_params p = base(); p.rgb_to_xyz = 1; p.tile_size = 32;
        try { refuse_subsampled_tiles(normalise(&p)); CHECK(false); }
        catch (const Error &e) { CHECK(e.code == J2K_HIP_ERR_PARAM && std::string(e.what()).find("rgb_to_xyz") != std::string::npos); }
        p.rgb_to_xyz = 0;
        refuse_subsampled_tiles(normalise(&p));
    }
    std::printf("ok refusals\n");
    return 0;
}
