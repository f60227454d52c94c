// rgba_sanitize.cpp -- the host side of the fused RGBA output stage (rgba_plan.cpp: classify_rgba, check_rgba_dst,
// decode_rgba_args) as a stand-alone program for ASan / UBSan (tests/test_rgba_host.py builds and runs it; no device).
//
// Arguments: files whose expected mode follows each as a number (J2K_HIP_RGBA_*, 0 = J2K_HIP_ERR_UNSUPPORTED, -1 = whatever
// parse_headers says).  Then, without any file: the packed form is chosen for every permutation of the four bases of a
// record and for nothing else (misaligned record, unequal strides, unequal extents, a stride that is no multiple of the
// record, no alpha); every refusal of the destination and of the class.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>

#include "../../j2k_amd/csrc/decode_plan.h"
#include "../../j2k_amd/csrc/rgba_plan.h"

using namespace j2k_hip;

static int fail(const std::string &m)
{
    std::fprintf(stderr, "FAIL: %s\n", m.c_str());
    return 1;
}

static j2k_hip_outplane plane(uintptr_t base, int sb, long long col, long long row, uint32_t depth, uint32_t w, uint32_t h)
{
    j2k_hip_outplane p{};
    p.base = reinterpret_cast<void *>(base); p.colbytes = (ptrdiff_t)col; p.rowbytes = (ptrdiff_t)row;
    p.sample_bits = 8u * (uint32_t)sb; p.depth = depth; p.width = w; p.height = h;
    return p;
}

// the four channels of a record at `p`, sample order perm (perm[c] = slot of R, G, B, A)
static j2k_hip_rgba_dst record(uintptr_t p, const int perm[4], int sb, long long row, uint32_t w = 37, uint32_t h = 21)
{
    j2k_hip_rgba_dst d{};
    d.struct_size = sizeof(d);
    j2k_hip_outplane *ch[4] = {&d.r, &d.g, &d.b, &d.a};
    for (int c = 0; c < 4; ++c) *ch[c] = plane(p + (uintptr_t)(perm[c] * sb), sb, 4 * sb, row, 8u * (uint32_t)sb, w, h);
    return d;
}

template <typename F> static bool refused(int code, F &&f)
{
    try { f(); } catch (const Error &e) { return e.code == code; }
    return false;
}

int main(int argc, char **argv)
{
    // ---- the classifier over the files given
    int nfiles = 0;
    for (int i = 1; i + 1 < argc; i += 2) {
        std::ifstream f(argv[i], std::ios::binary);
        std::vector<uint8_t> d((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        if (d.empty()) return fail(std::string("cannot read ") + argv[i]);
        const int want = std::atoi(argv[i + 1]);
        int got = -1;
        std::string text;
        try {
            const FileHeader H = parse_headers(d.data(), d.size());
            try { got = (int)classify_rgba(H).mode; } catch (const Error &e) { if (e.code != J2K_HIP_ERR_UNSUPPORTED) return fail("wrong refusal by the classifier"); got = 0; text = e.what(); }
        } catch (const Error &) { got = -1; }
        if (got != want) return fail(std::string(argv[i]) + ": mode " + std::to_string(got) + ", expected " + std::to_string(want) + " " + text);
        if (got == 0 && text.find("colour space") == std::string::npos) return fail("the refusal does not name the colour space: " + text);
        // truncated headers: refused by the parser or classified, never read past the end (the sanitizer's to see)
        for (size_t cut : {d.size() / 2, (size_t)40, (size_t)90, (size_t)3}) {
            if (cut >= d.size()) continue;
            std::vector<uint8_t> t(d.begin(), d.begin() + (ptrdiff_t)cut);
            try { (void)classify_rgba(parse_headers(t.data(), t.size())); } catch (const Error &) {}
        }
        ++nfiles;
    }

    // ---- the arguments' filler
    const RgbaComp comps[4] = {{nullptr, 8, 1, 1}, {nullptr, 8, 2, 2}, {nullptr, 8, 2, 2}, {nullptr, 8, 1, 1}};
    const RgbaClass rgb4 = rgba_class(J2K_HIP_RGBA_RGB, 4), ycc = rgba_class(J2K_HIP_RGBA_SYCC, 3);
    int perm[4] = {0, 1, 2, 3}, nperm = 0;
    do {
        for (int sb = 1; sb <= 2; ++sb) {
            const uintptr_t p = 0x10000;
            const long long rec = 4 * sb;
            for (long long row : {rec * 40, -rec * 40}) {
                const DecRgbaArgs a = decode_rgba_args(true, false, 37, 21, 64, comps, ycc, record(p, perm, sb, row), true);
                if (!a.packed || a.pix != reinterpret_cast<uint8_t *>(p) || a.pix_rowbytes != row) return fail("a record was not recognised");
                for (int c = 0; c < 4; ++c) if (a.slot[c] != perm[c]) return fail("wrong slot");
                if (a.dst_w[0] != 37 || a.dst_h[0] != 21 || a.sample_bytes != sb || a.ncomp != 3 || a.alpha_comp != -1) return fail("wrong geometry");
            }
            // one sample off: the same samples, the general form
            if (decode_rgba_args(true, false, 37, 21, 64, comps, ycc, record(p + (uintptr_t)sb, perm, sb, rec * 40), true).packed) return fail("a misaligned record was packed");
            if (decode_rgba_args(true, false, 37, 21, 64, comps, ycc, record(p, perm, sb, rec * 40 + sb), true).packed) return fail("a stride that is no multiple of the record was packed");
            if (decode_rgba_args(true, false, 37, 21, 64, comps, ycc, record(p, perm, sb, rec * 40), false).packed) return fail("three channels were packed");
            j2k_hip_rgba_dst d = record(p, perm, sb, rec * 40);
            d.g.rowbytes += rec;
            if (decode_rgba_args(true, false, 37, 21, 64, comps, ycc, d, true).packed) return fail("unequal strides were packed");
            d = record(p, perm, sb, rec * 40);
            d.b.width = 36;
            if (decode_rgba_args(true, false, 37, 21, 64, comps, ycc, d, true).packed) return fail("unequal extents were packed");
            d = record(p, perm, sb, rec * 40);
            d.a.colbytes = 2 * rec;
            if (decode_rgba_args(true, false, 37, 21, 64, comps, ycc, d, true).packed) return fail("unequal column steps were packed");
            d = record(p, perm, sb, rec * 40);
            d.a.base = d.r.base; // two channels on one sample
            if (decode_rgba_args(true, false, 37, 21, 64, comps, ycc, d, true).packed) return fail("a sample used twice was packed");
            d = record(p, perm, sb, rec * 40);
            d.a.base = static_cast<uint8_t *>(d.a.base) + 4 * rec; // the alpha of another pixel
            if (decode_rgba_args(true, false, 37, 21, 64, comps, ycc, d, true).packed) return fail("samples of two records were packed");
            // planar
            d = record(p, perm, sb, rec * 40);
            j2k_hip_outplane *ch[4] = {&d.r, &d.g, &d.b, &d.a};
            for (int c = 0; c < 4; ++c) *ch[c] = plane(p + (uintptr_t)(c * 4096), sb, sb, 37 * sb, 8u * (uint32_t)sb, 37, 21);
            const DecRgbaArgs g = decode_rgba_args(true, false, 37, 21, 64, comps, rgb4, d, true);
            if (g.packed || g.alpha_comp != 3 || g.ncomp != 4 || g.dst[3] != reinterpret_cast<uint8_t *>(p + 3 * 4096)) return fail("planar channels");
        }
        ++nperm;
    } while (std::next_permutation(perm, perm + 4));
    if (nperm != 24) return fail("permutations");

    // ---- refusals
    const int id[4] = {1, 2, 3, 0};
    const j2k_hip_rgba_dst good = record(0x10000, id, 2, 8 * 40);
    auto args = [&](const j2k_hip_rgba_dst &d, const RgbaClass &k = rgba_class(J2K_HIP_RGBA_SYCC, 3), bool mct = false, int w = 37, int h = 21, int ox = 0, int oy = 0,
                    const RgbaComp *cp = nullptr) { (void)decode_rgba_args(true, mct, w, h, 64, cp ? cp : comps, k, d, true, ox, oy); };
    j2k_hip_rgba_dst d = good;
    d.struct_size -= 4;
    if (!refused(J2K_HIP_ERR_PARAM, [&] { args(d); })) return fail("struct_size");
    d = good; d.g.sample_bits = 8; d.g.depth = 8;
    if (!refused(J2K_HIP_ERR_PARAM, [&] { args(d); })) return fail("mixed sample_bits");
    d = good; d.a.depth = 12;
    if (!refused(J2K_HIP_ERR_PARAM, [&] { args(d); })) return fail("mixed depth");
    d = good; d.r.sample_bits = d.g.sample_bits = d.b.sample_bits = d.a.sample_bits = 12;
    if (!refused(J2K_HIP_ERR_PARAM, [&] { args(d); })) return fail("sample_bits 12");
    d = good; d.r.depth = d.g.depth = d.b.depth = d.a.depth = 17;
    if (!refused(J2K_HIP_ERR_PARAM, [&] { args(d); })) return fail("depth 17");
    d = good; d.r.depth = d.g.depth = d.b.depth = d.a.depth = 0;
    if (!refused(J2K_HIP_ERR_PARAM, [&] { args(d); })) return fail("depth 0");
    d = good; d.demote_ae16 = 1; d.r.depth = d.g.depth = d.b.depth = d.a.depth = 12;
    if (!refused(J2K_HIP_ERR_PARAM, [&] { args(d); })) return fail("demote at depth 12");
    const int id8[4] = {1, 2, 3, 0};
    d = record(0x10000, id8, 1, 4 * 40); d.demote_ae16 = 1;
    if (!refused(J2K_HIP_ERR_PARAM, [&] { args(d); })) return fail("demote with 8-bit samples");
    d = good; d.demote_ae16 = 1;
    if (refused(J2K_HIP_ERR_PARAM, [&] { args(d); })) return fail("demote at depth 16 was refused");
    if (!refused(J2K_HIP_ERR_PARAM, [&] { args(good, rgba_class(J2K_HIP_RGBA_SYCC, 3), true); })) return fail("mct on unlike components");
    if (!refused(J2K_HIP_ERR_PARAM, [&] { args(good, rgba_class(J2K_HIP_RGBA_GREY, 2), true); })) return fail("mct on two components");
    if (!refused(J2K_HIP_ERR_PARAM, [&] { args(good, rgba_class(J2K_HIP_RGBA_SYCC, 3), false, 0, 21); })) return fail("width 0");
    if (!refused(J2K_HIP_ERR_PARAM, [&] { args(good, rgba_class(J2K_HIP_RGBA_SYCC, 3), false, 37, 21, -1, 0); })) return fail("negative origin");
    const RgbaComp deep[4] = {{nullptr, 17, 1, 1}, {nullptr, 8, 1, 1}, {nullptr, 8, 1, 1}, {nullptr, 8, 1, 1}};
    if (!refused(J2K_HIP_ERR_PARAM, [&] { args(good, rgba_class(J2K_HIP_RGBA_SYCC, 3), false, 37, 21, 0, 0, deep); })) return fail("precision 17");
    const RgbaComp nosub[4] = {{nullptr, 8, 0, 1}, {nullptr, 8, 1, 1}, {nullptr, 8, 1, 1}, {nullptr, 8, 1, 1}};
    if (!refused(J2K_HIP_ERR_PARAM, [&] { args(good, rgba_class(J2K_HIP_RGBA_SYCC, 3), false, 37, 21, 0, 0, nosub); })) return fail("sub-sampling 0");
    const uint32_t bad_modes[][2] = {{0, 3}, {5, 3}, {J2K_HIP_RGBA_RGB, 2}, {J2K_HIP_RGBA_RGB, 5}, {J2K_HIP_RGBA_GREY, 3}, {J2K_HIP_RGBA_GREY, 0},
                                     {J2K_HIP_RGBA_PALETTE, 2}, {J2K_HIP_RGBA_SYCC, 2}};
    for (const auto &m : bad_modes)
        if (!refused(J2K_HIP_ERR_PARAM, [&] { (void)rgba_class(m[0], m[1]); })) return fail("a mode took components it cannot take");
    RgbaClass hand = rgba_class(J2K_HIP_RGBA_PALETTE, 1);
    hand.lut_size = 257;
    if (!refused(J2K_HIP_ERR_PARAM, [&] { args(good, hand); })) return fail("a palette of 257 entries");
    hand = rgba_class(J2K_HIP_RGBA_GREY, 1);
    hand.alpha_comp = 1;
    if (!refused(J2K_HIP_ERR_PARAM, [&] { args(good, hand); })) return fail("alpha from a component that is not read");
    // a palette's entries beyond lut_size never reach the kernel
    hand = rgba_class(J2K_HIP_RGBA_PALETTE, 1);
    hand.lut_size = 3;
    for (uint32_t &e : hand.lut) e = 0xffffffu;
    const DecRgbaArgs pa = decode_rgba_args(true, false, 37, 21, 64, comps, hand, good, true);
    for (uint32_t i = 0; i < 256; ++i) if (pa.lut[i] != (i < 3 ? 0xffffffu : 0u)) return fail("palette entries beyond lut_size");

    std::printf("classified %d files, filled the arguments for %d permutations\n", nfiles, nperm);
    return 0;
}
