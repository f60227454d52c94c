// rgba_plan.cpp -- see rgba_plan.h.  Host code only: no device is needed to classify a file or to fill the arguments.
#include "rgba_plan.h"

#include <algorithm>
#include <cstring>

#include "decode_plan.h"

namespace j2k_hip {

uint32_t cs_from_enum(uint32_t enumcs)
{
    switch (enumcs) { // reference: j2k_openjpeg_codec.cpp:318-330
    case 16: return J2K_HIP_CS_SRGB;
    case 17: return J2K_HIP_CS_GRAY;
    case 18: return J2K_HIP_CS_SYCC;
    case 24: case 19: return J2K_HIP_CS_EYCC;
    case 12: return J2K_HIP_CS_CMYK;
    default: return J2K_HIP_CS_UNSPECIFIED;
    }
}

RgbaClass rgba_class(uint32_t mode, uint32_t ncomp)
{
    RgbaClass k;
    k.mode = mode;
    switch (mode) {
    case J2K_HIP_RGBA_RGB:
        if (ncomp != 3 && ncomp != 4) throw Error(J2K_HIP_ERR_PARAM, "RGB takes 3 or 4 components");
        k.ncomp = (int)ncomp; k.alpha_comp = ncomp == 4 ? 3 : -1;
        break;
    case J2K_HIP_RGBA_GREY:
        if (ncomp != 1 && ncomp != 2) throw Error(J2K_HIP_ERR_PARAM, "grey takes 1 or 2 components");
        k.ncomp = (int)ncomp; k.alpha_comp = ncomp == 2 ? 1 : -1;
        break;
    case J2K_HIP_RGBA_PALETTE:
        if (ncomp != 1) throw Error(J2K_HIP_ERR_PARAM, "a palette takes one component of indices");
        k.ncomp = 1;
        break;
    case J2K_HIP_RGBA_SYCC:
        if (ncomp != 3 && ncomp != 4) throw Error(J2K_HIP_ERR_PARAM, "sYCC takes 3 components");
        k.ncomp = 3; // (a fourth is not read: reference j2k_rgba_file.cpp:669-713 never sets haveAlpha)
        break;
    default:
        throw Error(J2K_HIP_ERR_PARAM, "unknown RGBA mode");
    }
    return k;
}

RgbaClass classify_rgba(const FileHeader &H)
{
    const uint32_t n = H.cod.ncomp_out();
    const uint32_t cs = H.icc_len ? (uint32_t)J2K_HIP_CS_UNSPECIFIED : cs_from_enum(H.enumcs);
    uint32_t alpha = 0; // as j2k_hip_read_info reports it: k + 1 = channel k is opacity
    for (uint32_t k = 0; k < n; ++k) if (H.alpha_mask & (1u << k)) { alpha = k + 1; break; }
    static const char *const names[] = {"unspecified", "sRGB", "grey", "sYCC", "e-sYCC", "CMYK"};
    const std::string where = std::to_string(n) + (n == 1 ? " channel" : " channels") + " in colour space " + names[cs < 6 ? cs : 0];
    const bool grey_like = cs == J2K_HIP_CS_GRAY || cs == J2K_HIP_CS_UNSPECIFIED, rgb_like = cs == J2K_HIP_CS_SRGB || cs == J2K_HIP_CS_UNSPECIFIED;
    if (H.pal_entries) { // (parse_headers has accepted it: one component, <= 256 entries of 8 bits, three columns)
        RgbaClass k = rgba_class(J2K_HIP_RGBA_PALETTE, 1);
        k.lut_size = std::min<uint32_t>(H.pal_entries, 256);
        // HipCodec::GetFileInfo: LUTmap[c] = the name of channel pal_column_of[c]; CopyWithLutType gives the channel named
        // RED column c with LUTmap[c] == RED, and column 0 where no column is named so (j2k_rgba_file.cpp:83-106)
        uint32_t col[3] = {0, 1, 2};
        for (uint32_t c = 0; c < 3 && c < H.pal_columns; ++c) if (H.pal_column_of[c] < 3) col[H.pal_column_of[c]] = c;
        for (uint32_t i = 0; i < k.lut_size; ++i)
            for (uint32_t j = 0; j < 3; ++j)
                if (col[j] < H.pal_columns) k.lut[i] |= (uint32_t)H.palette[(size_t)i * H.pal_columns + col[j]] << (8 * j);
        return k;
    }
    const bool misplaced = alpha != 0 && alpha != n;
    if ((n == 1 || n == 2) && grey_like) {
        if (misplaced) throw Error(J2K_HIP_ERR_UNSUPPORTED, "the opacity channel is not the last one (" + where + ")");
        return rgba_class(J2K_HIP_RGBA_GREY, n);
    }
    if (n >= 3 && cs == J2K_HIP_CS_SYCC) return rgba_class(J2K_HIP_RGBA_SYCC, n);
    if (n >= 3 && rgb_like) {
        if (misplaced) throw Error(J2K_HIP_ERR_UNSUPPORTED, "the opacity channel is not the last one (" + where + ")");
        return rgba_class(J2K_HIP_RGBA_RGB, n);
    }
    throw Error(J2K_HIP_ERR_UNSUPPORTED, "no conversion to RGBA for " + where);
}

void check_xyz_to_rgb(const FileHeader &H, const RgbaClass &cls)
{
    if (cls.mode != J2K_HIP_RGBA_RGB) throw Error(J2K_HIP_ERR_PARAM, "xyz_to_rgb: only a file of mode RGB holds X'Y'Z' code values");
    const Coding &c = H.cod;
    for (int k = 0; k < 3; ++k) {
        if (c.csgnd[k]) throw Error(J2K_HIP_ERR_PARAM, "xyz_to_rgb: component " + std::to_string(k) + " is signed");
        if (c.cprec[k] != c.cprec[0]) throw Error(J2K_HIP_ERR_PARAM, "xyz_to_rgb: components 0..2 of unlike precision");
    }
}

void check_rgba_dst(const j2k_hip_rgba_dst &dst, bool alpha)
{
    if (dst.struct_size != sizeof(j2k_hip_rgba_dst)) throw Error(J2K_HIP_ERR_PARAM, "j2k_hip_rgba_dst.struct_size mismatch (ABI drift)");
    const j2k_hip_outplane *ch[4] = {&dst.r, &dst.g, &dst.b, &dst.a};
    for (int c = 0; c < (alpha ? 4 : 3); ++c) {
        const j2k_hip_outplane &p = *ch[c];
        check_sample_type(p.sample_bits, p.depth, p.base, p.colbytes, p.rowbytes);
        if (p.sample_bits != dst.r.sample_bits || p.depth != dst.r.depth) throw Error(J2K_HIP_ERR_PARAM, "the RGBA channels must share sample_bits and depth");
    }
    if (dst.demote_ae16 && ((dst.r.sample_bits != 16 && dst.r.sample_bits != 32) || dst.r.depth != 16))
        throw Error(J2K_HIP_ERR_PARAM, "demote_ae16 needs 16-bit or float samples of depth 16");
}

DecRgbaArgs decode_rgba_args(bool reversible, bool mct, int width, int height, long long stride, const RgbaComp *comps,
                             const RgbaClass &cls, const j2k_hip_rgba_dst &dst, bool alpha, int org_x, int org_y, uint32_t xyz_to_rgb)
{
    check_rgba_dst(dst, alpha);
    (void)rgba_class(cls.mode, (uint32_t)cls.ncomp); // (a class made by hand)
    if (width < 1 || height < 1 || org_x < 0 || org_y < 0 || !comps) throw Error(J2K_HIP_ERR_PARAM, "bad RGBA output stage arguments");
    if (cls.alpha_comp >= cls.ncomp || cls.lut_size > 256) throw Error(J2K_HIP_ERR_PARAM, "bad RGBA class");
    for (int c = 0; c < cls.ncomp; ++c) {
        if (comps[c].prec < 1 || comps[c].prec > 16) throw Error(J2K_HIP_ERR_PARAM, "component precision outside 1..16");
        if (comps[c].sub_x < 1 || comps[c].sub_x > 255 || comps[c].sub_y < 1 || comps[c].sub_y > 255) throw Error(J2K_HIP_ERR_PARAM, "sub-sampling factor outside 1..255");
    }
    if (mct && cls.ncomp < 3) throw Error(J2K_HIP_ERR_PARAM, "component transform on fewer than 3 components");
    if (mct)
        for (int c = 1; c < 3; ++c)
            if (comps[c].prec != comps[0].prec || comps[c].sub_x != comps[0].sub_x || comps[c].sub_y != comps[0].sub_y)
                throw Error(J2K_HIP_ERR_PARAM, "component transform on components of unlike precision or sub-sampling");
    if (xyz_to_rgb > 3) throw Error(J2K_HIP_ERR_PARAM, "xyz_to_rgb must be 0..3");
    if (xyz_to_rgb && cls.mode != J2K_HIP_RGBA_RGB) throw Error(J2K_HIP_ERR_PARAM, "xyz_to_rgb: only the RGB mode holds X'Y'Z' code values");
    if (xyz_to_rgb && (comps[1].prec != comps[0].prec || comps[2].prec != comps[0].prec))
        throw Error(J2K_HIP_ERR_PARAM, "xyz_to_rgb: components 0..2 of unlike precision");
    DecRgbaArgs a{};
    a.xyz_to_rgb = (int)xyz_to_rgb;
    a.stride = stride; a.ncomp = cls.ncomp; a.width = width; a.height = height;
    a.reversible = reversible; a.mct = mct; a.org_x = org_x; a.org_y = org_y;
    for (int c = 0; c < 4; ++c) { a.cprec[c] = (int)comps[0].prec; a.sub_x[c] = a.sub_y[c] = 1; }
    for (int c = 0; c < cls.ncomp; ++c) {
        a.comp[c] = comps[c].plane;
        a.cprec[c] = (int)comps[c].prec; a.sub_x[c] = (int)comps[c].sub_x; a.sub_y[c] = (int)comps[c].sub_y;
    }
    a.mode = (int)cls.mode; a.alpha_comp = cls.alpha_comp;
    a.depth = (int)dst.r.depth; a.sample_bytes = (int)dst.r.sample_bits / 8; a.demote = dst.demote_ae16 ? 1 : 0;
    a.lut_size = cls.lut_size;
    std::memcpy(a.lut, cls.lut, sizeof(a.lut));
    for (uint32_t i = a.lut_size; i < 256; ++i) a.lut[i] = 0;

    const j2k_hip_outplane *ch[4] = {&dst.r, &dst.g, &dst.b, &dst.a};
    const int nch = alpha ? 4 : 3;
    for (int c = 0; c < nch; ++c) {
        const j2k_hip_outplane &p = *ch[c];
        a.dst[c] = static_cast<uint8_t *>(p.base);
        a.colbytes[c] = p.colbytes; a.rowbytes[c] = p.rowbytes;
        a.dst_w[c] = (int)std::min<uint32_t>(p.width, (uint32_t)width); a.dst_h[c] = (int)std::min<uint32_t>(p.height, (uint32_t)height);
    }
    // the packed form: the four channels are the four samples of one pixel record
    const long long rec = 4 * a.sample_bytes;
    bool packed = alpha;
    uintptr_t lo = ~(uintptr_t)0;
    for (int c = 0; c < 4 && packed; ++c) {
        packed = a.colbytes[c] == rec && a.rowbytes[c] == a.rowbytes[0] && a.rowbytes[c] % rec == 0 && a.dst_w[c] == a.dst_w[0] && a.dst_h[c] == a.dst_h[0];
        lo = std::min(lo, reinterpret_cast<uintptr_t>(a.dst[c]));
    }
    if (packed && lo % (uintptr_t)rec == 0) {
        unsigned seen = 0;
        for (int c = 0; c < 4; ++c) {
            const uintptr_t off = reinterpret_cast<uintptr_t>(a.dst[c]) - lo;
            if (off % (uintptr_t)a.sample_bytes || off >= (uintptr_t)rec) { seen = 0; break; }
            a.slot[c] = (int)(off / (uintptr_t)a.sample_bytes);
            seen |= 1u << a.slot[c];
        }
        if (seen == 0xf) {
            a.packed = 1;
            a.pix = reinterpret_cast<uint8_t *>(lo); a.pix_rowbytes = a.rowbytes[0];
        }
    }
    return a;
}

} // namespace j2k_hip
