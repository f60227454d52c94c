// rgba_plan.h -- host side of the fused RGBA output stage (no HIP types here): how a file's components become R, G, B, A
// (what RGBAinputFile::ReadFile decides per file, reference: src/common/j2k_rgba_file.cpp:450-735), and the one function
// that fills the kernel's arguments -- for a decode and for the stage hook alike, as decode_output_args does for DecOutArgs.
#pragma once

#include "common.h"

namespace j2k_hip {

struct FileHeader; // decode_plan.h

uint32_t cs_from_enum(uint32_t enumcs); // colr EnumCS -> J2K_HIP_CS_* (reference: j2k_openjpeg_codec.cpp:318-330)

// What the output stage does with the components: the mode (J2K_HIP_RGBA_*), how many components it reads (the first
// `ncomp`), which of them is A (-1: none, A is filled), and for a palette its entries as R | G << 8 | B << 16.
struct RgbaClass {
    uint32_t mode = 0;
    int ncomp = 0;
    int alpha_comp = -1;
    uint32_t lut_size = 0;
    uint32_t lut[256] = {};
};
// By mode and number of components alone (the stage hook; classify_rgba ends here): J2K_HIP_ERR_PARAM for a mode that
// cannot take that many components.  The palette is the caller's to fill.
RgbaClass rgba_class(uint32_t mode, uint32_t ncomp);
// From the parsed header, by the rules of include/j2k_hip.h (j2k_hip_rgba_mode); J2K_HIP_ERR_UNSUPPORTED with a text that
// names the colour space for files the fused path does not take.
RgbaClass classify_rgba(const FileHeader &H);

// Arguments of decode_rgba_kernel (rgba_out.hip).  Per destination pixel: the component samples as decode_output_kernel
// produces them, the mode's arithmetic, the alpha fill, Demote, and either one store of the pixel's record (packed) or one
// store per given channel.
struct DecRgbaCore {
    const void *comp[4]; long long stride; // decoded components (int32 or float32 words)
    int ncomp, width, height, reversible, mct;
    int cprec[4], sub_x[4], sub_y[4];
    int org_x, org_y;                      // as in DecOutArgs
    int mode, alpha_comp;                  // J2K_HIP_RGBA_*; the component that is A, or -1: A = 2^depth - 1
    int depth, sample_bytes, demote;       // shared by the four destinations
    // packed: R, G, B, A are samples slot[0..3] of one record of 4 * sample_bytes bytes at pix + y * pix_rowbytes + x * record;
    // pix and pix_rowbytes are multiples of the record size, all four channels have dst_w[0] x dst_h[0] samples
    int packed, slot[4];
    uint8_t *pix; long long pix_rowbytes;
    // general: R, G, B, A = dst[0..3]; dst[c] == nullptr: the channel is not written
    uint8_t *dst[4]; long long colbytes[4], rowbytes[4];
    int dst_w[4], dst_h[4];
    uint32_t lut_size, lut[256];           // palette entry = R | G << 8 | B << 16; entries from lut_size on are 0
};
// ... and, behind them, what the X'Y'Z' -> R'G'B' variants read (j2k_hip_decode_set_xyz_to_rgb; xyz_tables.h).  The kernels
// without the conversion take DecRgbaCore as their argument, so their argument layout is what it was before these existed.
struct DecRgbaArgs : DecRgbaCore {
    int xyz_to_rgb;        // 0: off (nothing below is read); 1..3: the target coding, mode RGB only
    const float *xyz_dl;   // max(2^cprec[0], 4) words: code -> linear light; 16-byte aligned
    const float *xyz_othr; // max(2^depth, 4) words: the 2^depth - 1 thresholds of codes 1 .. top, then +infinity; 16-byte aligned
    float xyz_n[9];        // X Y Z -> R G B, row by row
};
// Preconditions (not checked on the device; decode_rgba_args below is the one place that fills the struct):
//   * mode RGB: ncomp 3 or 4, alpha_comp 3 or -1; GREY: ncomp 1 or 2, alpha_comp 1 or -1; PALETTE: ncomp 1, alpha_comp -1,
//     lut_size <= 256; SYCC: ncomp 3, alpha_comp -1; alpha_comp < ncomp.  With mct, ncomp >= 3 and components 0..2 share
//     precision and sub-sampling factors;
//   * cprec[c] in 1..16, sub_x[c] and sub_y[c] >= 1, org_x, org_y >= 0; comp[c] holds ceil((org_x + width) / sub_x[c]) x
//     ceil((org_y + height) / sub_y[c]) words at row stride `stride` for every c < ncomp (each is read);
//   * sample_bytes is 1 or 2, 1 <= depth <= 8 * sample_bytes, or 4 (32-bit floats) with 1 <= depth <= 16; demote only with
//     sample_bytes 2 or 4 and depth == 16;
//   * dst_w[c] <= width, dst_h[c] <= height; dst[c] + y * rowbytes[c] + x * colbytes[c] is writable for x < dst_w[c],
//     y < dst_h[c] and aligned to sample_bytes (general form: dst[0..2] given, dst[3] may be nullptr);
//   * packed: slot[] is a permutation of 0..3, pix and pix_rowbytes are multiples of 4 * sample_bytes, and every record of
//     dst_w[0] x dst_h[0] is writable;
//   * xyz_to_rgb != 0: mode RGB, cprec[0] == cprec[1] == cprec[2] (every component sample is an index into xyz_dl: the clamp
//     of component_samples keeps it below 2^cprec), and both tables on the device.

struct RgbaComp { const void *plane; uint32_t prec, sub_x, sub_y; };
// What j2k_hip_decode_rgba refuses about its destination before anything else happens (J2K_HIP_ERR_PARAM): a struct of
// another size, sample_bits other than 8 / 16 / 32, a depth outside 1..sample_bits (float: 1..16), a float channel off the
// 4-byte grid, channels of unlike sample_bits or depth, demote_ae16 on anything but 16-bit or float samples of depth 16.  `alpha`: whether dst.a is a destination
// (the C ABI: a.base != NULL; the stage hook, whose bases are offsets: a.sample_bits != 0).
void check_rgba_dst(const j2k_hip_rgba_dst &dst, bool alpha);
// Fills the arguments.  comps: the cls.ncomp components the mode reads.  ch[0..3] = R, G, B, A with their FINAL (device)
// addresses in .base; ch[3] is read only with `alpha`.  Chooses the packed form when the four channels are the four samples
// of one pixel record (all given; colbytes == 4 * sample_bytes; equal rowbytes, a multiple of the record; equal extents;
// bases a permutation of p + {0,1,2,3} * sample_bytes with p aligned to the record), the general form otherwise.
// xyz_to_rgb (0..3): the conversion of j2k_hip_decode_set_xyz_to_rgb; non-zero is refused (J2K_HIP_ERR_PARAM, the text naming
// xyz_to_rgb) for every mode but RGB and for components 0..2 of unlike precision.  The tables' device addresses and the
// matrix are the caller's to add (they belong to the handle).
DecRgbaArgs decode_rgba_args(bool reversible, bool mct, int width, int height, long long stride, const RgbaComp *comps,
                             const RgbaClass &cls, const j2k_hip_rgba_dst &dst, bool alpha, int org_x = 0, int org_y = 0,
                             uint32_t xyz_to_rgb = 0);
// What a non-zero xyz_to_rgb refuses about a file, from the header alone (J2K_HIP_ERR_PARAM, the text naming xyz_to_rgb): a
// mode other than RGB, components 0..2 that are signed or of unlike precision.
void check_xyz_to_rgb(const FileHeader &H, const RgbaClass &cls);

} // namespace j2k_hip
