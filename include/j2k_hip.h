/*
 * j2k_hip.h -- C ABI of the MI355X-native JPEG 2000 encode path (libj2k_hip.so).
 *
 * This is the drop-in boundary behind the reference plug-in's encode entry point.  Every entry
 * point below replaces a step of
 *     j2k::OpenJPEGCodec::WriteFile(OutputFile&, const FileInfo&, const Buffer&, Progress*)
 *         reference: src/common/j2k_openjpeg_codec.cpp:589-758 (declared src/common/j2k_codec.h:315)
 * and is what a `j2k::Codec` subclass registered in CodecContainer::CodecContainer
 * (reference: src/common/j2k_codec.cpp:508-519) binds to.  See INTEGRATION.md for the ~50-line
 * C++ subclass (shipped as j2k_amd/host/hip_codec.cpp).
 *
 * Conventions: plain C types only, no exceptions cross this boundary, every function returns an
 * int status (0 = J2K_HIP_OK) unless stated otherwise; j2k_hip_last_error() gives the text that the
 * C++ side turns into `throw j2k::Exception(...)` (reference: src/common/j2k_exception.h:35-45,
 * thrown at j2k_openjpeg_codec.cpp:756-757).  All entry points are re-entrant as long as each
 * thread uses its own encoder handle (SURVEY.md section 8b "Threading").
 *
 * There is NO CPU fallback: without a usable HIP device every call fails with
 * J2K_HIP_ERR_DEVICE.
 */
#ifndef J2K_HIP_H
#define J2K_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define J2K_HIP_ABI_VERSION 9

enum {
    J2K_HIP_OK = 0,
    J2K_HIP_ERR_PARAM = 1,    /* bad argument / unsupported coding parameter               */
    J2K_HIP_ERR_DEVICE = 2,   /* HIP runtime error (message holds hipGetErrorString)        */
    J2K_HIP_ERR_MEMORY = 3,   /* host or device allocation failed                            */
    J2K_HIP_ERR_OVERFLOW = 4, /* an internal or caller buffer was too small -- or, from an encode, "code-block has more
                               * bit-planes than its sub-band signals (guard bits exceeded)": a coefficient of the frame
                               * outgrew the Mb = exponent + guard bits - 1 bit-planes its sub-band's QCD entry allows (two
                               * guard bits unless j2k_hip_params.guard_bits says otherwise).  The
                               * frame is refused, never written wrongly                                                  */
    J2K_HIP_ERR_SINK = 5,     /* the sink's write callback reported a short write            */
    J2K_HIP_ERR_UNSUPPORTED = 6 /* decode only: a well-formed file that uses a JPEG 2000 feature this decoder does
                                 * not implement (the text names it).  A host that has another reader -- the
                                 * reference's OpenJPEGCodec -- hands the file to it (HipCodec::SetFallback);
                                 * a malformed file is J2K_HIP_ERR_PARAM instead                 */
};

/* Progression orders: values of j2k::Order (reference: src/common/j2k_codec.h:117-124) = OPJ_PROG_ORDER =
 * the COD marker's SGcod byte.  The reference's WriteFile never copies settings.order into
 * opj_cparameters_t (j2k_openjpeg_codec.cpp:703-709), so it always writes LRCP -- the default (0) here too;
 * the other orders give the bytes OpenJPEG writes for them. */
enum { J2K_HIP_LRCP = 0, J2K_HIP_RLCP = 1, J2K_HIP_RPCL = 2, J2K_HIP_PCRL = 3, J2K_HIP_CPRL = 4 };

typedef struct j2k_hip_encoder j2k_hip_encoder;

/*
 * Coding parameters = the subset of j2k::FileInfo / j2k::CompressionSettings
 * (reference: src/common/j2k_codec.h:131-209) that reaches the codec, plus the OpenJPEG defaults
 * that WriteFile leaves untouched (reference: j2k_openjpeg_codec.cpp:703-719).
 * Zero means "reference default" for every field marked (0 = default).
 */
typedef struct j2k_hip_params {
    uint32_t struct_size;     /* = sizeof(j2k_hip_params); guards ABI drift                     */
    uint32_t width, height;   /* FileInfo.width / .height                                        */
    uint32_t channels;        /* FileInfo.channels: 1, 3 or 4                                    */
    uint32_t depth;           /* FileInfo.depth: target precision 1..16, unsigned                */
    uint32_t reversible;      /* settings.reversible: 1 = 5/3 lossless, 0 = 9/7                  */
    uint32_t ycc;             /* settings.ycc: 1 = RCT/ICT on channels 0..2 (tcp_mct)            */
    uint32_t layers;          /* settings.layers (0 = 1); without layer_rates the extra layers   */
                              /*    are empty, as in the reference                               */
    uint32_t tile_size;       /* settings.tileSize: tiles tile_size^2 at origin 0; 0 = untiled   */
    uint32_t num_resolutions; /* (0 = 6)  OpenJPEG numresolution = DWT levels + 1                */
    uint32_t cblk_w, cblk_h;  /* (0 = 64) code-block size, power of two, 4..64                   */
    uint32_t progression;     /* settings.order: J2K_HIP_LRCP (default) .. J2K_HIP_CPRL            */
    uint32_t promote_ae16;    /* 1: apply the AE 15+1 -> 16 bit Promote() to 16-bit samples on   */
                              /*    load (reference: src/aftereffects/FrameSeq.cpp:311-355) so   */
                              /*    the host can skip PromoteWorld/DemoteWorld (j2k.cpp:843-855) */
    const char *comment;      /* COM marker text; NULL = "Created by j2k_hip"; "" = no COM       */
    /* ---- file wrapper (ABI 2).  All zero = raw J2K codestream, which is what the
     * reference writes (j2k_openjpeg_codec.cpp:609-614 disables its JP2 branch because OpenJPEG's
     * JP2 writer seeks; this one never does). */
    uint32_t file_format;     /* FileInfo.format: J2K_HIP_FMT_J2K or J2K_HIP_FMT_JP2                 */
    uint32_t color_space;     /* J2K_HIP_CS_*: the OPJ_COLOR_SPACE the reference derives from        */
                              /*    FileInfo.colorSpace (j2k_openjpeg_codec.cpp:650-661)             */
    uint32_t alpha;           /* 0 = none; k + 1 = channel k is opacity (FileInfo.alpha != NO_ALPHA) */
    uint32_t alpha_premultiplied; /* FileInfo.alpha == PREMULTIPLIED: cdef Typ 2 instead of 1       */
    const void *icc_profile;  /* FileInfo.iccProfile / .profileLen: restricted ICC profile for the   */
    size_t icc_profile_len;   /*    colr box (method 2); NULL/0 = enumerated colour space            */
    /* ---- rate control (ABI 3).  NULL = no rate target: every coding pass goes into
     * layer 0, which is all the reference's WriteFile ever asks OpenJPEG for (it never copies
     * settings.method / fileSize / quality, j2k_openjpeg_codec.cpp:707).  Otherwise `layers` compression
     * ratios, strictly decreasing, one per quality layer, with OpenJPEG's tcp_rates semantics
     * (cp_disto_alloc): layer l of each tile is cut so that layers 0..l stay within
     * raw tile bytes / layer_rates[l]; a ratio <= 1 (or 0) lifts the limit (last layer lossless for 5/3).
     * The result is byte-identical to OpenJPEG's rate allocation for the same ratios. */
    const float *layer_rates;
    /* Fixed quality instead (excludes layer_rates): `layers` PSNR targets in dB, one per quality layer, with
     * the semantics of OpenJPEG's cp_fixed_quality / tcp_distoratio (opj_compress -q): layer l is cut where
     * the distortion estimate of layers 0..l reaches the target; 0 = everything that is left.  Byte-identical
     * to OpenJPEG's allocation for the same targets. */
    const float *layer_psnr;
    /* ---- resolution box (ABI 5): FileInfo.pixelAspect and .dpi (reference: src/common/j2k_codec.h:168-169, set at
     * src/aftereffects/j2k.cpp:743).  JP2 only: a `res ` super-box with a capture-resolution box goes into the JP2
     * header when the pixels are not square or a dpi is given; all zero (or aspect 1:1 and dpi 0) = no box, the
     * file OpenJPEG would write. */
    uint32_t pixel_aspect_num, pixel_aspect_den; /* width : height of one pixel                                */
    float dpi;                /* vertical resolution in dots per inch; 0 = 72 when only the aspect is known      */
    /* ---- user-defined precincts (ABI 7; T.800 B.6, COD Scod bit 0).  0 = maximal precincts (2^15), which is what the
     * reference's WriteFile leaves (OpenJPEG's default).  Otherwise num_precincts sizes (powers of two), HIGHEST
     * resolution first, with the semantics of OpenJPEG's res_spec / prcw_init / prch_init (opj_compress -c): the
     * resolutions below the last one given take half the size each.  Digital-cinema profiles prescribe them
     * (128 x 128 for the lowest resolution, 256 x 256 above; CompressionMethod::CINEMA, reference:
     * src/common/j2k_codec.h:108-128).  Byte-identical to OpenJPEG for the same sizes, in all five progressions. */
    uint32_t num_precincts;
    uint32_t precinct_w[33], precinct_h[33];
    /* ---- digital cinema profiles (ABI 8; CompressionMethod::CINEMA with DCIProfile DCI_2K / DCI_4K, reference:
     * src/common/j2k_codec.h:108-128, populated at src/aftereffects/j2k.cpp:810-830).  0 = none.  3 / 4 = the 2K / 4K profile
     * as OpenJPEG writes it for Rsiz 3 / 4 (OPJ_PROFILE_CINEMA_2K / _4K), byte for byte: three 12-bit components within
     * 2048 x 1080 / 4096 x 2160, 9/7 with ICT, one layer, CPRL, 32 x 32 code-blocks, at most 6 / 7 resolutions, precincts of
     * 128 (lowest resolution) and 256, one tile-part per component (4K: per component and resolution group, with the
     * progression order change that puts the 2K resolutions first), a TLM marker segment; the frame cut to
     * max_cs_size bytes in all and max_comp_size bytes per component.  Every other coding field of this struct is then
     * overridden by the profile; `comment` and the file wrapper fields still apply (the comment's bytes come off the budget,
     * as in OpenJPEG, which writes its own there). */
    uint32_t dci_profile;
    uint32_t max_cs_size;     /* bytes per frame; 0 or more than 1302083 = 1302083 (24 frames/s at 250 Mbit/s)      */
    uint32_t max_comp_size;   /* bytes per component; 0 or more than 1041666 = 1041666                               */
    /* ---- code-block style (T.800 Table A.19, D.4 - D.7; opj_compress -M, Kakadu Cmodes).  The COD marker's SPcod code-block
     * style byte: 0 = none, which is all the reference's WriteFile asks for (CompressionSettings has no such field); otherwise
     * any combination of J2K_HIP_CBLK_BYPASS, _RESET, _TERMALL, _PTERM and _SEGSYM, byte for byte what OpenJPEG writes for the
     * same mode.  Vertically causal contexts (bit 8) are not written: J2K_HIP_ERR_PARAM.  A style excludes layer_rates,
     * layer_psnr and dci_profile (J2K_HIP_ERR_PARAM): the layer allocation does not price codeword segments.
     * J2K_HIP_ABI_VERSION is still 9: the field was appended, no function changed.  struct_size is the guard against a caller
     * built with another layout, as for every field before it.  Where the struct ends in alignment padding (LP64: 4 bytes
     * behind max_comp_size) the field takes that padding and sizeof does not move: a caller of the older header that
     * zero-initialises the whole struct, as the header has always asked for, passes style 0. */
    uint32_t cblk_style;
    /* ---- sub-sampled components (T.800 A.5.1, SIZ XRsiz / YRsiz; 4:2:2 and 4:2:0 Y Cb Cr).  comp_sub_x[c] / comp_sub_y[c]:
     * component c has one sample per comp_sub_x[c] x comp_sub_y[c] points of the reference grid; 0 = 1; 1, 2 or 4.  All ones
     * (or all zero) = the file the library has always written.  `width` and `height` stay the image area on the reference grid
     * (origin 0); component c is ceil(width / sub_x) x ceil(height / sub_y) samples.
     *   rgb_to_sycc == 0: planes[c] views component c on its OWN grid -- that many samples.  Host planes may be
     *     allocations of their own: channels that do not share a buffer are uploaded one by one, nothing between them is read.
     *   rgb_to_sycc == 1: `channels` is 3 or 4, planes are R, G, B[, A] of the full image (width x height each) and the library
     *     makes Y, Cb, Cr[, A] from them on the GPU while it loads them: components 1 and 2 share one factor pair out of
     *     (1,1), (2,1), (2,2); a fourth component (alpha) is (1,1) and passes through.  Exact integer arithmetic on the samples
     *     at `depth` bits (after Promote and the depth conversion), h = 2^(depth-1), top = 2^depth - 1, >> a floor shift:
     *         Y   = (19595 R + 38470 G + 7471 B + 32768) >> 16
     *         cb' = -11059 R - 21709 G + 32768 B,   cr' = 32768 R - 27439 G - 5329 B        (per pixel, not rounded)
     *         Cb  = clamp(h + ((sum cb' + (1 << (15 + k))) >> (16 + k)), 0, top),  Cr alike,   k = log2(sub_x * sub_y)
     *     the sum over the chroma sample's sub_x x sub_y pixels; a pixel beyond the right or bottom edge repeats the last column
     *     or row.  This is the analysis to the replicating sYCC read of j2k_hip_decode_rgba.  Set color_space = J2K_HIP_CS_SYCC
     *     for a JP2 file that says so.
     * Component 0 is never sub-sampled (libopenjp2's byte budget is computed from component 0's factors; nothing else is pinned).
     * J2K_HIP_ERR_PARAM, the text naming the field: a factor outside {1, 2, 4}; comp_sub on component 0; `ycc` with a sub-sampled
     * component or with rgb_to_sycc; dci_profile or layer_psnr with either; rgb_to_sycc with fewer than 3 channels or with other
     * factor pairs than the above.  layer_rates and cblk_style combine with sub-sampling as they do without.
     * Entry points: j2k_hip_encode, _encode_to_buffer, _encode_device, _encode_begin / _end and _encode_begin_borrowed / _end
     * write identical bytes, byte for byte what libopenjp2 writes for the same components (the synchronous host call is then not
     * band-pipelined: j2k_hip_stats.bands = 0); so do j2k_hip_encode_sequence_device and j2k_hip_encode_batch, frame by frame.
     * The tile-sharded entry points -- j2k_hip_encode_tiles, _encode_tiles_device, _encode_tiles_distributed -- refuse a
     * sub-sampled frame or rgb_to_sycc with J2K_HIP_ERR_PARAM ("comp_sub / rgb_to_sycc: ...") before any device work.
     * J2K_HIP_ABI_VERSION is still 9: fields were appended, no function changed; struct_size is the guard. */
    uint32_t comp_sub_x[4], comp_sub_y[4];
    uint32_t rgb_to_sycc;
    /* ---- cinema colour: R'G'B' to X'Y'Z' code values in the front end (a DCI frame holds 12-bit X'Y'Z': CIE XYZ normalised to
     * 48 cd/m2 out of 52.37, under a 1/2.6 power).  0 = off: every byte, launch and statistic is what it was without the field.
     * Otherwise channels 0..2 are R, G, B of the full image and say how they are coded:
     *     1  sRGB (IEC 61966-2-1 piecewise curve, Rec.709 primaries, D65)
     *     2  Rec.709 primaries under a pure 2.4 power (BT.1886)
     *     3  Rec.709 primaries, linear light
     * A fourth channel (alpha) takes the ordinary path (Promote, depth conversion, DC shift).  A pixel, to the rounding:
     *   1. v = the integer sample of d bits, d = the plane's `depth` (after Promote where promote_ae16 applies; a float plane:
     *      the integer j2k_hip_plane's rule makes of it); a stored sample above 2^d - 1 counts as 2^d - 1.
     *      l = lin[v],  lin[v] = (float)EOTF((double)v / (2^d - 1)), a table of 2^d binary32 values computed on the host in double:
     *      EOTF_1(x) = x <= 0.04045 ? x / 12.92 : pow((x + 0.055) / 1.055, 2.4),  EOTF_2(x) = pow(x, 2.4),  EOTF_3(x) = x.
     *   2. M_ij = (float)((double)m_ij * (48.0 / 52.37)), m = the sRGB -> XYZ (D65) matrix, no chromatic adaptation (DCI practice):
     *          0.4124564 0.3575761 0.1804375 / 0.2126729 0.7151522 0.0721750 / 0.0193339 0.1191920 0.9503041
     *      X = fadd(fadd(fmul(M00, r), fmul(M01, g)), fmul(M02, b)): every product and sum rounded to binary32 on its own,
     *      nothing contracted to an FMA; Y and Z alike from rows 1 and 2.
     *   3. top = 2^depth - 1 (params.depth), thr[c] = (float)pow(((double)c - 0.5) / top, 2.6) for c = 1..top (strictly increasing
     *      in binary32 for every depth); the code is the number of c with thr[c] <= X -- round-to-nearest of top * X^(1/2.6),
     *      decided on thresholds: no transcendental function decides a code on the device.
     *   The code minus the DC shift is the component sample (the 9/7 path: the same integer as a float); with `ycc` the RCT / ICT
     *   follows as for any three components.  j2k_hip_xyz_tables hands out lin, thr and M as the kernel gets them.
     * J2K_HIP_ERR_PARAM, the text naming rgb_to_xyz: a value above 3; fewer than 3 channels; rgb_to_sycc with it; a comp_sub
     * factor other than 1.  It combines with everything else: dci_profile, layer_rates / layer_psnr, ycc, cblk_style, tiles
     * inside one call, the JP2 wrapper, float planes, promote_ae16.  The main header and the file header do not depend on it.
     * Entry points: as for rgb_to_sycc -- every entry point that takes planes but the tile-sharded ones, which refuse it with
     * J2K_HIP_ERR_PARAM before any device work.  The front end runs as a pass of its own (never fused into DWT level 1, never
     * band-pipelined: j2k_hip_stats.bands = 0).
     * J2K_HIP_ABI_VERSION is still 9: the field was appended, no function changed; struct_size is the guard.  Where the struct
     * ended in alignment padding (LP64: 4 bytes behind rgb_to_sycc) the field takes that padding and sizeof does not move: a
     * caller of the older header that zero-initialises the whole struct, as the header has always asked for, passes 0. */
    uint32_t rgb_to_xyz;
    /* ---- guard bits (T.800 A.6.4 Sqcd, E.1: a sub-band signals Mb = exponent + guard bits - 1 bit-planes).  A lossless frame
     * under the reversible colour transform can hold code-blocks of Mb + 1 bit-planes at two guard bits;
     * libopenjp2 writes such a frame wrongly, this library refuses it -- or, asked to, writes it with the guard bits it needs.
     *     0                    two guard bits, what libopenjp2 writes: every byte, launch and statistic is what it was without
     *                          the field; a frame beyond them is J2K_HIP_ERR_OVERFLOW.
     *     1 .. 7               that many guard bits, strictly: Sqcd = style | g << 5, every band signals exponent + g - 1
     *                          bit-planes (the code-block slots grow with them), a frame beyond them is refused alike.  2 writes
     *                          the bytes of 0.
     *     J2K_HIP_GUARD_AUTO | floor (floor 0 .. 7, 0 = 2)
     *                          the smallest G >= floor at which no code-block has more bit-planes than its band signals:
     *                          G = max(floor, max over the blocks of numbps - exponent(band) + 1), one G for the file (QCD is a
     *                          main-header marker segment).  A frame in range at floor 2 is written byte for byte as with 0, at
     *                          no launch, copy or wait more (j2k_hip_stats.bands is what it is without the field).  A frame
     *                          beyond the floor is planned once more on the host from the Tier-1 results it has -- packet
     *                          headers, QCD, tile-part lengths, and under layer_rates the layer allocation, on the host and on
     *                          the device path alike -- and no kernel of the front end, the DWT or Tier-1 runs again: a block's
     *                          decisions, passes and codeword do not depend on the guard bits.  More than 7, or more bit-planes
     *                          than the reader takes, is J2K_HIP_ERR_OVERFLOW as with 0.
     * What stays an error in every mode: a Tier-1 slot overflow -- the kernels' own "Tier-1 kernel reported error" (too many
     * bit-planes for the pass tables, decision buffer, codeword buffer) -- is J2K_HIP_ERR_OVERFLOW and never a short block.
     * J2K_HIP_ERR_PARAM, the text naming guard_bits, before any device work: any other value; a count that gives a sub-band
     * more than the 30 bit-planes this library's own reader accepts in a code-block; a non-zero value with dci_profile (the
     * profile is pinned to libopenjp2's bytes); J2K_HIP_GUARD_AUTO on the entry points that take or make a header without a
     * frame -- j2k_hip_main_header, j2k_hip_encode_tiles, _encode_tiles_device, _encode_tiles_distributed (rank 0 writes the
     * header before any tile is coded); a fixed count is fine there.
     * Entry points: every one that writes a file -- j2k_hip_encode, _encode_to_buffer, _encode_begin / _end,
     * _encode_begin_borrowed, _encode_device, _encode_sequence_device (each frame its own G), _encode_batch -- and the
     * tile-sharded ones with a fixed count.  The band-pipelined call writes at the floor while its stages come down and, where a
     * stage's block exceeds it, plans the frame again once all stages are in: the sink sees nothing before the plan is final.
     * j2k_hip_encode_get_guard_bits reports what the handle's last file got.  The read side takes the count from the file.
     * J2K_HIP_ABI_VERSION is still 9: the field was appended and functions were added, none changed.  struct_size is the guard:
     * sizeof(j2k_hip_params) of this header, or the size the struct had before the field (it ended behind rgb_to_xyz), which
     * reads as guard_bits 0. */
    uint32_t guard_bits;
    /* ---- quality layers at given rate-distortion slopes (excludes layer_rates, layer_psnr, dci_profile and cblk_style:
     * J2K_HIP_ERR_PARAM, the text naming layer_slopes).  `layers` thresholds, one per quality layer: layer l of every tile is
     * opj_tcd_makelayer(l, layer_slopes[l], final) over the tile's code-blocks -- a block gives the layer the passes whose
     * weighted distortion decrease per byte reaches the threshold (OpenJPEG's units and arithmetic, IEEE doubles).  A negative
     * entry takes everything that is left; entries need not be ordered.  A NaN or an infinite entry is J2K_HIP_ERR_PARAM.
     * There is no search and no byte budget: blocks are cut independently, in one launch on the device behind the coder for
     * all tiles (and all frames of j2k_hip_encode_sequence_device), and the per-pass tables are not copied to the host.  One
     * threshold for every frame of a sequence gives constant quality: the bytes follow the content.
     * j2k_hip_encode_get_layer_slopes reports the thresholds a layer_rates / layer_psnr search ended at; a file written with
     * them is that search's file, byte for byte.  Combines with what layer_rates combines with (tiles, precincts, every
     * progression, comp_sub_* / rgb_to_sycc, rgb_to_xyz, guard_bits) on every entry point that writes a file, the tile-sharded
     * ones included; the band-pipelined host call stays off as under every rate control.  NULL: every byte, launch, copy and
     * statistic is what it was without the field.
     * J2K_HIP_ABI_VERSION is still 9: the field was appended and functions were added, none changed.  struct_size is the guard:
     * sizeof(j2k_hip_params) of this header, the size before this field (offsetof layer_slopes: guard_bits and the padding
     * behind it) or the size before guard_bits; the two older sizes read as layer_slopes NULL. */
    const double *layer_slopes;
} j2k_hip_params;

#define J2K_HIP_GUARD_AUTO 0x100u /* OR-ed with the floor, 0 .. 7 (0 = 2) */

enum { J2K_HIP_CBLK_BYPASS = 1, J2K_HIP_CBLK_RESET = 2, J2K_HIP_CBLK_TERMALL = 4, J2K_HIP_CBLK_VCAUSAL = 8 /* decode only */,
       J2K_HIP_CBLK_PTERM = 16, J2K_HIP_CBLK_SEGSYM = 32 };

enum { J2K_HIP_FMT_J2K = 0, J2K_HIP_FMT_JP2 = 1 };
enum { J2K_HIP_CS_UNSPECIFIED = 0, J2K_HIP_CS_SRGB = 1, J2K_HIP_CS_GRAY = 2, J2K_HIP_CS_SYCC = 3,
       J2K_HIP_CS_EYCC = 4, J2K_HIP_CS_CMYK = 5 };

/*
 * One image channel = a faithful image of j2k::Channel (reference: src/common/j2k_codec.h:221-247):
 * a borrowed, strided view, valid only for the duration of the call, never written.
 * For the *_device entry points `base` is a device pointer.
 *
 * Float samples (an After Effects 32-bpc world, PF_PixelFormat_ARGB128): sample_bits == 32 means IEEE binary32 samples of
 * nominal range 0..1.  depth keeps its meaning: it is the integer depth d (1..16) that the float stands for; d < 1 or
 * d > 16 is J2K_HIP_ERR_PARAM.  base, colbytes and rowbytes must be multiples of 4 (J2K_HIP_ERR_PARAM before any device
 * work).  A float sample x becomes the d-bit integer sample v that everything downstream sees as it sees a d-bit integer
 * sample -- the depth conversion to params.depth, the DC shift, the colour transform, rgb_to_sycc:
 *     t = x > 1 ? 1 : (x > 0 ? x : 0)                 NaN, -0.0, negatives and -inf give 0, +inf gives 1
 *     v = (unsigned)(t * (float)(2^d - 1) + 0.5f)     product and sum each rounded to binary32; the cast truncates
 *     v = Promote((unsigned)(t * 32768.0f + 0.5f))    with promote_ae16, which needs d == 16 on a float channel
 * (d = 8: the reference's Convert<PF_FpShort, A_u_char>; d = 16: FLOAT_TO_SIXTEEN, src/aftereffects/FrameSeq.h:47; the
 * promote form: its ARGB128 -> ARGB64 copy followed by PromoteWorld, FrameSeq.cpp:95-110, :189-198, taken as the 16-bit
 * value it evidently means).  The float of a grid point, (float)p / (float)(2^d - 1), returns p for every d and p, and
 * v / 32768 returns Promote(v): a float world made from integers encodes to the integer world's bytes.
 * Every entry point that takes planes takes float ones, and float and integer channels may mix in one call.  Float frames
 * run the front end as a pass of its own (like sub-sampled ones: never fused into DWT level 1, never band-pipelined --
 * j2k_hip_stats.bands = 0).  sample_bits other than 8, 16 or 32: J2K_HIP_ERR_PARAM.  J2K_HIP_ABI_VERSION is still 9: no
 * struct and no function changed -- a sample type was added that every earlier version refused.
 */
typedef struct j2k_hip_plane {
    const void *base;    /* Channel.buf                                                          */
    ptrdiff_t colbytes;  /* Channel.colbytes                                                     */
    ptrdiff_t rowbytes;  /* Channel.rowbytes                                                     */
    uint32_t sample_bits; /* 8 (sampleType UCHAR), 16 (USHORT) or 32 (IEEE float, see above)     */
    uint32_t depth;       /* Channel.depth (significant bits in the sample, = sample_bits in AE);
                             float samples: the integer depth 1..16 they stand for              */
} j2k_hip_plane;

/* Sink = OutputFile::Write (reference: src/common/j2k_io.h:58-79). Must return n on success.
 * The codestream is delivered front to back; Seek is never needed. */
typedef size_t (*j2k_hip_write_fn)(void *user, const void *buf, size_t n);

/* Per-call timing/size report (all times in milliseconds, device times from hipEvents). */
typedef struct j2k_hip_stats {
    double ms_upload;    /* H2D of the interleaved frame (0 for *_device)                        */
    double ms_frontend;  /* A1+A2+A4+A5 kernel                                                   */
    double ms_dwt;       /* A6 kernels, all levels                                               */
    double ms_t1;        /* A7+A8 kernels                                                        */
    double ms_t2_host;   /* A9 on the host (packet headers, markers)                             */
    double ms_assemble;  /* metadata D2H + header H2D + codestream gather kernel                 */
    double ms_download;  /* D2H of the finished codestream                                       */
    double ms_total;     /* wall time of the call                                                */
    uint64_t codestream_bytes;
    uint64_t num_codeblocks;
    uint64_t num_symbols; /* MQ decisions coded                                                  */
    double dwt_bytes;     /* algorithmic DWT bytes of this call                   */
    /* ---- band-pipelined host calls (ABI 9): the frame goes up in `bands` row bands while the GPU already transforms and
     * codes the bands that have arrived (0 = the call was not pipelined).  ms_upload is then the host time spent in the
     * bands' copies, ms_after_upload what was left of the call once the last byte of the frame had gone up -- the part of
     * the GPU work, Tier-2 and download that the upload did NOT hide (not pipelined: everything but the upload) -- and
     * early_download_bytes the codeword bytes that were already in host memory when the last code-block was finished. */
    uint32_t bands;
    uint32_t reserved_;
    double ms_after_upload;
    uint64_t early_download_bytes;
} j2k_hip_stats;

/* --- lifetime ----------------------------------------------------------------------------------
 * Replaces opj_create_compress/opj_destroy_codec (reference: j2k_openjpeg_codec.cpp:616, :746).
 * `device` is the HIP device ordinal.  The handle owns streams and growable device arenas that are
 * reused across calls (frames of a sequence reuse all allocations).  One handle serves one call at a
 * time; several handles driven from several host threads share the device, and their frames overlap
 * on it (the MQ coder chains of one frame run beside the DWT and context modelling of the next),
 * which is where most of the throughput of an image sequence comes from. */
int j2k_hip_abi_version(void);
int j2k_hip_create(j2k_hip_encoder **enc, int device);
void j2k_hip_destroy(j2k_hip_encoder *enc);
const char *j2k_hip_last_error(const j2k_hip_encoder *enc); /* never NULL; enc may be NULL */

/* --- encode ------------------------------------------------------------------------------------
 * Replaces CopyBuffer + opj_setup_encoder + opj_start_compress + opj_encode + opj_end_compress
 * (reference: j2k_openjpeg_codec.cpp:700-736).  `planes[i]` is codec channel i (R,G,B[,A] after
 * RGBAoutputFile's channelMap, reference: src/common/j2k_rgba_file.cpp:763-813). */
int j2k_hip_encode(j2k_hip_encoder *enc, const j2k_hip_params *params, const j2k_hip_plane *planes,
                   j2k_hip_write_fn write, void *user);
/* When an encode fails.  The sink sees the file's first byte only after the whole file has been planned (host Tier-2), in
 * the one-piece and in the band-pipelined path alike: a failure up to there -- every J2K_HIP_ERR_OVERFLOW of a frame that
 * exceeds its guard bits, every Tier-1 error -- returns its code with NOT ONE BYTE handed to the sink, and the buffer
 * and device entry points write neither their output pointers nor *len / *out_len nor a byte of the caller's buffer (the
 * caller's values stand; nothing is a file's length).  Only J2K_HIP_ERR_SINK (a short write), a device error during the
 * download and a caller buffer too small for the planned file (J2K_HIP_ERR_OVERFLOW with the file's length reported) come
 * later: what a sink holds then is a prefix of the file and is to be discarded.  After any failure the handle is
 * drained -- nothing pending, nothing in flight -- and takes the next frame, of the same geometry or another. */

/* The same call cut in two, for a host that pipelines the frames of an image sequence from ONE thread over
 * several handles (the reference's frame loop, src/aftereffects/FrameSeq.cpp:1211-1372, calls WriteFile once
 * per frame): _begin returns when the frame has left the caller's buffers (which may be reused at once) and
 * every GPU stage is queued; _end waits for the frame, plans and assembles the codestream and hands it to the
 * sink.  begin(h0,f0) begin(h1,f1) end(h0) begin(h0,f2) end(h1) ... keeps the GPU busy across frames.
 * `params` and `planes` are read during _begin only.  One _begin per handle at a time. */
int j2k_hip_encode_begin(j2k_hip_encoder *enc, const j2k_hip_params *params, const j2k_hip_plane *planes);
int j2k_hip_encode_end(j2k_hip_encoder *enc, j2k_hip_write_fn write, void *user);
/* _begin for a host that can leave the frame alone until _end: returns at once (the parameters are checked, the two
 * structs copied); the upload and the launches run on a thread of the handle, so the calling thread is free to run the
 * _end -- Tier-2, download, sink -- of another handle meanwhile.  The frame the planes point to, and whatever `params`
 * points to (comment, ICC profile), stay BORROWED until the matching _end has returned; a failure of the deferred half
 * is reported by that _end.  Between the two calls every other entry point on this handle returns J2K_HIP_ERR_PARAM. */
int j2k_hip_encode_begin_borrowed(j2k_hip_encoder *enc, const j2k_hip_params *params, const j2k_hip_plane *planes);

/* Same, into a caller buffer. *out_len receives the codestream length (also on OVERFLOW). */
int j2k_hip_encode_to_buffer(j2k_hip_encoder *enc, const j2k_hip_params *params,
                             const j2k_hip_plane *planes, void *out, size_t out_cap, size_t *out_len);

/* Input already resident in HBM (planes[i].base are device pointers on the encoder's device).
 * The codestream stays on the device: *d_codestream (owned by the encoder, valid until the next
 * call on this handle) and *len.  If host_out != NULL it is also copied to the host. */
int j2k_hip_encode_device(j2k_hip_encoder *enc, const j2k_hip_params *params,
                          const j2k_hip_plane *planes, const void **d_codestream, size_t *len,
                          void *host_out, size_t host_cap);

/* Image sequence: nframes frames of identical geometry and coding parameters, all resident in HBM
 * (planes = nframes consecutive sets of `channels` planes), encoded in one call.  The frames share the
 * launches of the context modeller and of the MQ coder, so their serial coder chains run side by
 * side: this is what the frame loop of the reference's host (src/aftereffects/FrameSeq.cpp, one
 * WriteFile per frame) needs for small frames, whose encode time is one coder chain each.
 * d_codestreams[f] / lens[f] receive frame f's codestream (owned by the encoder, valid until the next
 * call on this handle); each is byte-identical to what j2k_hip_encode_device returns for that frame. */
int j2k_hip_encode_sequence_device(j2k_hip_encoder *enc, const j2k_hip_params *params,
                                   const j2k_hip_plane *planes, uint32_t nframes,
                                   const void **d_codestreams, size_t *lens);

/* Guard bits (j2k_hip_params.guard_bits).  j2k_hip_encode_get_guard_bits: the count in the QCD of the last file the handle
 * wrote -- of a sequence call its last frame's -- and 0 before any; a failed call leaves it alone.
 * j2k_hip_guard_bits_needed: host only, no handle (error text through j2k_hip_last_error(NULL)): the rule the encoder uses,
 * on per-block bit-plane counts in j2k_hip_debug_blocks order -- *g = max(floor, max over the blocks of numbps[i] -
 * exponent(band of block i) + 1), the floor being the count `params` ask for (0 = 2, J2K_HIP_GUARD_AUTO | floor alike).
 * J2K_HIP_ERR_OVERFLOW with the guard-bits text where that is more than 7 or gives a band more bit-planes than the reader
 * takes; J2K_HIP_ERR_PARAM where nblocks is not the frame's number of code-blocks. */
int j2k_hip_encode_get_guard_bits(const j2k_hip_encoder *enc, uint32_t *g);
int j2k_hip_guard_bits_needed(const j2k_hip_params *params, const uint32_t *numbps, size_t nblocks, uint32_t *g);

/* The rate-distortion slope thresholds the layers of tile `tile` (raster index, Isot) of the handle's last file were laid out
 * at (j2k_hip_params.layer_slopes): after a layer_rates, layer_psnr or dci_profile file the thresholds its search ended at,
 * -1 where a layer took everything that was left; after a layer_slopes file the thresholds it was given.  Of a sequence call:
 * its last frame's; of a tile-range call: the tiles of the range.  *n (optional) = the number of layers; out (optional)
 * receives min(cap, layers) entries.  Feeding them back as layer_slopes, tile by tile, writes the same tile bytes; a
 * single-tile file is reproduced byte for byte.  J2K_HIP_ERR_PARAM before any such file (a file without rate control has no
 * thresholds) or for a tile the last file does not have; a failed call leaves the record alone. */
int j2k_hip_encode_get_layer_slopes(const j2k_hip_encoder *enc, uint32_t tile, double *out, uint32_t cap, uint32_t *n);

/* --- a sequence to a byte budget: one slope threshold per shot, found on the device -----------------
 * The candidates are a fixed public grid, T(k) = ldexp(m[k mod 16], floor(k / 16)) for J2K_HIP_SLOPE_K_MIN <= k <=
 * J2K_HIP_SLOPE_K_MAX with m[j] = the double nearest 2^(j / 16) (mod and floor towards minus infinity), and
 * J2K_HIP_SLOPE_ALL for the threshold -1: everything that is left.  The integer order of the indices is the order of the
 * candidates, finest first.  j2k_hip_slope_grid: *t = T(k), -1.0 for J2K_HIP_SLOPE_ALL; J2K_HIP_ERR_PARAM outside the range.
 *
 * len_f(c) = the length of the file j2k_hip_encode_device writes of frame f under `params` with layers = 1 and
 * layer_slopes = { T(c) }.  total_bytes limits all files of the call together, frame_max_bytes any one of them; 0 = no limit.
 *   cap_f: J2K_HIP_SLOPE_ALL without frame_max_bytes; else len_f(cap_f) <= frame_max_bytes, and cap_f is J2K_HIP_SLOPE_ALL or
 *          len_f(cap_f - 1) > frame_max_bytes.
 *   c*:    with c_f(c) = max(c, cap_f): sum over f of len_f(c_f(c*)) <= total_bytes, and c* is J2K_HIP_SLOPE_ALL or the sum at
 *          c* - 1 is above total_bytes (without total_bytes: c* = J2K_HIP_SLOPE_ALL).
 * Frame f of the call is the file at c_f(c*), byte for byte.  File length is not a monotone function of the threshold, so such
 * boundaries need not be unique: any index with the property may be returned, the same one for the same input.
 * Where even J2K_HIP_SLOPE_K_MAX does not fit: J2K_HIP_ERR_OVERFLOW, the text naming the field (total_bytes / frame_max_bytes)
 * and the length at the coarsest candidate; nothing is written -- no output pointer, no length -- and the handle takes its next call.
 * Overflow goes by the search's walk: from where it stands it moves to coarser candidates until one fits and reports overflow
 * once J2K_HIP_SLOPE_K_MAX itself does not; as lengths need not fall with the index, that may be reported although some finer
 * index would have fitted by a few header bytes.  A successful call leaves no file above frame_max_bytes: a frame that exceeds it
 * at the shared index takes the next boundary at or above that index as its cap.
 * The search always runs on the device; the tuning knob rate_dev = -1 leaves the cut of the final layers to the host, over the
 * downloaded pass tables, as for layer_slopes -- the same files.
 *
 * j2k_hip_encode_sequence_budget_check (host only, no handle; text through j2k_hip_last_error(NULL)) refuses with
 * J2K_HIP_ERR_PARAM, the text naming the field, what the call refuses before any device work: layers other than 0 or 1;
 * layer_rates, layer_psnr, layer_slopes, dci_profile or cblk_style set; J2K_HIP_GUARD_AUTO (a re-plan would move the lengths the
 * search priced; a fixed count is fine); a struct_size that is not the struct's; flags other than 0; nframes == 0.
 * j2k_hip_encode_sequence_budget_device: the frames are resident, as for j2k_hip_encode_sequence_device, whose outputs these
 * are; frame_index (optional, nframes entries) receives c_f(c*), result (optional; struct_size set by the caller) what the
 * search did: curve_launches = launches of rate_curve_kernel, exact_plans = whole-frame plans beyond the one every frame needs.
 * Afterwards j2k_hip_encode_get_layer_slopes reports the last frame's threshold.
 * J2K_HIP_ABI_VERSION is still 9: functions and structs were added, none changed. */
#define J2K_HIP_SLOPE_K_MIN (-2048)
#define J2K_HIP_SLOPE_K_MAX 2047
#define J2K_HIP_SLOPE_ALL (-2049)
typedef struct j2k_hip_budget {
    uint32_t struct_size; /* sizeof(j2k_hip_budget) */
    uint32_t flags;       /* 0 */
    uint64_t total_bytes, frame_max_bytes;
} j2k_hip_budget;
typedef struct j2k_hip_budget_result {
    uint32_t struct_size; /* sizeof(j2k_hip_budget_result) */
    int32_t shared_index; /* c* */
    uint64_t total_bytes; /* of the files written */
    uint32_t capped_frames, curve_launches, exact_plans, reserved;
} j2k_hip_budget_result;
int j2k_hip_slope_grid(int32_t k, double *t);
int j2k_hip_encode_sequence_budget_check(const j2k_hip_params *params, uint32_t nframes, const j2k_hip_budget *budget);
int j2k_hip_encode_sequence_budget_device(j2k_hip_encoder *enc, const j2k_hip_params *params, const j2k_hip_plane *planes,
                                          uint32_t nframes, const j2k_hip_budget *budget, const void **d_codestreams,
                                          size_t *lens, int32_t *frame_index, j2k_hip_budget_result *result);
/* The same from host frames (planes = nframes consecutive sets of channel views in host memory), the files handed to one sink
 * per frame, users[f] with `write`, each front to back, frame 0 first.  No sink sees a byte before every frame's plan is final:
 * a budget that cannot be met, and every other refusal, leaves all of them untouched.  The handle keeps one input arena per
 * host frame of the largest such call it has served (nframes frames' worth of device memory) until j2k_hip_destroy. */
int j2k_hip_encode_sequence_budget(j2k_hip_encoder *enc, const j2k_hip_params *params, const j2k_hip_plane *planes,
                                   uint32_t nframes, const j2k_hip_budget *budget, j2k_hip_write_fn write, void *const *users,
                                   int32_t *frame_index, j2k_hip_budget_result *result);

/* --- tile-sharded encode (multi-GPU) -----------------------------------------------
 * Encode only tiles [tile_first, tile_first+tile_count) of the image (raster tile index, Isot).
 * Emits the tile-parts (SOT..data) of those tiles, in order, without main header or EOC, into the
 * device buffer; rank 0 concatenates main header + all ranks' tile-parts + EOC.
 * planes[] describe the WHOLE image (device pointers); only the rows/columns of the requested
 * tiles are read. */
int j2k_hip_encode_tiles_device(j2k_hip_encoder *enc, const j2k_hip_params *params,
                                const j2k_hip_plane *planes, uint32_t tile_first, uint32_t tile_count,
                                const void **d_tileparts, size_t *len, void *host_out, size_t host_cap);

/* The same from host buffers into a host buffer (planes[] describe the whole image in host memory; only the rows
 * of the requested tiles are uploaded).  *out_len receives the length (also on OVERFLOW). */
int j2k_hip_encode_tiles(j2k_hip_encoder *enc, const j2k_hip_params *params, const j2k_hip_plane *planes,
                         uint32_t tile_first, uint32_t tile_count, void *out, size_t out_cap, size_t *out_len);

/* --- one process, several GPUs ------------------------------------------------
 * Number of HIP devices this process sees (0 without a usable runtime). */
int j2k_hip_device_count(void);
/* Image sequence over several devices: frame f = planes[f * channels .. ] (host buffers, identical geometry and
 * parameters) goes to sink (write, users[f]) -- one output file per frame, like the reference's frame loop
 * (src/aftereffects/FrameSeq.cpp:1211-1372, one WriteFile per frame).  handles_per_device worker threads per
 * device (0 = 3), each with its own handle; frames are handed out in order, each sink is written by exactly one
 * thread, front to back.  Returns the first failure (text: j2k_hip_multi_last_error()). */
int j2k_hip_encode_batch(const int *devices, uint32_t num_devices, uint32_t handles_per_device,
                         const j2k_hip_params *params, const j2k_hip_plane *planes, uint32_t nframes,
                         j2k_hip_write_fn write, void *const *users);
/* One tiled image over several devices: contiguous blocks of tiles in raster order per device, the tile-parts
 * are put together on the host in tile order behind the main header ([JP2 boxes,] SOC..QCD, tile-parts, EOC) and
 * written to the sink sequentially.  The file is byte-identical to the single-device one. */
int j2k_hip_encode_tiles_distributed(const int *devices, uint32_t num_devices, const j2k_hip_params *params,
                                     const j2k_hip_plane *planes, j2k_hip_write_fn write, void *user);
const char *j2k_hip_multi_last_error(void);

/* Main header (SOC,SIZ,COD,QCD[,COM]) and number of tiles for `params`; no device needed.
 * Returns the header length through *len. */
int j2k_hip_main_header(const j2k_hip_params *params, void *out, size_t cap, size_t *len,
                        uint32_t *num_tiles);

/* File wrapper: every byte that precedes a codestream of `codestream_len` bytes in the output file --
 * the JP2 signature, file-type and header boxes plus the contiguous-codestream box header for
 * J2K_HIP_FMT_JP2 (what OpenJPEG's opj_jp2 writer produces for the reference's image description,
 * j2k_openjpeg_codec.cpp:613, :650-661), nothing for J2K_HIP_FMT_J2K.  The framed entry points
 * (j2k_hip_encode*, j2k_hip_encode_device) emit it themselves; a tile-sharded job calls this on
 * rank 0 once the total length is known.  No device needed. */
int j2k_hip_file_header(const j2k_hip_params *params, uint64_t codestream_len, void *out, size_t cap,
                        size_t *len);

/* --- decode --------------------------------------------------------------------
 * Replaces OpenJPEGCodec::GetFileInfo and ::ReadFile (reference: src/common/j2k_openjpeg_codec.cpp:222-426,
 * :451-586).  The caller hands over the whole file (raw codestream or JP2) in host memory -- what the
 * reference's stream callbacks (:81-120) pull out of its InputFile.  Supported: the files this library and the
 * reference's WriteFile produce, any of the five progression orders, quality layers, tiles, SOP/EPH markers,
 * user-defined precincts, image / tile grid origin offsets, components of up to 16 bits each (of up to 16 components the first
 * four are decoded, like the reference: src/common/j2k_openjpeg.cpp:278, :530) -- sub-sampled, signed or
 * of different depths (replicated / offset on the way out like the reference's CopyChannel); J2K_HIP_ERR_UNSUPPORTED
 * for: a component with coding parameters of its own (a COC that differs from COD), coding-style or quantisation
 * overrides in tile-part headers, a region-of-interest shift that takes a block beyond 30 bit-planes, code-blocks beyond 64 x 64, more than 16 components, more than 16 bits,
 * a palette beyond what the reference itself accepts (256 entries of 8 bits, three columns).
 * Decoded: every code-block style (bypass, reset, termall, vcausal, pterm, segsym), per-component quantisation (QCC),
 * progression order changes in the main header (POC: the 4K cinema profile), packed packet headers (PPM / PPT), regions of interest
 * (RGN, MAXSHIFT), TLM, several tile-parts per tile. */
typedef struct j2k_hip_file_info {
    uint32_t struct_size;        /* = sizeof(j2k_hip_file_info)                                          */
    uint32_t width, height;      /* FileInfo.width / .height (reference :294-295)                        */
    uint32_t channels, depth;    /* FileInfo.channels / .depth (:299-301)                                */
    uint32_t reversible;         /* settings.reversible (:357)                                           */
    uint32_t ycc;                /* multiple component transform in use                                  */
    uint32_t layers, num_resolutions, tile_width, tile_height, progression;
    uint32_t file_format;        /* J2K_HIP_FMT_J2K / J2K_HIP_FMT_JP2 (:292)                             */
    uint32_t color_space;        /* J2K_HIP_CS_* from the colr box's EnumCS (:318-330); UNSPECIFIED with ICC */
    uint32_t alpha;              /* 0 = none; k + 1 = channel k is opacity (cdef box, :359-377)          */
    uint32_t alpha_premultiplied;
    size_t icc_profile_offset;   /* restricted ICC profile inside the file (colr method 2, :333-351):    */
    size_t icc_profile_len;      /*    bytes [offset, offset + len) of `file`; 0 = none                  */
    /* per component (ABI 7): FileInfo.subsampling[i] (:304-317), and the component's own depth / sign where they differ
     * from `depth` (the reference reports comps[0].prec only, :301).  The decode replicates a sub-sampled component's
     * samples onto the destination channel's full grid and maps a signed one to unsigned like CopyChannel does. */
    uint32_t sub_x[4], sub_y[4], comp_depth[4], comp_signed[4];
    /* palette (ABI 9; JP2 pclr + cmap boxes): FileInfo.LUTsize / .LUT / .LUTmap (reference :362-401).  lut_size = 0: none.
     * Otherwise the codestream's single component holds indices -- j2k_hip_decode delivers them, as the reference's ReadFile
     * does (OPJ_DPARAMETERS_IGNORE_PALETTE_FLAG, :503) -- and output channel i of a pixel is lut[index][lut_column[i]].
     * Supported like the reference accepts it: at most 256 entries of 8 bits in three columns, every channel mapped from
     * component 0; anything else is J2K_HIP_ERR_UNSUPPORTED (the host's other reader takes the file). */
    uint32_t lut_size, lut_channels;
    uint8_t lut[256][4];
    uint8_t lut_column[4];
} j2k_hip_file_info;
/* Header only; no device needed.  info->struct_size must be set by the caller. */
int j2k_hip_read_info(const void *file, size_t len, j2k_hip_file_info *info);

/* One destination channel = a faithful image of the j2k::Channel the host passes in its Buffer (reference:
 * src/common/j2k_codec.h:221-247): a borrowed, strided view that is written.  Only the channel's samples are
 * written, like Codec::CopyBuffer (src/common/j2k_codec.cpp:402-427) does; width/height = Channel.width/.height
 * decide how much is copied (:496-499).
 * Float destinations: sample_bits == 32 means IEEE binary32 samples of nominal range 0..1, depth the integer depth d (1..16)
 * they stand for, base / colbytes / rowbytes multiples of 4 (anything else: J2K_HIP_ERR_PARAM before any device work).  The
 * integer ov of depth d is computed exactly as for an integer destination -- component samples, colour conversion,
 * palette, CopyChannel's depth conversion, the alpha fill -- and stored as (float)ov / (float)(2^d - 1), a correctly
 * rounded division; the highest value gives exactly 1.0f.  (A palette entry widens to 16 bits, b * 257, for d > 8, as it
 * does for 16-bit samples.)  This holds for every decode entry point, the four planes of j2k_hip_rgba_dst included; there
 * demote_ae16 (d == 16) stores (float)Demote(ov) / 32768.0f -- what the reference's DemoteWorld and its ARGB64 -> ARGB128
 * copy leave (src/aftereffects/FrameSeq.cpp:82-86, :211-216) -- and the opaque alpha fill is exactly 1.0f.  Outside
 * j2k_hip_rgba_dst, float and integer channels may mix in one call.  The 9/7 path still rounds to integers first: the floats
 * are those of libopenjp2's samples. */
typedef struct j2k_hip_outplane {
    void *base;
    ptrdiff_t colbytes, rowbytes;
    uint32_t sample_bits;        /* 8 (UCHAR), 16 (USHORT) or 32 (IEEE float, see above)                 */
    uint32_t depth;              /* Channel.depth: the decoded precision is converted to it like CopyChannel */
    uint32_t width, height;
} j2k_hip_outplane;
/* Decode at 1/subsample of the size (subsample = 1, 2, 4 ...: cp_reduce = log2(subsample), :501): the image of
 * ceil(width / subsample) x ceil(height / subsample) goes to the top-left of the destination channels.
 * planes[i] receives codestream component i (after the inverse colour transform: R,G,B[,A]).
 * A file cut short (its write was aborted) decodes what is there, in every decode entry point and in j2k_hip_compare:
 *  - a cut inside a tile-part: the whole code-block contributions that arrived are decoded -- a packet whose header or
 *    whose body is cut keeps the contributions in front of the cut -- and everything else of the tile is zero coefficients
 *    (libopenjp2 2.4 / 2.5 refuse such a file: "Tile part length size inconsistent with stream length");
 *  - whole tile-parts missing, with or without an EOC: decoded as libopenjp2 decodes them.  The samples of a tile of which
 *    no tile-part arrived are component value 0 (not the mid level a tile of zero coefficients decodes to), and every
 *    conversion behind it -- signed offset, depth, colour, palette, float -- runs on that 0;
 *  - a cut in front of the first SOD, or inside a later tile-part's SOT .. SOD: J2K_HIP_ERR_PARAM. */
int j2k_hip_decode(j2k_hip_encoder *enc, const void *file, size_t len, uint32_t subsample,
                   const j2k_hip_outplane *planes, uint32_t nplanes);
/* Same with destination channels in device memory (planes[i].base are device pointers). */
int j2k_hip_decode_device(j2k_hip_encoder *enc, const void *file, size_t len, uint32_t subsample,
                          const j2k_hip_outplane *planes, uint32_t nplanes);

/* Decode a window of the image.  `region` is in pixels of the image as j2k_hip_decode delivers it at this `subsample`:
 * the reduced image with its top-left at (0, 0), whatever image or tile origin the file has.  Destination channel i
 * receives, at its top-left, exactly the samples j2k_hip_decode with the same arguments would have put at
 * [y, y + h) x [x, x + w).  Everything else is j2k_hip_decode's: planes[i].width / .height limit what is copied, only
 * channel samples are written, sub-sampled components are replicated (at the phase of the window's origin), signed ones
 * offset, depths converted, palettes left as indices, the first four components decoded.
 * What is skipped: code-blocks whose coefficients the window's synthesis does not read are neither gathered nor decoded
 * (j2k_hip_stats.num_codeblocks counts the ones that were), and the inverse DWT produces, per resolution, only the window
 * the next resolution needs.  What is not: every packet header is parsed (they are one serial bit stream), the whole file
 * is uploaded, and the coefficient planes keep the image's size and are cleared.
 * region == NULL: j2k_hip_decode itself.  w == 0, h == 0 or a rectangle that leaves the reduced image:
 * J2K_HIP_ERR_PARAM, nothing written.  J2K_HIP_ABI_VERSION is still 9: functions were added, none changed. */
typedef struct j2k_hip_rect { uint32_t x, y, w, h; } j2k_hip_rect;
int j2k_hip_decode_region(j2k_hip_encoder *enc, const void *file, size_t len, uint32_t subsample,
                          const j2k_hip_rect *region, const j2k_hip_outplane *planes, uint32_t nplanes);
/* Same with destination channels in device memory (planes[i].base are device pointers). */
int j2k_hip_decode_region_device(j2k_hip_encoder *enc, const void *file, size_t len, uint32_t subsample,
                                 const j2k_hip_rect *region, const j2k_hip_outplane *planes, uint32_t nplanes);
/* Which band coefficients a window needs: for one plane of width x height at origin (x0, y0) with `levels` decompositions,
 * rects[0] = LL, then HL, LH, HH per level from the lowest resolution up (3 * levels + 1 rects, in band coordinates of the
 * Mallat layout the stage hooks use: x, y index the plane itself, so rects[k] is the part of the plane that is read).  A
 * band nothing is read from has w == h == 0.  `window` is in plane coordinates.  The rectangles are what the inverse DWT
 * kernels read, never less: outputs are produced in (even, odd) pairs of absolute positions, and a pair reads 5 (5/3) or
 * 9 (9/7) interleaved positions around it.  Window empty or outside the plane, nrects < 3 * levels + 1: J2K_HIP_ERR_PARAM
 * (message: j2k_hip_last_error(NULL)).  No device needed. */
int j2k_hip_region_footprint(int reversible, uint32_t width, uint32_t height, uint32_t levels, uint32_t x0, uint32_t y0,
                             const j2k_hip_rect *window, j2k_hip_rect *rects, uint32_t nrects);

/* --- decode straight to R, G, B, A ----------------------------------------------------------------
 * What RGBAinputFile::ReadFile (reference: src/common/j2k_rgba_file.cpp:450-735) does on the CPU after Codec::ReadFile --
 * sYCC -> RGB, grey into three channels, the palette look-up, the alpha fill -- and the DemoteWorld pass of
 * j2k_DrawSparseFrame (src/aftereffects/j2k.cpp:482-492), done by the decode's output kernel instead.
 *
 * j2k_hip_rgba_mode: how a file's components become R, G, B, A; header only, no device needed.  n = min(channels, 4);
 * the rules in order:
 *   what j2k_hip_read_info refuses is refused the same way (same status, same text);
 *   PALETTE  a palette is present (then n == 1): R / G / B = the palette column c whose lut_column[c] is 0 / 1 / 2 (the
 *            column HipCodec::GetFileInfo reports as LUTmap[c] = RED / GREEN / BLUE; without one, column 0 / 1 / 2); a
 *            fourth column is ignored;
 *   GREY     n is 1 or 2, colour space grey or unspecified (ICC included): component 0 -> R, G and B, component 1 -> A;
 *   SYCC     colour space sYCC, n >= 3: components 0, 1, 2 are Y, Cb, Cr; a fourth component is not read, A is filled;
 *   RGB      n >= 3, colour space sRGB or unspecified (ICC included): components 0, 1, 2 -> R, G, B, component 3 -> A;
 *   anything else (CMYK, e-sYCC, one or two channels in a colour space that is not grey ...) is J2K_HIP_ERR_UNSUPPORTED with a
 *   text that names the colour space -- the reference's own code asserts there; the host takes its old path.  So is an
 *   opacity channel that the cdef box declares anywhere but last (alpha not 0 and not n) in the GREY and RGB modes. */
enum { J2K_HIP_RGBA_RGB = 1, J2K_HIP_RGBA_GREY = 2, J2K_HIP_RGBA_PALETTE = 3, J2K_HIP_RGBA_SYCC = 4 };
int j2k_hip_rgba_mode(const void *file, size_t len, uint32_t *mode);

/* The four destination channels.  They share sample_bits (8, 16 or 32 = float: j2k_hip_outplane) and depth D (1 <= D <=
 * sample_bits; float: 1 <= D <= 16).  Per pixel:
 *   1. component samples exactly as j2k_hip_decode delivers them at depth D (replication of sub-sampled components,
 *      inverse RCT / ICT, DC shift, clamp, CopyChannel's depth conversion);
 *   2. RGB: R, G, B[, A] = v0, v1, v2[, v3].  GREY: R = G = B = v0[, A = v1].
 *      PALETTE: idx = component 0 at its own precision; e = idx < lut_size ? lut[idx] : {0, 0, 0}; a channel is its column
 *      of e for 8-bit samples and (e << 8) | e for 16-bit samples, whatever D is (ConvertToType, :57-70).
 *      SYCC, with h = 1 << (D - 1) and sY = v0 - h, sCb = v1 - h, sCr = v2 - h, in float, every operation rounded on its
 *      own (no fused multiply-add), the reference's irreversible branch (:185-278, :392):
 *          fR = sY + 1.402f * sCr;  fG = (sY - kCrG * sCr) - kCbG * sCb;  fB = sY + 1.772f * sCb
 *          channel = clamp((int)((f + h) + 0.5f), 0, 2^D - 1)                          (the cast truncates)
 *      kCrG = (float)(2 * 0.299 * (1 - 0.299) / 0.587), kCbG = (float)(2 * 0.114 * (1 - 0.114) / 0.587);
 *   3. a mode that delivers no A fills it with 2^D - 1 (the reference narrows that value to 8 bits first, :416, so a
 *      16-bit world gets 255 there: deliberately not reproduced);
 *   4. demote_ae16: every channel, the filled A included, leaves as v > 32768 ? ((v - 1) >> 1) + 1 : v >> 1 (Demote,
 *      src/aftereffects/FrameSeq.cpp:265-268); needs sample_bits == 16 or 32 and D == 16;
 *   5. only samples of the given channels are written; a.base == NULL: no alpha wanted.  Four channels that are the four
 *      samples of one pixel record (A,R,G,B or R,G,B,A interleaved, record-aligned) leave as one store per pixel (an
 *      ARGB128 pixel: one 16-byte store).
 * Width, height, subsample and region are j2k_hip_decode's / j2k_hip_decode_region's (region == NULL: the whole image).
 * Refused before any device work, nothing written: J2K_HIP_ERR_PARAM for a bad struct_size, a NULL r / g / b, channels of
 * unlike sample_bits or depth, demote_ae16 without 16-bit or float samples of depth 16, a bad region; J2K_HIP_ERR_UNSUPPORTED for
 * what j2k_hip_rgba_mode does not classify.  J2K_HIP_ABI_VERSION is still 9: functions were added, none changed. */
typedef struct j2k_hip_rgba_dst {
    uint32_t struct_size;
    j2k_hip_outplane r, g, b, a;
    uint32_t demote_ae16;
} j2k_hip_rgba_dst;
int j2k_hip_decode_rgba(j2k_hip_encoder *enc, const void *file, size_t len, uint32_t subsample,
                        const j2k_hip_rect *region, const j2k_hip_rgba_dst *dst);
/* Same with destination channels in device memory. */
int j2k_hip_decode_rgba_device(j2k_hip_encoder *enc, const void *file, size_t len, uint32_t subsample,
                               const j2k_hip_rect *region, const j2k_hip_rgba_dst *dst);

/* --- decode an image sequence in one call ---------------------------------------------------------
 * The frames of one call share their launches: one gather, one Tier-1 launch (pair), one inverse DWT launch pair per
 * resolution and one output launch serve the code-blocks of all of them, from one host thread on the handle's one stream,
 * whatever GPU_MAX_HW_QUEUES is.  (A long call is cut into groups of consecutive frames whose lane waves the chip holds at
 * once and whose arenas fit a share of the free device memory; a group is what shares launches.)
 *
 * Output: frame f goes to planes[f * nplanes + i] (i < nplanes) or dsts[f], and every destination receives exactly what
 * j2k_hip_decode_region / j2k_hip_decode_rgba with the same subsample, region and destination would have written for
 * files[f] -- region == NULL: the whole image; sub-sampled, signed and mixed-depth components, palettes, code-block styles,
 * files cut short (j2k_hip_decode: a missing tile is component value 0 in its own frame, whatever its neighbours hold) and
 * the first four of sixteen components included.  Only channel samples are written.  Destinations of
 * different frames may be pieces of one buffer but must not overlap.  Channel i has the same sample_bits and depth in every
 * frame (RGBA: also the same demote_ae16, and an alpha destination in all frames or in none); bases, strides and extents are
 * each frame's own.
 * The frames must match: identical SIZ (geometry, components, their depths, signs and sub-sampling), COD (levels,
 * code-blocks, style, wavelet, MCT, precincts, progression, layers), QCD / QCC values, RGN and POC, and for the RGBA calls
 * the colour space, the opacity channel and the palette.  COM, TLM, the tile-part structure, PPM / PPT, SOP / EPH and JP2
 * boxes that do not enter the decode may differ.
 * Refused before any device work, nothing written, the text beginning with "frame k: ": J2K_HIP_ERR_PARAM for nframes == 0
 * (k = 0), a NULL or empty file, a frame that differs from frame 0, a bad region, a bad destination;
 * J2K_HIP_ERR_UNSUPPORTED for a file that j2k_hip_read_info (RGBA calls: j2k_hip_rgba_mode) does not take.
 * j2k_hip_decode_sequence_check does the header part of that alone -- no device, no handle; *bad_frame (optional) receives
 * k, the text is j2k_hip_last_error(NULL)'s -- so that a host can sort its files into calls beforehand.
 * A frame whose headers are sound but whose packets turn out malformed fails the call with that frame's status and
 * "frame k: "; frames before it may have been written by then (those of the groups that had completed), frame k and the
 * frames behind it have not.
 * nframes == 1 gives the single-frame call's output (which Tier-1 kernel runs may differ from the single-frame choice: the
 * choice sees the blocks of all frames of a group).  j2k_hip_stats after the call holds sums over the frames;
 * num_codeblocks counts the blocks decoded, ms_total is the call's wall time.
 * J2K_HIP_ABI_VERSION is still 9: functions were added, none changed. */
typedef struct j2k_hip_file { const void *data; size_t len; } j2k_hip_file;
int j2k_hip_decode_sequence_check(const j2k_hip_file *files, uint32_t nframes, uint32_t *bad_frame);
int j2k_hip_decode_sequence(j2k_hip_encoder *enc, const j2k_hip_file *files, uint32_t nframes, uint32_t subsample,
                            const j2k_hip_rect *region, const j2k_hip_outplane *planes, uint32_t nplanes);
/* Same with destination channels in device memory (planes[].base are device pointers). */
int j2k_hip_decode_sequence_device(j2k_hip_encoder *enc, const j2k_hip_file *files, uint32_t nframes, uint32_t subsample,
                                   const j2k_hip_rect *region, const j2k_hip_outplane *planes, uint32_t nplanes);
int j2k_hip_decode_rgba_sequence(j2k_hip_encoder *enc, const j2k_hip_file *files, uint32_t nframes, uint32_t subsample,
                                 const j2k_hip_rect *region, const j2k_hip_rgba_dst *dsts);
/* Same with destination channels in device memory. */
int j2k_hip_decode_rgba_sequence_device(j2k_hip_encoder *enc, const j2k_hip_file *files, uint32_t nframes, uint32_t subsample,
                                        const j2k_hip_rect *region, const j2k_hip_rgba_dst *dsts);

/* --- decode only the first quality layers of a file -------------------------------------------------
 * A property of the handle, as decoder parameters are of libopenjp2's codec (opj_dparameters_t::cp_layer): max_layers = 0
 * (the initial value) decodes every layer; L >= 1 makes every decode call on the handle -- j2k_hip_decode[_device],
 * _decode_region[_device], _decode_rgba[_device], _decode_sequence[_device] and _decode_rgba_sequence[_device], all frames
 * of a sequence call alike -- deliver, sample for sample, what it would deliver for the file that holds only the first L
 * layers: the codestream with every packet of layer index >= L removed, COD's layer count set to L and the tile-part
 * lengths fixed up.  The setting is sticky until it is set again.
 * What happens: every packet header is still parsed (the headers are one serial bit stream whose inclusion, length and
 * segment state advance with every layer), the contributions of layers >= L are dropped, a code-block keeps the coding
 * passes and bytes of the layers below L, and one first included in a later layer stays all zero.  Under the bypass and
 * termall styles the segments handed to Tier-1 list the kept passes and bytes only (the last may hold fewer passes than it
 * has room for; bytes past the kept ones read 0xFF, as for a file cut short).  Files with POC are filtered the same way.
 * L equal to the file's layer count, or larger, is the decode of 0: the same launches, tables and bytes.  A malformed file is
 * malformed whatever L is.  Tier-1 time follows the coding passes that remain (j2k_hip_debug_decode_work).
 * enc == NULL: J2K_HIP_ERR_PARAM; between j2k_hip_encode_begin_borrowed and its _end both calls are refused like every
 * other.  j2k_hip_read_info, j2k_hip_rgba_mode and j2k_hip_decode_sequence_check take no handle and are unaffected.
 * J2K_HIP_ABI_VERSION is still 9: functions were added, none changed. */
int j2k_hip_decode_set_max_layers(j2k_hip_encoder *enc, uint32_t max_layers);
int j2k_hip_decode_get_max_layers(const j2k_hip_encoder *enc, uint32_t *max_layers);

/* --- cinema frames to R'G'B': X'Y'Z' code values to RGB in the RGBA output kernel ---------------------------
 * A DCI codestream carries no colour space, so j2k_hip_rgba_mode classifies a cinema frame as plain RGB and the RGBA calls
 * deliver its X'Y'Z' code values as R, G, B.  xyz_to_rgb, a property of the handle like max_layers (sticky until set again,
 * initially 0), makes j2k_hip_decode_rgba[_device] and j2k_hip_decode_rgba_sequence[_device] -- region and subsample
 * included -- convert them in the output kernel: the inverse of j2k_hip_params.rgb_to_xyz.  target:
 *     0  off: every byte and launch is what it was without the setting
 *     1  sRGB (IEC 61966-2-1 piecewise curve, Rec.709 primaries, D65)
 *     2  Rec.709 primaries under a pure 2.4 power (BT.1886)
 *     3  Rec.709 primaries, linear light
 * -- the three codings of rgb_to_xyz, with its EOTF_1..3.  It applies to mode J2K_HIP_RGBA_RGB only.  A destination pixel, to
 * the rounding:
 *   1. c_i (i = 0..2) = the component sample at the component's own precision P: what j2k_hip_decode delivers at depth P
 *      (replication of sub-sampled components, inverse RCT / ICT, DC shift, clamp to 0 .. 2^P - 1), NOT converted to the
 *      destination's depth first.  Components 0..2 must be unsigned and share P (1..16).
 *      l_i = dl[c_i],  dl[c] = (float)pow((double)c / (2^P - 1), 2.6), a table of 2^P binary32 values computed on the host in double.
 *   2. N_ij = (float)((double)n_ij * (52.37 / 48.0)), n = the XYZ -> linear Rec.709 (D65) matrix, no chromatic adaptation:
 *          3.2404542 -1.5371385 -0.4985314 / -0.9692660 1.8760108 0.0415560 / 0.0556434 -0.2040259 1.0572252
 *      r = fadd(fadd(fmul(N00, l_X), fmul(N01, l_Y)), fmul(N02, l_Z)): every product and sum rounded to binary32 on its own,
 *      nothing contracted to an FMA; g and b alike from rows 1 and 2.
 *   3. D = the destination's depth, top = 2^D - 1, othr[k] = (float)EOTF_target(((double)k - 0.5) / top) for k = 1..top (strictly
 *      increasing in binary32 for every target and depth); the channel is the number of k with othr[k] <= r -- round-to-nearest
 *      of top * OETF(r), decided on thresholds: no transcendental function decides a code on the device.  A negative r (a
 *      colour outside the Rec.709 gamut) gives 0, r >= othr[top] gives top.
 *   4. Everything else is the RGB mode's: a fourth component is A through the depth conversion, without one A is filled with
 *      top; demote_ae16 and the float store ((float)v / (2^D - 1)) follow as without the setting.
 * j2k_hip_xyz_inverse_tables hands out dl, othr and N as the kernel gets them.  The way there and back is not the identity:
 * 12-bit codes under a 2.6 power are coarser in the dark than an 8-bit sRGB or 2.4 code (DESIGN.md has the measured errors).
 * J2K_HIP_ERR_PARAM, the text naming xyz_to_rgb, nothing changed: a target above 3; enc == NULL (the text through
 * j2k_hip_last_error(NULL)); between j2k_hip_encode_begin_borrowed and its _end.  With the setting non-zero the RGBA calls
 * refuse, with J2K_HIP_ERR_PARAM naming xyz_to_rgb, before any device work and with nothing written: a file whose mode is GREY,
 * PALETTE or SYCC; components 0..2 that are signed or of unlike precision.  The planar decode calls and j2k_hip_compare ignore
 * the setting.
 * j2k_hip_read_profile: Rsiz of the codestream's SIZ segment, from the headers alone (no handle, no device; failures as
 * j2k_hip_read_info's): 3 and 4 are the 2K and 4K digital cinema profiles -- the one mark a DCI frame carries, for a host
 * that wants to convert such files only.  Nothing decodes by it.
 * J2K_HIP_ABI_VERSION is still 9: functions were added, none changed. */
int j2k_hip_decode_set_xyz_to_rgb(j2k_hip_encoder *enc, uint32_t target);
int j2k_hip_decode_get_xyz_to_rgb(const j2k_hip_encoder *enc, uint32_t *target);
int j2k_hip_read_profile(const void *file, size_t len, uint32_t *rsiz);

/* --- compare a file with its source frame ------------------------------------------------------------
 * What did a file lose?  The source frame is given exactly as j2k_hip_encode takes it (params + planes), the file is decoded
 * as j2k_hip_decode decodes it (subsample 1, the handle's max_layers), and both stay on the device: only the file goes up and
 * only the results come down.  For every component c < params->channels, on the component's own grid of
 * ceil(width / sub_x) x ceil(height / sub_y) samples:
 *   S_c(x, y)  the unsigned integer of params->depth bits that the encode's front end makes of the planes, before the DC shift
 *              and before any RCT / ICT: promote_ae16, the float quantisation of j2k_hip_plane, CopyChannel's depth conversion,
 *              and with rgb_to_sycc the integer Y / Cb / Cr formula of j2k_hip_params with its decimation; with rgb_to_xyz
 *              the X'Y'Z' code of j2k_hip_params for channels 0..2 (a fourth channel as without it);
 *   D_c(x, y)  what j2k_hip_decode delivers for component c at the file's own depth; for a sub-sampled component the delivered
 *              sample at (x * sub_x, y * sub_y) (the decode replicates: that is the component's own sample);
 *   e = D - S, per sample.
 * j2k_hip_diff, one per component (struct_size set by the caller in every element): samples = the grid's size; differing = the
 * samples with e != 0; sum_abs, sum_sq, max_abs over |e|, e^2; (first_x, first_y) = the first differing sample in raster order
 * on the component's grid, both 0 when differing == 0.  These are exact integers, whatever order the device sums in.  The two
 * doubles are made on the host from them: mse = (double)sum_sq / (double)samples, psnr = 10 * log10((top * top) / mse) with
 * top = (double)(2^depth - 1), and +infinity when sum_sq == 0.  min(ndiffs, channels) elements are written.
 * The file must describe the image of `params`: the same width, height, number of components (of more than four the first
 * four count, as for the decode) and sub-sampling factors, unsigned components, every compared component of params->depth
 * bits; anything else is J2K_HIP_ERR_PARAM, the text naming the field, before any device work and with nothing written.  So is
 * a component of 2^32 samples or more (sum_sq could not hold it).  A file the decoder does not read stays
 * J2K_HIP_ERR_UNSUPPORTED and a malformed one J2K_HIP_ERR_PARAM, both with j2k_hip_read_info's texts; a file cut short
 * compares what decodes; a handle with an encode pending refuses as j2k_hip_decode does.  Only the fields of `params` that
 * define the source samples and the geometry count -- width, height, channels, depth, promote_ae16, comp_sub_x / _y,
 * rgb_to_sycc, rgb_to_xyz; the coding fields (wavelet, ycc, layers, tiles, precincts, style, rates, profile, wrapper) are not read.
 * j2k_hip_compare: planes in host memory.  j2k_hip_compare_device: planes[i].base are device pointers and the image never
 * crosses the bus.  j2k_hip_compare_check: the agreement test above alone -- no handle, no device, the text through
 * j2k_hip_last_error(NULL); both calls run it first.
 * J2K_HIP_ABI_VERSION is still 9: functions and a struct were added, none changed. */
typedef struct j2k_hip_diff {
    uint32_t struct_size;    /* = sizeof(j2k_hip_diff) */
    uint32_t max_abs;
    uint64_t samples, differing, sum_abs, sum_sq;
    uint32_t first_x, first_y;
    double mse, psnr;
} j2k_hip_diff;
int j2k_hip_compare_check(const j2k_hip_params *params, const void *file, size_t len);
int j2k_hip_compare(j2k_hip_encoder *enc, const j2k_hip_params *params, const j2k_hip_plane *planes, const void *file, size_t len,
                    j2k_hip_diff *diffs, uint32_t ndiffs);
int j2k_hip_compare_device(j2k_hip_encoder *enc, const j2k_hip_params *params, const j2k_hip_plane *planes, const void *file,
                           size_t len, j2k_hip_diff *diffs, uint32_t ndiffs);

/* --- the tables of rgb_to_xyz -------------------------------------------------------------------------
 * What the cinema colour front end (j2k_hip_params.rgb_to_xyz) looks its values up in, as the kernel gets them: no handle and
 * no device needed.  source = 1..3 as rgb_to_xyz; lin receives 2^src_depth values (lin[v]), thr 2^dst_depth - 1 values
 * (thr[c - 1] = the threshold of code c, c = 1 .. 2^dst_depth - 1), matrix the nine M_ij row by row.  A NULL output is
 * skipped.  J2K_HIP_ERR_PARAM for a source outside 1..3 or a depth outside 1..16.
 * J2K_HIP_ABI_VERSION is still 9: a function was added, none changed. */
int j2k_hip_xyz_tables(uint32_t source, uint32_t src_depth, uint32_t dst_depth, float *lin, float *thr, float matrix[9]);
/* The tables of the way back (j2k_hip_decode_set_xyz_to_rgb), alike: target = 1..3; dl receives 2^comp_depth values (dl[c]), othr
 * 2^dst_depth - 1 values (othr[k - 1] = the threshold of code k, k = 1 .. 2^dst_depth - 1), matrix the nine N_ij row by row.  A
 * NULL output is skipped.  J2K_HIP_ERR_PARAM for a target outside 1..3 or a depth outside 1..16.
 * J2K_HIP_ABI_VERSION is still 9: a function was added, none changed. */
int j2k_hip_xyz_inverse_tables(uint32_t target, uint32_t comp_depth, uint32_t dst_depth, float *dl, float *othr, float matrix[9]);

/* --- stage-level entry points (parity tests and roofline measurement call these) -----------------
 * A1+A2+A4+A5: front end only. d_out = channels planes of width*height 32-bit words (int32 for
 * reversible, float32 bit patterns otherwise), row stride = width.  With sub-sampled components (comp_sub_x / _y,
 * rgb_to_sycc) the components follow one another, each dense at its own size ceil(width / sub_x) x ceil(height / sub_y).
 * rgb_to_xyz is honoured: channels 0..2 come out as X'Y'Z' codes minus the DC shift (then the RCT / ICT with ycc).
 * An encode pending on the handle (j2k_hip_encode_begin without its _end): J2K_HIP_ERR_PARAM, nothing of the handle is touched. */
int j2k_hip_stage_frontend(j2k_hip_encoder *enc, const j2k_hip_params *params,
                           const j2k_hip_plane *planes_device, void *d_out);
/* A6: forward DWT of `nplanes` planes of width*height 32-bit words (row stride = width), in the
 * Mallat layout of the oracle, origin (x0,y0).  d_in is preserved; d_out receives the result.
 * `repeat` > 1 re-runs the transform (for timing); *ms (optional) = mean device time per run.
 * An encode pending on the handle: J2K_HIP_ERR_PARAM, its job table and planes stay as they are. */
int j2k_hip_stage_dwt(j2k_hip_encoder *enc, int reversible, uint32_t width, uint32_t height,
                      uint32_t nplanes, uint32_t levels, uint32_t x0, uint32_t y0, const void *d_in,
                      void *d_out, uint32_t repeat, double *ms);
/* The region form of j2k_hip_stage_dwt (the mirror of the region form of j2k_hip_stage_idwt, whose j2k_hip_idwt_region it
 * takes): every plane holds `nregions` sub-rectangles (x, y, w, h), each transformed on its own into a Mallat layout of its
 * own with its own origin (x0, y0) -- the tiles of a tiled component.  Per level every (plane, region) is one job of the same
 * launch: sizes, lifting parities and word offsets differ from job to job, and the launch is sized by the largest.  A region
 * of which nothing is left at a level (a single odd-phase sample is all high-pass) takes no part from there on.  The regions
 * must be non-empty, lie inside the plane and not overlap, nregions >= 1, levels <= 32, no encode pending on the handle:
 * J2K_HIP_ERR_PARAM otherwise.  d_in is preserved; d_out receives the coefficients, and the words outside every region are
 * copied from d_in.  The handle's cached geometry is dropped: the next encode builds it again.
 * J2K_HIP_ABI_VERSION is still 9: a function was added, none changed. */
struct j2k_hip_idwt_region;
int j2k_hip_stage_dwt_regions(j2k_hip_encoder *enc, int reversible, uint32_t width, uint32_t height,
                              uint32_t nplanes, uint32_t levels, const struct j2k_hip_idwt_region *regions,
                              uint32_t nregions, const void *d_in, void *d_out);
/* A1..A6 as an encode runs them: the front end and every DWT launch of j2k_hip_encode_device for these parameters and
 * channel views (device pointers) -- the same geometry and job tables, the same choice between the fused level-1 kernel and
 * the stand-alone front end, the same launch shapes under the tuning knobs -- and nothing behind them: no Tier-1 launch,
 * no pending encode on the handle.  d_out (device) receives the `channels` coefficient planes, dense, width*height 32-bit
 * words each (int32 for the reversible path, float32 bit patterns otherwise): every tile's rectangle holds that
 * tile-component's Mallat layout; with one resolution it is the front end's output.  With sub-sampled components
 * (comp_sub_x / _y, rgb_to_sycc) the planes follow one another, each dense at its own size, as j2k_hip_stage_frontend's.
 * Row-pair ranges: level l (0 = full resolution) of the first `ncut_levels` levels is launched once per interval
 * [0, c_1), [c_1, c_2), .., [c_n, end) of its row pairs, n = ncuts[l], the intervals in ascending or (descending != 0)
 * descending order; `cuts` holds the c_i of level 0, then those of level 1, and so on.  A level still starts after the whole
 * level above it.  A cut point that does not exceed the one before it, or is 0, or lies at or beyond the row pairs of the
 * level's tallest tile-component ((height + parity of its origin + 1) / 2): J2K_HIP_ERR_PARAM.  cuts == NULL with
 * ncut_levels == 0: one launch per level, as an encode.
 * The handle's cached geometry is dropped: the next encode builds it again.
 * J2K_HIP_ABI_VERSION is still 9: a function was added, none changed. */
int j2k_hip_stage_transform(j2k_hip_encoder *enc, const j2k_hip_params *params, const j2k_hip_plane *planes_device,
                            const uint32_t *cuts, const uint32_t *ncuts, uint32_t ncut_levels, int descending,
                            void *d_out);
/* A7+A8: Tier-1 of `nblocks` code-blocks cut from one coefficient plane (row stride `stride`
 * words). Block i = rectangle (bx[i],by[i],bw[i],bh[i]), orientation orient[i], band step size
 * stepsize[i] (ignored when reversible).  Outputs (host): numbps[i], npasses[i], length[i] and the
 * concatenated codewords in `data` (offsets[i] = start of block i).  Rectangles must not overlap:
 * the kernel rewrites each block of d_coef in place as scaled magnitudes (d_coef is scratch).
 * An encode pending on the handle: J2K_HIP_ERR_PARAM (j2k_hip_stage_t1_passes and _styled alike) -- the pending frame's
 * coder streams still read the block table and the Tier-1 arenas this call would overwrite. */
int j2k_hip_stage_t1(j2k_hip_encoder *enc, int reversible, void *d_coef, uint32_t stride,
                     uint32_t nblocks, const uint32_t *bx, const uint32_t *by, const uint32_t *bw,
                     const uint32_t *bh, const uint32_t *orient, const float *stepsize,
                     uint32_t *numbps, uint32_t *npasses, uint32_t *length, uint64_t *offsets,
                     void *data, size_t data_cap);

/* Same as j2k_hip_stage_t1, additionally returning what rate control needs per coding pass
 * (row i = block i, J2K_HIP_MAX_PASSES columns): pass_rate = cumulative codeword bytes after the
 * reference's fix-ups (estimate = bytes + 3, never decreasing towards the end, never ending a pass
 * on 0xFF), pass_dist = the pass's integer distortion-LUT sum (OpenJPEG's nmsedec). */
#define J2K_HIP_MAX_PASSES 96
int j2k_hip_stage_t1_passes(j2k_hip_encoder *enc, int reversible, void *d_coef, uint32_t stride,
                            uint32_t nblocks, const uint32_t *bx, const uint32_t *by, const uint32_t *bw,
                            const uint32_t *bh, const uint32_t *orient, const float *stepsize,
                            uint32_t *numbps, uint32_t *npasses, uint32_t *length, uint64_t *offsets,
                            void *data, size_t data_cap, uint32_t *pass_rate, int32_t *pass_dist);

/* Same as j2k_hip_stage_t1_passes under a code-block style (cblk_style as in j2k_hip_params; no pass_dist: a style excludes
 * rate control).  The blocks take the way of a styled frame: codeword capacities by the frame's formula, the bypass
 * instantiation of the modeller, the styled coder, and the fix-ups of pass_rate applied on the device.  pass_rate holds
 * the exact end of a codeword segment at every pass that terminates one and at the last pass, libopenjp2's estimate at
 * any other.  Vertically causal contexts (bit 8) and unknown bits: J2K_HIP_ERR_PARAM, as for a frame.  With
 * cblk_style = 0 the results are those of j2k_hip_stage_t1_passes.
 * J2K_HIP_ABI_VERSION is still 9: a function was added, none changed. */
int j2k_hip_stage_t1_styled(j2k_hip_encoder *enc, int reversible, void *d_coef, uint32_t stride,
                            uint32_t nblocks, const uint32_t *bx, const uint32_t *by, const uint32_t *bw,
                            const uint32_t *bh, const uint32_t *orient, const float *stepsize,
                            uint32_t *numbps, uint32_t *npasses, uint32_t *length, uint64_t *offsets,
                            void *data, size_t data_cap, uint32_t *pass_rate, uint32_t cblk_style);

/* j2k_hip_stage_t1_styled with the caller's slots: the same launches under the same tuning knobs (modeller, coder -- the
 * two-wave coder with cblk_style = 0, its pass-rate instantiation when pass_rate is given, the styled coder otherwise -- and
 * the rate fix-up under a style), but block i gets sym_cap[i] bytes for its decisions and out_cap[i] for its codeword in
 * place of what the frame's rule (j2k_hip_debug_cblk_capacities) would give, and a block that does not fit does not fail
 * the call.  For the tests that hold the kernels' capacity checks to their reports.
 * In: sym_cap[i], out_cap[i]: multiples of 16, at least 16, at most the rule's value for the block's area at Mb = 30 under
 * cblk_style; guard_bytes: a multiple of 16.  Anything else is J2K_HIP_ERR_PARAM before any launch.
 * Layout of both arenas: guard, slot 0, guard, slot 1, .., slot nblocks-1, guard -- slot i of an arena begins
 * guard_bytes + sum over j < i of (cap[j] + guard_bytes) bytes in.  Before the launches every byte of both arenas, guards and
 * slots alike, is set to J2K_HIP_SLOT_FILL.
 * Out (host): *err = the kernels' error word: 0, or 2 = a block's decisions did not fit sym_cap (the modeller reports that
 * block with no passes, no decisions, and the coder leaves its codeword slot alone), or 3 = a codeword did not fit out_cap
 * (its length[i] is the length it would have had; the bytes that fit are in the slot); with both kinds in one call either.
 * The call itself returns J2K_HIP_OK then.  numbps, npasses, nsym (decisions) and length per block; pass_rate (NULL, or
 * nblocks rows of J2K_HIP_MAX_PASSES, as j2k_hip_stage_t1_styled's -- a block whose codeword did not fit gets the coder's
 * counts without the fix-ups that look at bytes); sym_arena / out_arena receive the arenas whole (a buffer smaller than the
 * layout: J2K_HIP_ERR_OVERFLOW before any launch).
 * A block fits exactly: round_up(decisions, 16) bytes of sym_cap and round_up(length, 16) bytes of out_cap suffice, and the
 * kernels write no byte outside [0, round_up(decisions, 16)) and [0, round_up(length, 4)) of a slot that holds its block.
 * J2K_HIP_ABI_VERSION is still 9: a function was added, none changed. */
#define J2K_HIP_SLOT_FILL 0xA5
int j2k_hip_stage_t1_slots(j2k_hip_encoder *enc, int reversible, void *d_coef, uint32_t stride,
                           uint32_t nblocks, const uint32_t *bx, const uint32_t *by, const uint32_t *bw,
                           const uint32_t *bh, const uint32_t *orient, const float *stepsize, uint32_t cblk_style,
                           const uint32_t *sym_cap, const uint32_t *out_cap, uint32_t guard_bytes, uint32_t *err,
                           uint32_t *numbps, uint32_t *npasses, uint32_t *nsym, uint32_t *length, uint32_t *pass_rate,
                           void *sym_arena, size_t sym_arena_cap, void *out_arena, size_t out_arena_cap);

/* The rate control's kernels alone (rate_prepare_kernel, rate_ahead_kernel, rate_scan_kernel), on Tier-1 tables the caller
 * supplies, driven through the objects an encode drives them with.  All arrays are host memory.
 * In, per block i < nblocks (>= 1): weight[i] (the block's weight without the bit-plane), comp[i] (0..3), numbps[i] (<= 31),
 * npasses[i] (<= 3 numbps - 2 and <= J2K_HIP_MAX_PASSES; 0: an empty block), and the rows pass_rate[i][..], pass_dist[i][..]
 * of J2K_HIP_MAX_PASSES entries each, as j2k_hip_stage_t1_passes returns them.
 * Out, after the prepare kernel: disto[nblocks][J2K_HIP_MAX_PASSES] (cumulative weighted distortion), reach[nblocks][..]
 * and bounds[3][nblocks] (smallest / largest single-pass slope, steepest piece).  Entries of a row at and beyond npasses
 * are not written by the kernel: every byte of them comes back as 0xA5.
 * Then, for the blocks [first, first + count) as one tile's layer, done[count] = their passes in earlier layers (NULL: none):
 *   - K > 0: ahead[K], descending thresholds, give body[4][K], the per-component bound on the candidates' body bytes;
 *   - nscans scans, in order.  scans[i].mode = J2K_HIP_RATE_SCAN: the scan whose per-block results come back with it;
 *     J2K_HIP_RATE_SUMS_FETCH: the scan that brings back only its sums, into slot scans[i].slot (0..2), and a fetch of that
 *     slot straight behind it; J2K_HIP_RATE_SUMS_FETCH_LAST: the same with the fetch put off until every scan of the list
 *     has run (no later scan of the list may then use the slot; J2K_HIP_RATE_SCAN uses slot 0).  Scan i leaves
 *     taken[i][count], bytes[i][count] and sums[i][8] (per component c: [2c] body bytes in the layer, [2c + 1] header bits).
 * Refused with J2K_HIP_ERR_PARAM: what is outside the limits above, K > 128, thresholds ahead that ascend, a block range
 * outside the blocks or empty with a query, done[i] > npasses, an encode pending on the handle.  The handle's cached
 * geometry is dropped.  J2K_HIP_ABI_VERSION is still 9: a function was added, none changed. */
typedef struct j2k_hip_rate_taken { uint64_t lo; uint32_t hi; uint32_t n; } j2k_hip_rate_taken; /* bit p: the scan moved on at pass p; n: passes in layers 0..this one */
typedef struct j2k_hip_rate_scan { double thresh; uint32_t mode; uint32_t slot; } j2k_hip_rate_scan;
#define J2K_HIP_RATE_SCAN 0
#define J2K_HIP_RATE_SUMS_FETCH 1
#define J2K_HIP_RATE_SUMS_FETCH_LAST 2
int j2k_hip_stage_rate(j2k_hip_encoder *enc, uint32_t nblocks, const double *weight, const uint8_t *comp,
                       const uint32_t *numbps, const uint32_t *npasses, const uint32_t *pass_rate, const int32_t *pass_dist,
                       double *disto, float *reach, double *bounds, uint32_t first, uint32_t count, const uint8_t *done,
                       const double *ahead, uint32_t K, uint64_t *body, const j2k_hip_rate_scan *scans, uint32_t nscans,
                       j2k_hip_rate_taken *taken, uint32_t *bytes, uint64_t *sums);

/* rate_layers_kernel alone (j2k_hip_params.layer_slopes): ONE launch over Tier-1 tables the caller supplies, as an encode
 * queues it behind the coder.  In: the per-block arrays and rows of j2k_hip_stage_rate (all host memory; weight is looked up
 * at i % nweights, as the frames of a sequence share one frame's weights: 1 <= nweights <= nblocks), and slopes[layers],
 * 1 <= layers <= 100, finite.  Out, per block i and layer l at [i * layers + l]: passes[] = the block's passes in layers 0..l
 * (opj_tcd_makelayer at slopes[l] on top of the layers before), bytes[] = pass_rate[i][passes - 1], 0 without passes.
 * Both out arrays have (nblocks + J2K_HIP_RATE_LAYERS_SPARE) * layers entries: the device arrays are filled with 0xA5 first and
 * come back whole, so the spare entries show what the launch's idle lanes wrote (nothing).  rate_back / dist_back (optional,
 * nblocks rows of J2K_HIP_MAX_PASSES) receive the pass tables as they lie on the device after the launch: the kernel writes
 * neither, so a row's entries at and beyond npasses come back as the caller filled them.
 * Refused with J2K_HIP_ERR_PARAM: what j2k_hip_stage_rate refuses of the tables, layers out of range, a slope that is not
 * finite, an encode pending on the handle.  The handle's cached geometry is dropped. */
#define J2K_HIP_RATE_LAYERS_SPARE 64
int j2k_hip_stage_rate_layers(j2k_hip_encoder *enc, uint32_t nblocks, const double *weight, uint32_t nweights,
                              const uint32_t *numbps, const uint32_t *npasses, const uint32_t *pass_rate,
                              const int32_t *pass_dist, const double *slopes, uint32_t layers, uint8_t *passes,
                              uint32_t *bytes, uint32_t *rate_back, int32_t *dist_back);

/* rate_curve_kernel alone (j2k_hip_encode_sequence_budget_device): ONE launch over the tables of j2k_hip_stage_rate_layers, read
 * as nframes frames of nblocks / nframes blocks each.  Candidate j < K is the grid index min(base + j * step,
 * J2K_HIP_SLOPE_K_MAX); frame f is evaluated at max(candidate, cap[f]).  Out: sums[(f * K + j) * 2] = the body bytes of frame f's
 * blocks cut at T(that index), [.. + 1] = their header bits (rate_block_header_bits), followed by J2K_HIP_RATE_LAYERS_SPARE
 * entries that keep the 0xA5 fill; rate_back / dist_back as for j2k_hip_stage_rate_layers.
 * Refused with J2K_HIP_ERR_PARAM: what that hook refuses of the tables, K outside 1..64, step == 0, nframes == 0 or not a divisor
 * of nblocks, nweights other than 1..nblocks (block i takes weight[i % nweights]), base or a cap outside J2K_HIP_SLOPE_ALL..J2K_HIP_SLOPE_K_MAX, an encode
 * pending on the handle.  The handle's cached geometry is dropped. */
#define J2K_HIP_RATE_CURVE_MAX 64
int j2k_hip_stage_rate_curve(j2k_hip_encoder *enc, uint32_t nblocks, const double *weight, uint32_t nweights,
                             const uint32_t *numbps, const uint32_t *npasses, const uint32_t *pass_rate,
                             const int32_t *pass_dist, uint32_t nframes, const int32_t *cap, int32_t base, uint32_t step,
                             uint32_t K, uint64_t *sums, uint32_t *rate_back, int32_t *dist_back);

/* The codestream assembly alone: ONE launch of gather_kernel over three lists of pieces, its arguments filled as an encode
 * and a decode fill them.  dst (host, dst_bytes) goes up as it is, receives the pieces and comes back; `src` (host) is the
 * codeword arena, `blob` (host) the packet-header blob.  A piece copies len bytes from offset src of its source to offset dst:
 * blocks[] read `src` at 4-byte aligned offsets through a code-block table (a block of length 0 is skipped), headers[] read
 * `blob` at offsets below 2^32, segments[] read `src` at any 64-bit offset.
 * Refused with J2K_HIP_ERR_PARAM: a piece that reaches outside its source or the destination, a block source off the 4-byte
 * grid, destinations that overlap, an encode pending on the handle.  The handle's cached geometry is dropped.
 * J2K_HIP_ABI_VERSION is still 9: a function was added, none changed. */
typedef struct j2k_hip_gather_piece { uint64_t dst, src; uint32_t len, reserved; } j2k_hip_gather_piece;
int j2k_hip_stage_gather(j2k_hip_encoder *enc, const void *src, size_t src_bytes, const void *blob, size_t blob_bytes,
                         void *dst, size_t dst_bytes, const j2k_hip_gather_piece *blocks, uint32_t nblocks,
                         const j2k_hip_gather_piece *headers, uint32_t nheaders,
                         const j2k_hip_gather_piece *segments, uint32_t nsegments);
/* One launch of pack_offsets_kernel: dst[i] = base + len[0] + .. + len[i - 1] for i < n (host arrays).  n = 0: no launch,
 * dst is left alone.  J2K_HIP_ABI_VERSION is still 9: a function was added, none changed. */
int j2k_hip_stage_pack_offsets(j2k_hip_encoder *enc, const uint32_t *len, uint32_t n, uint64_t base, uint64_t *dst);

/* Inverse DWT (the mirror of j2k_hip_stage_dwt): `nplanes` planes of width*height 32-bit words (row stride =
 * width) in the Mallat layout of the oracle are synthesised from the lowest of `levels` resolutions upwards,
 * one kernel launch pair per level, the jobs built like a decode builds them.  With nregions == 0 a plane is
 * one region of origin (x0,y0).  Otherwise every plane holds `nregions` sub-rectangles (the tiles of a tiled
 * component), each a Mallat layout of its own with its own origin, all of them jobs of the same launches;
 * they must lie inside the plane and must not overlap; (x0,y0) is ignored.  d_in is preserved, d_out receives
 * the samples; words outside every region are copied from d_in. */
typedef struct j2k_hip_idwt_region {
    uint32_t x, y, w, h; /* the rectangle in the plane */
    uint32_t x0, y0;     /* its absolute origin (parities of the lifting) */
} j2k_hip_idwt_region;
int j2k_hip_stage_idwt(j2k_hip_encoder *enc, int reversible, uint32_t width, uint32_t height,
                       uint32_t nplanes, uint32_t levels, uint32_t x0, uint32_t y0,
                       const j2k_hip_idwt_region *regions, uint32_t nregions, const void *d_in,
                       void *d_out);
/* The windowed inverse DWT of a region decode alone (idwt_win_h_kernel + idwt_win_v_kernel), on the layout of
 * j2k_hip_stage_idwt with one region of origin (x0,y0) per plane: per resolution only the window the next one needs is
 * synthesised, from the coefficients j2k_hip_region_footprint names and no others.  Only the window (plane coordinates)
 * of d_out is specified; words outside it may hold anything; nothing outside the nplanes * height * width words is
 * written.  d_in is preserved. */
int j2k_hip_stage_idwt_window(j2k_hip_encoder *enc, int reversible, uint32_t width, uint32_t height,
                              uint32_t nplanes, uint32_t levels, uint32_t x0, uint32_t y0,
                              const j2k_hip_rect *window, const void *d_in, void *d_out);

/* The decode's output stage alone (decode_output_kernel: inverse RCT / ICT, DC level shift, clamp, replication of
 * sub-sampled components, CopyChannel's depth conversion), its arguments filled by the function a decode fills them with.
 * The image is width x height.  Component c is a plane of ceil(width / sub_x) x ceil(height / sub_y) 32-bit words (int32
 * for reversible, float32 otherwise) at row stride `stride` words, starting `offset` words into the device buffer d_comp of
 * comp_words words.  planes[i] receives component i as in j2k_hip_decode, except that planes[i].base is a byte OFFSET into
 * the device buffer d_buf of buf_bytes bytes; only the channels' samples are written.  Refused with J2K_HIP_ERR_PARAM:
 * what j2k_hip_decode refuses (sample_bits other than 8 / 16 / 32, depth outside 1..sample_bits -- float: 1..16 --, a float
 * channel off the 4-byte grid, precisions outside 1..16,
 * unlike precision or sub-sampling on components 0..2 with mct), a component plane or a channel that leaves its buffer,
 * and a 16-bit channel with a sample at an odd address. */
typedef struct j2k_hip_outcomp {
    uint64_t offset;     /* of the plane's first word in d_comp, in words */
    uint32_t prec;       /* the component's precision, 1..16 */
    uint32_t sub_x, sub_y;
} j2k_hip_outcomp;
int j2k_hip_stage_decode_output(j2k_hip_encoder *enc, int reversible, int mct, uint32_t width, uint32_t height,
                                const void *d_comp, size_t comp_words, uint32_t stride,
                                const j2k_hip_outcomp *comps, uint32_t ncomp, void *d_buf, size_t buf_bytes,
                                const j2k_hip_outplane *planes, uint32_t nplanes);

/* The RGBA output stage alone (decode_rgba_kernel), in the manner of j2k_hip_stage_decode_output: the components lie in
 * d_comp as there -- ceil((org_x + width) / sub_x) x ceil((org_y + height) / sub_y) words each, the destination's pixel
 * (0, 0) being image position (org_x, org_y) -- and the bases of dst's channels are byte OFFSETS into d_buf, so here the
 * alpha channel is absent when dst->a.sample_bits == 0.  mode: J2K_HIP_RGBA_*; ncomp: 3 or 4 (RGB: the fourth is A), 1 or 2
 * (GREY: the second is A), 1 (PALETTE), 3 or 4 (SYCC: three are read).  PALETTE: lut_size <= 256 entries of lut_columns <= 4
 * bytes each in `lut`; R, G, B take columns lut_rgb[0..2].  Refused with J2K_HIP_ERR_PARAM: what j2k_hip_decode_rgba and
 * j2k_hip_stage_decode_output refuse, a mode that cannot take ncomp components, a palette column beyond lut_columns. */
typedef struct j2k_hip_rgba_stage {
    uint32_t struct_size;
    uint32_t mode;
    uint32_t org_x, org_y;
    uint32_t lut_size, lut_columns;
    uint8_t lut[256][4];
    uint8_t lut_rgb[4];
} j2k_hip_rgba_stage;
int j2k_hip_stage_rgba_output(j2k_hip_encoder *enc, int reversible, int mct, uint32_t width, uint32_t height,
                              const void *d_comp, size_t comp_words, uint32_t stride,
                              const j2k_hip_outcomp *comps, uint32_t ncomp, void *d_buf, size_t buf_bytes,
                              const j2k_hip_rgba_dst *dst, const j2k_hip_rgba_stage *stage);
/* ... and with the X'Y'Z' -> R'G'B' conversion of j2k_hip_decode_set_xyz_to_rgb: xyz_to_rgb = 0..3 (0: the call above), the
 * kernel's arguments filled by the same function as for a decode.  Refused with J2K_HIP_ERR_PARAM, the text naming xyz_to_rgb: a
 * value above 3, a mode other than RGB, components 0..2 of unlike precision.  The handle's own setting is not read. */
int j2k_hip_stage_rgba_output_xyz(j2k_hip_encoder *enc, int reversible, int mct, uint32_t width, uint32_t height,
                                  const void *d_comp, size_t comp_words, uint32_t stride,
                                  const j2k_hip_outcomp *comps, uint32_t ncomp, void *d_buf, size_t buf_bytes,
                                  const j2k_hip_rgba_dst *dst, const j2k_hip_rgba_stage *stage, uint32_t xyz_to_rgb);

/* The compare's reduction alone (compare_kernel), with no file involved: the source planes (device pointers, as for
 * j2k_hip_compare_device) against decoded component planes that the caller supplies.  d_decoded (device) holds `channels` planes
 * of unsigned 16-bit samples, each dense at the component's own size ceil(width / sub_x) x ceil(height / sub_y), one after
 * another.  Parameters, refusals and results as for j2k_hip_compare. */
int j2k_hip_stage_compare(j2k_hip_encoder *enc, const j2k_hip_params *params, const j2k_hip_plane *planes_device,
                          const void *d_decoded, j2k_hip_diff *diffs, uint32_t ndiffs);

/* Tier-1 DECODING of `nblocks` code-blocks (default code-block style) into one coefficient plane of 32-bit
 * words (row stride `stride` words; int32 for reversible, float32 otherwise).  kernel = 0: a wavefront per
 * block; 1: a lane per block, the blocks in groups of 64 IN THE ORDER GIVEN.  Codewords are bytes
 * [cw_off, cw_off + cw_len) of the host buffer `cw`.  npasses is clamped to 3 * numbps - 2; a block with
 * npasses == 0 or numbps == 0 holds nothing and its rectangle is left as it was -- the rules of a file decode.
 * Rectangles (1..64 on either edge) must lie inside the stride and must not overlap. */
typedef struct j2k_hip_dec_block {
    uint32_t x, y, w, h;
    uint32_t orient, numbps, npasses, roishift;
    float half_step;     /* 0.5 x band step size (ignored when reversible) */
    uint32_t cw_len;
    uint64_t cw_off;
} j2k_hip_dec_block;
int j2k_hip_stage_t1_decode(j2k_hip_encoder *enc, int kernel, int reversible, void *d_coef,
                            uint32_t stride, uint32_t nblocks, const j2k_hip_dec_block *blocks,
                            const void *cw, size_t cw_bytes);
/* The same under a code-block style, through the lane-per-block kernel alone (the one that reads styled files).
 * cblk_style: the COD SPcod bits, 0..63 (1 bypass, 2 reset, 4 termall, 8 vertically causal, 16 pterm, 32 segsym).  Under
 * bypass or termall block i has the codeword segments segs[2 k], segs[2 k + 1] = (bytes, coding passes) for
 * k = seg_first[i] .. seg_first[i] + seg_count[i] - 1, in order; a pass beyond them opens a segment without bytes, and a
 * segment ends where the block's cw_len bytes end (what a file cut short leaves): both read as 1-bits.  Blocks, clamp,
 * empty blocks and the overlap check as above; cblk_style = 0 without segments gives j2k_hip_stage_t1_decode at kernel = 1.
 * Refused with J2K_HIP_ERR_PARAM: style bits above 63, a segment range outside segs[0 .. 2 nsegs_total), segments given under
 * a style without bypass and termall, a segment of more than 2^24 - 1 bytes or 255 passes, and under bypass or termall a
 * block that holds passes but no segment. */
int j2k_hip_stage_t1_decode_styled(j2k_hip_encoder *enc, int reversible, void *d_coef, uint32_t stride, uint32_t nblocks,
                                   const j2k_hip_dec_block *blocks, const void *cw, size_t cw_bytes, uint32_t cblk_style,
                                   const uint32_t *seg_first, const uint32_t *seg_count, const uint32_t *segs,
                                   uint32_t nsegs_total);

/* --- introspection ----------------------------------------------------------------------------- */
int j2k_hip_get_stats(const j2k_hip_encoder *enc, j2k_hip_stats *stats);
/* Device-time of the DWT kernels of the last encode call, per level (ms); returns levels. */
int j2k_hip_get_dwt_level_ms(const j2k_hip_encoder *enc, double *ms, int cap);

/* --- diagnostics --------------------------------------------------------------------------------
 * Process-wide tuning knob (names: j2k_amd/csrc/tuning.cpp; each also has a J2K_* environment variable that
 * is read once at first use).  Knobs move work between streams, CUs and launch shapes; no knob changes an
 * output byte.  Returns J2K_HIP_ERR_PARAM for an unknown key. */
int j2k_hip_debug_tune(const char *key, int value);
/* Host-only hooks for the tests (no handle, no device; the error text through j2k_hip_last_error(NULL)).
 * j2k_hip_debug_cblk_capacities: the slot a frame gives a code-block of `area` samples in a sub-band of Mb bit-planes under
 * cblk_style -- bytes of decisions and of codewords (the one rule, cblk_capacities).
 * j2k_hip_debug_blocks: the code-blocks of a frame of `params` in the order of the encoder's tables (Tier-2 packet order),
 * ten words each: tile, component, resolution, band inside the resolution, orientation, x, y (in the component's Mallat
 * plane), width, height, Mb.  *nblocks receives their number (rows == NULL: only that); J2K_HIP_ERR_OVERFLOW when cap is
 * less.
 * j2k_hip_debug_tier2: host Tier-2 alone on per-block results in that order (no code-block style): pricer == 0 plans the
 * codestream (*total_len = its length), pricer != 0 constructs the rate control's TilePricer of every tile.  Returns what
 * an encode whose Tier-1 reported these results returns.  Both honour params.guard_bits: the Mb column moves with the count,
 * and under J2K_HIP_GUARD_AUTO the hook plans (or prices) at the floor and, on an excess, once more at the count found --
 * the encoder's own plan, excess, re-plan path.  j2k_hip_debug_tier2_guard is j2k_hip_debug_tier2 that also reports the
 * count the plan was made with through *guard_bits. */
int j2k_hip_debug_tier2_guard(const j2k_hip_params *params, const uint32_t *numbps, const uint32_t *npasses, const uint32_t *length,
                              size_t nblocks, int pricer, uint64_t *total_len, uint32_t *guard_bits);
int j2k_hip_debug_cblk_capacities(uint32_t area, uint32_t Mb, uint32_t cblk_style, uint64_t *decisions, uint64_t *codeword);
int j2k_hip_debug_blocks(const j2k_hip_params *params, uint32_t *rows, size_t cap, size_t *nblocks);
int j2k_hip_debug_tier2(const j2k_hip_params *params, const uint32_t *numbps, const uint32_t *npasses, const uint32_t *length,
                        size_t nblocks, int pricer, uint64_t *total_len);
/* j2k_hip_debug_tier2_plan: the plan itself, not only its length -- what plan_codestream hands the gather kernel.  Inputs as
 * j2k_hip_debug_tier2, and
 *   pass_rate    per block and pass, the bytes at the end of the pass (nblocks rows of J2K_HIP_MAX_PASSES words): required
 *                when `params` carry a code-block style, refused otherwise;
 *   alloc_np / alloc_len / alloc_off   a layer allocation, entry [block * alloc_layers + layer] (passes, bytes and the bytes'
 *                offset inside the block's codeword); all three or none, alloc_layers = params->layers;
 *   nworkers     0: planned serially; n: with n worker threads (tiles of 4096 blocks and more are planned side by side).
 * params.guard_bits is honoured as by j2k_hip_debug_tier2_guard (plan, excess, re-plan).  Sizes are queried as with
 * j2k_hip_debug_blocks: a first call with the pointers of `out` NULL fills total_len, guard_bits and the four counts; a second
 * call with buffers of those capacities fills them (J2K_HIP_ERR_OVERFLOW where one is too small, J2K_HIP_ERR_PARAM where a
 * piece list is given in part).  A plan is laid into a
 * codestream by copying blob[src, src + len) to dst for every header piece and the blocks' bytes to cblk_dst[block] (no
 * allocation: ncblk_dst = nblocks, nbodies = 0) or bytes [off, off + len) of block `cblk` to dst for every body piece. */
typedef struct j2k_hip_tier2_plan {
    uint64_t total_len;
    uint32_t guard_bits;
    size_t blob_bytes, nheaders, ncblk_dst, nbodies;
    uint8_t *blob; size_t blob_cap;
    uint64_t *hdr_dst; uint32_t *hdr_src, *hdr_len; size_t hdr_cap;
    uint64_t *cblk_dst; size_t cblk_cap;
    uint64_t *body_dst; uint32_t *body_cblk, *body_off, *body_len; size_t body_cap;
} j2k_hip_tier2_plan;
int j2k_hip_debug_tier2_plan(const j2k_hip_params *params, const uint32_t *numbps, const uint32_t *npasses, const uint32_t *length,
                             size_t nblocks, const uint32_t *pass_rate, const uint32_t *alloc_np, const uint32_t *alloc_len,
                             const uint32_t *alloc_off, uint32_t alloc_layers, uint32_t nworkers, j2k_hip_tier2_plan *out);
/* The knob's current value through *value (tests restore what they change). */
int j2k_hip_debug_get_tune(const char *key, int *value);
/* Waves per SIMD the fused front end + level-1 DWT kernel reaches by its register count AS BUILT (read from the code object;
 * the kernel for `reversible` 5/3 or 9/7 and 1, 3 or 4 channels): the launch heuristics size their chunks by it, so a
 * compiler that changes the count changes them with it.  0 without a usable device. */
int j2k_hip_debug_fused_occupancy(j2k_hip_encoder *enc, int reversible, int channels);
/* Which Tier-1 decode kernel the handle's last decode call took (tools report it beside their timings): the code-blocks
 * decoded by the lane-per-block kernel and by the wave-per-block kernel (the whole call, or the tail beside the lanes). */
int j2k_hip_debug_decode_kernels(const j2k_hip_encoder *enc, uint64_t *lane_blocks, uint64_t *wave_blocks);
/* The work the handle's last decode call handed to Tier-1, summed over the frames of a sequence call: the coding passes of
 * the code-blocks decoded and their codeword bytes (what a layer limit, a region or a subsample leaves of the file). */
int j2k_hip_debug_decode_work(const j2k_hip_encoder *enc, uint64_t *passes, uint64_t *codeword_bytes);
/* Two sinks in native code for benchmarks and tools driven from a scripting language (bench.py's `host_path`): what they
 * time is then the library and a plain memcpy, not an interpreter's callback.  Both have j2k_hip_write_fn's signature.
 * j2k_hip_debug_copy_sink: `user` = a j2k_hip_copy_sink; appends the bytes at dst + pos (what OutputFile::Write into a
 * memory file costs: reference src/common/j2k_io.h:58-79); returns 0 -- which the encoder reports as a sink error -- when
 * the capacity would be exceeded.  j2k_hip_debug_count_sink: `user` = a size_t that receives the running byte count. */
typedef struct j2k_hip_copy_sink { void *dst; size_t capacity; size_t pos; } j2k_hip_copy_sink;
size_t j2k_hip_debug_copy_sink(void *user, const void *buf, size_t n);
size_t j2k_hip_debug_count_sink(void *user, const void *buf, size_t n);
/* Achieved copy bandwidth (GB/s, bytes read + bytes written per second) of a w x h float plane on the
 * encoder's device, averaged over `repeat` launches: the roofline's practical ceiling on this box.
 * mode 0: grid-stride 16-byte copy; 1: the DWT's access pattern without arithmetic (strips of 1 KiB rows,
 * four quadrant destinations, `rows` rows per wave); 2: 4 x 16 bytes in flight per lane; 3: the same with
 * non-temporal loads and stores; 4: one 16-byte element per thread (no loop). */
int j2k_hip_debug_membw(j2k_hip_encoder *enc, uint32_t w, uint32_t h, uint32_t rows, int mode, uint32_t repeat,
                        double *gbps);

/* The DWT launches of levels [first, first+count) (0 = level 1) of the handle's last encode call, replayed
 * `repeat` times back to back between two hipEvents; *ms = mean device time of one replay. */
int j2k_hip_debug_dwt_time(j2k_hip_encoder *enc, uint32_t first, uint32_t count, uint32_t repeat, double *ms);

/* --- device memory helpers for hosts without a HIP binding (tests, bench) ------------------------ */
int j2k_hip_malloc(j2k_hip_encoder *enc, void **dptr, size_t bytes);
int j2k_hip_free(j2k_hip_encoder *enc, void *dptr);
int j2k_hip_memcpy_h2d(j2k_hip_encoder *enc, void *dst, const void *src, size_t bytes);
int j2k_hip_memcpy_d2h(j2k_hip_encoder *enc, void *dst, const void *src, size_t bytes);
int j2k_hip_synchronize(j2k_hip_encoder *enc);

#ifdef __cplusplus
}
#endif
#endif /* J2K_HIP_H */
