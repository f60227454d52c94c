/*
 * j2k_oracle.h -- TEST INFRASTRUCTURE ONLY.
 *
 * CPU restatement (plain C) of the JPEG 2000 encode path that the reference plug-in drives through
 * OpenJPEG (reference call sites: src/common/j2k_openjpeg_codec.cpp:589-758; sample staging:
 * src/common/j2k_codec.cpp:222-427; input layout: src/aftereffects/j2k.cpp:324-362; promote:
 * src/aftereffects/FrameSeq.cpp:311-314).  The arithmetic follows ITU-T T.800 Annexes A-G,
 * reconciled byte-for-byte against libopenjp2 2.4.0 / 2.5.4 (see oracle/opj_replay.c and
 * tests/golden/).  Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may use it.
 */
#ifndef J2K_ORACLE_H
#define J2K_ORACLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct j2ko_params {
    int32_t width, height, ncomp, prec; /* prec = FileInfo.depth (1..16), unsigned samples */
    int32_t reversible;                 /* 1: 5/3 + RCT, 0: 9/7 + ICT                     */
    int32_t mct;                        /* 1: colour transform on comps 0..2              */
    int32_t numres;                     /* decomposition levels + 1 (OpenJPEG default 6)  */
    int32_t cblkw_exp, cblkh_exp;       /* log2 code-block size (default 6,6)             */
    int32_t layers;                     /* tcp_numlayers (reference default 12)           */
    int32_t tile_w, tile_h;             /* 0 = untiled                                    */
    int32_t prog;                       /* 0 LRCP, 1 RLCP, 2 RPCL, 3 PCRL, 4 CPRL         */
    int32_t mode;                       /* code-block style, COD SPcod bits (J2KO_STYLE_*); not with a rate target */
    int32_t nprec;                      /* precinct sizes given (0: maximal precincts); LRCP, RLCP and RPCL only   */
    int32_t prcw[8], prch[8];           /* in samples, highest resolution first; the last one halves for every      */
                                        /* resolution below it (libopenjp2: opj_compress -c)                        */
} j2ko_params;

/* Code-block styles (T.800 Table A.19).  Vertically causal contexts (8) are not coded. */
enum { J2KO_STYLE_BYPASS = 1, J2KO_STYLE_RESET = 2, J2KO_STYLE_TERMALL = 4, J2KO_STYLE_PTERM = 16, J2KO_STYLE_SEGSYM = 32,
       J2KO_STYLES_CODED = 1 | 2 | 4 | 16 | 32 };

/* What the coder of one block met on its way (for tests that steer blocks at these cases). */
typedef struct j2ko_t1_events {
    int32_t raw_ff_inside;      /* 0xFF bytes of raw segments with at least one bit behind them (seven bits follow)      */
    int32_t raw_ff_dropped;     /* raw segments that ended on a 0xFF, which was taken back                                */
    int32_t raw_ff7f_dropped;   /* raw segments that ended on 0xFF 0x7F, both taken back (no predictable termination)     */
    int32_t raw_ff7f_kept;      /* raw segments that ended on 0xFF 0x7F under predictable termination: both stay          */
    int32_t raw_empty;          /* raw segments of no bytes: without a bit, or with all their bytes taken back             */
    int32_t mq_after_empty_raw; /* MQ segments opened right behind such a segment                                          */
    int32_t restart_ct13;       /* MQ segments opened on a last byte 0xFF (CT = 13)                                        */
    int32_t segsym_alone;       /* cleanup passes whose only decisions were the four segmentation symbols                 */
} j2ko_t1_events;

/* A1: AE "15+1 bit" -> 16 bit (FrameSeq.cpp:311-314) and its inverse (FrameSeq.cpp:265-268). */
uint16_t j2ko_promote(uint16_t v);
uint16_t j2ko_demote(uint16_t v);

/* A2: Codec::CopyBuffer for one channel, destination = planar int32 (j2k_codec.cpp:222-378).
 * src_bytes = 1 (UCHAR) or 2 (USHORT); src_depth = Channel.depth (8/16); dst_depth = FileInfo.depth. */
void j2ko_copy_channel(int32_t *dst, int width, int height, const uint8_t *src, ptrdiff_t colbytes,
                       ptrdiff_t rowbytes, int src_bytes, int src_depth, int dst_depth);

/* A4+A5: DC level shift and colour transform, in place, n samples per plane.
 * reversible: planes stay int32; irreversible: planes are rewritten as float32 bit patterns. */
void j2ko_dc_mct(int32_t **planes, int ncomp, size_t n, int prec, int reversible, int mct);

/* A6: forward DWT of one tile-component, in place, Mallat layout, row stride `stride`.
 * (x0,y0) = absolute origin of the tile-component (lifting phase). */
void j2ko_dwt53(int32_t *a, int w, int h, int stride, int x0, int y0, int levels);
void j2ko_dwt97(float *a, int w, int h, int stride, int x0, int y0, int levels);

/* Quantisation tables (A7). band index b = 0 (LL), then (HL,LH,HH) per resolution 1..numres-1. */
void j2ko_band_quant(int prec, int reversible, int numres, int bandidx, int *expn, int *mant,
                     int *numbps, float *stepsize);

/* A7: T1 input scaling of one coefficient (6 fractional bits, sign-magnitude result in *out as
 * two's complement int32): 5/3: c << 6; 9/7: lrintf((c / stepsize) * 64). */
int32_t j2ko_quant53(int32_t c);
int32_t j2ko_quant97(float c, float stepsize);

/* A8: EBCOT Tier-1 of one code-block.
 * data: w*h int32 in raster order (row stride w), already scaled by j2ko_quant*.
 * orient: 0 LL, 1 HL, 2 LH, 3 HH.
 * out/out_cap: codeword bytes. pass_rate[], pass_nmsedec[] (cap 3*32): cumulative byte count (after
 * OpenJPEG's rate fix-ups) and per-pass integer distortion LUT sum.
 * sym/sym_cap (optional): the (ctx<<1|bit) MQ symbol stream in coding order; *nsym its length;
 * pass_nsym[] (optional) cumulative symbol count at the end of every pass.
 * Returns total passes; *numbps receives the code-block's magnitude bit-planes. */
int j2ko_t1_encode_block(const int32_t *data, int w, int h, int orient, uint8_t *out, size_t out_cap,
                         int *numbps, int *pass_rate, int *pass_nmsedec, uint8_t *sym, size_t sym_cap,
                         size_t *nsym, int *pass_nsym);

/* The same under a code-block style (J2KO_STYLE_* bits; 0 = none: then exactly j2ko_t1_encode_block).  pass_term[]
 * (optional): 1 where the pass ends a codeword segment -- pass_rate[] there is the exact end of the segment, elsewhere
 * libopenjp2's estimate.  In raw passes the traced decision of a sign is the sign itself.  The four segmentation symbols
 * are not in the trace.  events (optional) receives the counts above.  Returns -2 for a style that is not coded. */
int j2ko_t1_encode_block_styled(const int32_t *data, int w, int h, int orient, int style, uint8_t *out, size_t out_cap,
                                int *numbps, int *pass_rate, int *pass_nmsedec, int *pass_term, uint8_t *sym,
                                size_t sym_cap, size_t *nsym, int *pass_nsym, j2ko_t1_events *events);

/* number of passes layer 0 receives when there is no rate target (all of them). */
int j2ko_included_passes(int npasses, const int *pass_rate, const int *pass_nmsedec);

/* Whole path A3..A9: planes = ncomp consecutive width*height int32 planes of unsigned samples
 * (the representation after CopyBuffer).  comment = COM marker text (NULL -> none).
 * Returns codestream length or <0. */
long j2ko_encode(const j2ko_params *p, const int32_t *planes, uint8_t *out, size_t cap,
                 const char *comment);

/* Same, but also exports the per-tile-component coefficient planes after the DWT (for stage-level
 * parity of GPU kernels). coef_out (optional) = ncomp * width * height int32/float32 bit patterns,
 * valid for untiled images only. */
long j2ko_encode_ex(const j2ko_params *p, const int32_t *planes, uint8_t *out, size_t cap,
                    const char *comment, int32_t *coef_out);

/* Rate-controlled encode: rates[p->layers] = one compression ratio per quality layer
 * (OpenJPEG tcp_rates with cp_disto_alloc; 0 = everything that is left, i.e. lossless for 5/3). */
long j2ko_encode_rates(const j2ko_params *p, const int32_t *planes, uint8_t *out, size_t cap,
                       const char *comment, const float *rates);

/* Same when a file wrapper of prefix_len bytes (JP2 boxes up to and including the jp2c box header) sits
 * in front of the codestream: OpenJPEG charges those bytes to the budget too. */
long j2ko_encode_rates_ex(const j2ko_params *p, const int32_t *planes, uint8_t *out, size_t cap,
                          const char *comment, const float *rates, size_t prefix_len);

/* Fixed-quality encode: psnr[p->layers] = one PSNR target in dB per layer (OpenJPEG cp_fixed_quality with
 * tcp_distoratio; 0 = everything that is left). */
long j2ko_encode_psnr(const j2ko_params *p, const int32_t *planes, uint8_t *out, size_t cap,
                      const char *comment, const float *psnr);

/* JP2 file wrapper: the bytes OpenJPEG's JP2 writer (third-party, absent from
 * /root/reference: ext/openjpeg src/lib/openjp2/jp2.c -- opj_jp2_setup_encoder, opj_jp2_write_jp,
 * _ftyp, _jp2h {ihdr, colr, cdef}, _jp2c) puts in front of the codestream for the image the
 * reference describes to it (reference: j2k_openjpeg_codec.cpp:613 JP2 branch, :650-661 colour
 * space, T.800 Annex I for the box layouts).  color_space is the OPJ_COLOR_SPACE value; icc (may be
 * NULL) selects colr method 2; alpha_channel < 0 = none.  Returns the length; writes at most cap. */
size_t j2ko_jp2_header(uint32_t width, uint32_t height, uint32_t ncomp, uint32_t prec, int color_space,
                       const uint8_t *icc, uint32_t icc_len, int alpha_channel, uint32_t codestream_len,
                       uint8_t *out, size_t cap);

/* ---- decode path (j2k_oracle_dec.c; SURVEY.md 8f N4: reference src/common/j2k_openjpeg_codec.cpp:451-586) ----
 * Whole decode of a raw codestream or JP2 file at resolution `reduce` (= log2 of the reference's `subsample`,
 * :501): out = ncomp planes of dims[0] x dims[1] int32 samples (what opj_decode leaves in image->comps[].data,
 * :512), dims = {w, h, ncomp, prec}.  Returns 0, or -1 with j2ko_decode_error(). */
int j2ko_decode(const uint8_t *file, size_t len, int reduce, int32_t *out, size_t cap_samples, int dims[4]);
const char *j2ko_decode_error(void);
/* The code-blocks of a file as the Tier-2 of j2ko_decode finds them (every block that holds passes): meta = 16 words per
 * block -- tile, component, resolution, orientation, x, y (in the tile-component's Mallat plane), w, h, numbps, npasses, first
 * segment, segments, byte offset, bytes, 0.5 x step size (float bits; 1.0 reversible), 0; segs = (bytes, passes) pairs (bypass /
 * termall only); hdr = {code-block style, reversible, components, tiles}.  Returns the number of blocks or -1. */
long j2ko_file_blocks(const uint8_t *file, size_t len, int32_t *meta, size_t cap_blocks, uint32_t *segs, size_t cap_segs, uint8_t *bytes,
                      size_t cap_bytes, int hdr[4]);
/* The same, and what each packet header announced: pieces = 4 words per length field read -- block (index into meta), layer,
 * bytes, passes -- block after block, inside a block in the order read; one piece per layer a block contributes to, under
 * bypass / termall one per codeword segment the layer's passes fall into.  *npieces receives their number. */
long j2ko_file_block_pieces(const uint8_t *file, size_t len, int32_t *meta, size_t cap_blocks, uint32_t *segs, size_t cap_segs, uint8_t *bytes,
                            size_t cap_bytes, int hdr[4], uint32_t *pieces, size_t cap_pieces, size_t *npieces);
/* Of the file read last (j2ko_decode, j2ko_file_blocks, j2ko_file_block_pieces): out[0] = the packet headers read, out[1] =
 * those whose last bit was the last bit of a byte 0xFF, by the reader's own bit position (B.10.1: one more byte follows). */
void j2ko_packet_stats(long out[2]);
/* Header only (GetFileInfo, :222-426): info = {width, height, ncomp, prec, reversible, mct, numres, is_jp2, enumcs,
 * icc offset in the file, icc length, alpha channel mask}. */
int j2ko_decode_info(const uint8_t *file, size_t len, int info[12]);
/* Tier-1 decoding of one code-block: `npasses` coding passes of a block with `numbps` magnitude bit-planes from
 * its codeword segment.  out = w*h values in the decoder's representation (sign, magnitude with one fractional
 * bit: the middle of the interval known so far).  Returns the passes decoded. */
int j2ko_t1_decode_block(const uint8_t *data, size_t len, int w, int h, int orient, int numbps, int npasses, int32_t *out);
/* The same under a code-block style (COD SPcod bits: 1 bypass, 2 reset, 4 termall, 8 vertically causal, 16 pterm,
 * 32 segsym).  segs = nsegs pairs (bytes, coding passes) of the block's codeword segments, looked at under bypass or
 * termall only; a pass beyond the listed segments, and bytes beyond a segment's end or beyond `len`, read 0xFF.
 * Segmentation symbols are consumed, not checked.  style = 0, nsegs = 0: j2ko_t1_decode_block.
 * _ex: *below_significant = how often a sample of a stripe's last row was coded next to a significant sample of the row
 * below it (what vertically causal contexts hide: 0 means the style changed nothing for this block). */
int j2ko_t1_decode_block_styled(const uint8_t *data, size_t len, int w, int h, int orient, int numbps, int npasses, int style,
                                const uint32_t *segs, int nsegs, int32_t *out);
int j2ko_t1_decode_block_styled_ex(const uint8_t *data, size_t len, int w, int h, int orient, int numbps, int npasses, int style,
                                   const uint32_t *segs, int nsegs, int32_t *out, long *below_significant);
/* Inverse DWT of a Mallat-layout plane (inverse of j2ko_dwt53 / j2ko_dwt97 up to the irreversible path's own scaling:
 * the 9/7 synthesis scales the low band by K and the high band by 2/K like libopenjp2's decoder). */
void j2ko_idwt53(int32_t *a, int w, int h, int stride, int x0, int y0, int levels);
void j2ko_idwt97(float *a, int w, int h, int stride, int x0, int y0, int levels);
/* The tail of a tile's decode, in place (what j2ko_decode runs on every tile): inverse RCT / ICT on components 0..2 when
 * `mct`, DC level shift, saturating float conversion (irreversible; NaN gives the lowest value) and clamp to
 * [0, 2^prec[c] - 1].  planes[c] = n[c] words, int32 or float32 bit patterns in, int32 samples out. */
void j2ko_decode_output(int32_t *const planes[], int ncomp, const size_t n[], const int prec[], int reversible, int mct);
/* Codec::CopyBuffer towards the host's buffer (src/common/j2k_codec.cpp:222-427, DESTTYPE = unsigned char / short). */
void j2ko_copy_channel_out(uint8_t *dst, int dst_bytes, int dst_depth, ptrdiff_t colbytes, ptrdiff_t rowbytes, int width,
                           int height, const int32_t *src, int src_stride, int src_depth);

#ifdef __cplusplus
}
#endif
#endif
