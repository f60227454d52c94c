// decode_plan.h -- host side of the decode path: file / codestream parsing and Tier-2.
//
// Replaces what OpenJPEG does inside opj_read_header and the Tier-2 half of opj_decode for the reference's
// ReadFile / GetFileInfo (reference: src/common/j2k_openjpeg_codec.cpp:222-426, :451-586): JP2 boxes (T.800
// Annex I), main and tile-part headers (Annex A), packet headers with their tag trees (Annex B.10).  It never
// touches coefficient data: its product is, for every code-block, where its codeword bytes sit in the file and
// how many bit-planes / coding passes they hold -- the work list of the Tier-1 decode kernel.  O(#code-blocks).
#pragma once

#include <algorithm>

#include "geometry.h"

namespace j2k_hip {

struct FileHeader {
    Coding cod;                 // width, height, ncomp, prec, reversible, mct, layers, numres, cbw/cbh, prog, tiles
    uint32_t rsiz = 0;          // SIZ Rsiz, the codestream's capabilities (3 / 4: the 2K / 4K digital cinema profiles); nothing decodes by it
    bool sop = false, eph = false;
    std::vector<uint8_t> ppm;   // packed packet headers of the main header (PPM, A.7.4): the Ippm bytes of all segments in Zppm order
    uint8_t roishift[Coding::kMaxComps] = {}; // RGN (A.6.3): the component's region of interest by MAXSHIFT (H.1)
    std::vector<PocEntry> poc;  // progression order changes of the main header (empty: the COD progression throughout)
    uint32_t cblk_style = 0;    // COD SPcod code-block style: 1 bypass, 2 reset, 4 termall, 8 vcausal, 16 pterm, 32 segsym
    int guard = 2;
    int qstyle = 0;             // 0 none (reversible), 1 scalar derived, 2 scalar expounded
    std::vector<int> expn, mant; // per sub-band index (0 = LL, then HL,LH,HH per resolution)
    // file level (JP2 boxes)
    bool jp2 = false;
    uint32_t enumcs = 0;        // colr EnumCS (16 sRGB, 17 grey, 18 sYCC, 12 CMYK, 24 e-sYCC), 0 = none / ICC
    size_t icc_off = 0, icc_len = 0; // restricted ICC profile inside the file (colr method 2)
    uint32_t alpha_mask = 0;    // cdef: channels typed opacity (bit c)
    bool alpha_premultiplied = false;
    // palette (pclr + cmap boxes, I.5.3.4/5): the codestream's component 0 holds indices; the reference reports the palette to
    // its host as FileInfo.LUT / LUTmap and decodes the indices (src/common/j2k_openjpeg_codec.cpp:362-401, :503).  Only what
    // that code accepts: up to 256 entries of 8 bits in three columns, every channel mapped from component 0 through a column.
    uint32_t pal_entries = 0, pal_columns = 0;
    std::vector<uint8_t> palette;   // [entry][column]
    uint8_t pal_column_of[4] = {0, 1, 2, 3}; // cmap: output channel i takes palette column pal_column_of[i]
    size_t cs_off = 0, cs_len = 0; // the contiguous codestream inside the file
    size_t first_sot = 0;       // offset of the first SOT inside the codestream
    // per-component quantisation (QCC, A.6.5): what QCD gives every component, overridden for those that have their own
    struct Quant { bool present = false; int guard = 2, qstyle = 0; std::vector<int> expn, mant; };
    Quant qcc[Coding::kMaxComps];
    int band_numbps(uint32_t bandidx, uint32_t comp) const
    {
        const Quant &q = qcc[comp < Coding::kMaxComps ? comp : 0];
        return q.present ? q.expn[bandidx] + q.guard - 1 : expn[bandidx] + guard - 1;
    }
    // E.1.1 with Rb = precision for every band: libopenjp2's decoder folds the sub-band gains of the
    // irreversible path into its synthesis filter (high band x 2/K), see idwt.hip
    float band_stepsize(uint32_t bandidx, uint32_t comp) const; // (the precision is the component's)
};

// Header only: what GetFileInfo needs.  Throws Error(J2K_HIP_ERR_PARAM, ...) on anything unsupported.
FileHeader parse_headers(const uint8_t *file, size_t len);

struct DecSeg { uint64_t src; uint64_t dst; uint32_t len; }; // file offset -> codeword arena offset
struct DecBlock {
    uint32_t cblk;              // index into Geometry::cblks
    uint32_t numbps, npasses;
    uint64_t cw_off; uint32_t cw_len; // the block's codeword bytes in the arena (all layers, in order)
    // code-block styles with several codeword segments per block (bypass, termall): cwsegs[seg_first .. +nsegs) hold them in
    // order, each `len | passes << 24`; nsegs = 0: one segment with every pass
    uint32_t seg_first = 0, nsegs = 0;
    uint32_t roishift = 0;      // numbps counts the region-of-interest shift's planes too (H.1); samples at or above 2^roishift come down by it
};
// What the Tier-1 decode kernels are given, stated once for the plan, the decode call and the stage hook:
//  * the coding passes of a block: never more than the 3 numbps - 2 its bit-planes allow; 0 = the block holds nothing
//    (no pass or no bit-plane) and is NOT handed to the kernels, whose tables (masks, planes) and plane arithmetic
//    (t1_assemble: npasses - 1) start at one pass of one bit-plane -- its samples stay as the plane was cleared;
//  * the codeword arena: a block's bytes start 16-byte aligned, 2 bytes of slack follow them, 16 more close the
//    arena, and the buffer extends kCwArenaTail bytes past that (the wave-per-block kernel loads whole 256-byte windows).
inline uint32_t t1dec_passes(uint32_t numbps, uint32_t npasses) { return numbps ? std::min<uint32_t>(npasses, 3 * numbps - 2) : 0; }
inline uint64_t cw_arena_next(uint64_t end) { return (end + 2 + 15) & ~(uint64_t)15; } // where the next block starts after one that ends at `end`
inline uint64_t cw_arena_bytes(uint64_t next) { return next + 16; }
constexpr size_t kCwArenaTail = 512;
// A codeword segment of a block as the lane decoder reads it (DecodePlan::cwsegs, t1_dec_lane.h Block::segs), stated once for
// the plan and the styled stage hook: the bytes of it that are there -- a segment of `len` bytes that begins `at` bytes into a
// block of which `bytes` bytes arrived (a file cut short may have lost bytes the headers had promised) -- and the word.
constexpr uint32_t kCwSegMaxBytes = (1u << 24) - 1u, kCwSegMaxPasses = 255;
inline uint32_t cwseg_have(uint64_t len, uint64_t at, uint64_t bytes) { return (uint32_t)(at < bytes ? std::min<uint64_t>(len, bytes - at) : 0); }
inline uint32_t cwseg_word(uint32_t have, uint32_t passes) { return have | (passes << 24); }

// ---- region decode: which coefficients a window of the top decoded resolution needs (no device, no file)
// Rectangles are half open and in ABSOLUTE coordinates of their resolution or band (T.800 B.5: low-band sample n of a
// resolution is its interleaved position 2n, high-band sample n position 2n + 1).
struct IRect {
    int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
    bool empty() const { return x1 <= x0 || y1 <= y0; }
    bool meets(int ax0, int ay0, int ax1, int ay1) const { return !empty() && ax0 < x1 && x0 < ax1 && ay0 < y1 && y0 < ay1; }
};
struct ResFootprint {
    IRect win;      // the window of this resolution that is synthesised (resolution 0: the LL coefficients that are read)
    IRect band[3];  // resolution >= 1: the coefficients of HL, LH, HH that its synthesis reads
    // the band rows the vertical pass reads, so the rows the horizontal pass has to produce: low rows [ly0, ly1), high [hy0, hy1)
    int ly0 = 0, ly1 = 0, hy0 = 0, hy1 = 0;
};
// res[r] = the rectangle of resolution r of one tile-component (r = 0 .. nres - 1), `window` a non-empty rectangle inside
// res[nres - 1].  The support is idwt.hip's synth_pair: outputs come in (even, odd) pairs of absolute positions, a pair at
// (p, p + 1) reads interleaved positions p - 1 .. p + 3 (5/3) or p - 3 .. p + 5 (9/7), reflected into the line -- within
// those bounds every reflected position lies between the clamped ends, so clamping is exact.  Returns nres entries; below
// a resolution whose low-band need is empty (a line of one odd sample) everything stays empty.
std::vector<ResFootprint> region_footprints(const IRect *res, uint32_t nres, bool reversible, const IRect &window);

struct DecodePlan {
    FileHeader hdr;
    Geometry geo;               // all tiles
    uint32_t reduce = 0;
    std::vector<DecBlock> blocks; // blocks of the resolutions that are decoded and that hold at least one pass
    std::vector<DecSeg> segs;
    std::vector<uint32_t> cwsegs;
    uint64_t arena_bytes = 0;
    // a window decode: per tile (in geo.tiles order) and decoded component [tile * 4 + comp], the footprints of resolutions
    // 0 .. numres - 1 - reduce; empty where the window misses the tile-component.  Blocks outside them are not in `blocks`.
    bool windowed = false;
    std::vector<std::vector<ResFootprint>> windows;
    // a file cut short: tile_arrived[t] (geo.tiles order) = the file holds a tile-part of the tile (its SOT .. SOD at least);
    // tiles_missing = how many do not.  The samples of such a tile are component value 0 (libopenjp2 leaves its image buffer as
    // it allocated it), not what a tile of zero coefficients decodes to; a tile that arrived with packets missing is the latter.
    std::vector<uint8_t> tile_arrived;
    uint32_t tiles_missing = 0;
};

// Tier-2 of the whole file for a decode at resolution `reduce` (0 = full size).  window (optional): x, y, w, h in pixels of
// the image as it is delivered at this resolution (top-left at (0, 0)); outside that image: Error(J2K_HIP_ERR_PARAM).
// max_layers (0 = all): keep the first max_layers quality layers only.  The plan is, block for block, the plan of the file
// with every packet of a later layer removed and COD's layer count set to max_layers (what libopenjp2 decodes for
// opj_dparameters_t::cp_layer): all packet headers are parsed, a block keeps the passes and bytes of the kept layers, a block
// first included later holds nothing, and under bypass / termall the segment table lists the kept passes and bytes only
// (its last segment may hold fewer passes than it has room for).  max_layers >= the file's layers: the plan of 0.
DecodePlan plan_decode(const uint8_t *file, size_t len, uint32_t reduce, const uint32_t *window = nullptr, uint32_t max_layers = 0);
// the size of the delivered image at resolution `reduce` (opj_image_comp_header_update: both edges scaled, then subtracted)
void reduced_size(const Coding &cod, uint32_t reduce, int &ow, int &oh);

} // namespace j2k_hip
