// decode_seq.h -- host side of the sequence decode (j2k_hip_decode_sequence*, include/j2k_hip.h): which frames may share
// a call, and the merge of their plans (decode_plan.h) into the tables of one set of launches.  No HIP types here: the file
// is also built on its own under sanitizers (tests/native/decode_seq_sanitize.cpp).
#pragma once

#include "decode_plan.h"

namespace j2k_hip {

// The frames of one call must be decoded by the same launches with the same arguments: identical SIZ, COD (levels, blocks,
// style, wavelet, MCT, precincts, progression, layers), QCD / QCC values, RGN and POC; with `rgba` also what classify_rgba
// reads (colour space, opacity channel, palette).  COM, TLM, the tile-part structure, PPM / PPT, SOP / EPH and boxes that do
// not enter the decode may differ.  Returns what differs first, or an empty string.
std::string frames_differ(const FileHeader &a, const FileHeader &b, bool rgba);

// Where frame f of a merged plan lies: its file at byte file_off of the uploaded files (64-byte aligned), its codewords from
// arena_off on (a frame's arena keeps decode_plan.h's rules: blocks 16-byte aligned, 2 bytes of slack, 16 closing bytes), its
// coefficient planes from word coef_off on, and its ranges of the merged tables.
struct SeqFrame {
    uint64_t file_off = 0, file_len = 0, arena_off = 0, arena_len = 0, coef_off = 0;
    size_t blk_first = 0, blk_count = 0, seg_first = 0, seg_count = 0, cwseg_first = 0, cwseg_count = 0;
};
struct MergedPlan {
    std::vector<DecBlock> blocks;   // cw_off and seg_first are the merged tables'
    std::vector<uint32_t> frame_of; // per block: its frame
    std::vector<DecSeg> segs;       // src: byte of the uploaded files, dst: byte of the merged arena
    std::vector<uint32_t> cwsegs;
    uint64_t arena_bytes = 0, file_bytes = 0;
    std::vector<SeqFrame> frames;
};
// plans[f], f < n, of file_len[f] bytes, every frame's planes frame_words words apart.  The plans' blocks, segs and cwsegs are
// consumed (one frame: moved, not copied); their headers, geometry and windows stay.
MergedPlan merge_plans(DecodePlan *plans, size_t n, const size_t *file_len, uint64_t frame_words);

} // namespace j2k_hip
