// Host side of the sequence decode (decode_seq.cpp: the merge of the frames' plans into the tables of one set of launches)
// under AddressSanitizer + UndefinedBehaviorSanitizer.  Every file given is taken three times -- whole, cut at 70 % and cut
// at 35 % of its length -- as the frames of one call, at full size and at half size.  What the device code takes on trust
// from the merged plan is checked here.  Built and run by tests/test_decode_sequence_host.py; no HIP, no device.
#include "../../j2k_amd/csrc/decode_seq.h"

#include <algorithm>
#include <cstdio>
#include <fstream>
#include <iterator>

using namespace j2k_hip;

static bool same_block(const DecBlock &a, const DecBlock &b)
{
    return a.cblk == b.cblk && a.numbps == b.numbps && a.npasses == b.npasses && a.cw_off == b.cw_off && a.cw_len == b.cw_len &&
           a.seg_first == b.seg_first && a.nsegs == b.nsegs && a.roishift == b.roishift;
}

// nullptr, or what is wrong with the merge M of `plans` (copies of what was merged)
static const char *merge_fault(const MergedPlan &M, const std::vector<DecodePlan> &plans, const std::vector<size_t> &lens, uint64_t frame_words)
{
    const size_t n = plans.size();
    if (M.frames.size() != n || M.frame_of.size() != M.blocks.size()) return "frame tables of the wrong size";
    uint64_t file_end = 0, arena_end = 0, coef_end = 0;
    size_t blk_end = 0, seg_end = 0, cwseg_end = 0;
    for (size_t f = 0; f < n; ++f) {
        const SeqFrame &F = M.frames[f];
        const DecodePlan &P = plans[f];
        // the ranges of different frames are disjoint (they are in frame order, each behind the one before)
        if (F.file_off < file_end || F.file_off % 64 || F.file_len != lens[f]) return "a frame's file overlaps the one before or is misaligned";
        if (F.arena_off < arena_end || F.arena_off % 16 || F.arena_len != P.arena_bytes) return "a frame's arena overlaps the one before or is misaligned";
        if (F.coef_off < coef_end) return "a frame's coefficient planes overlap the one before";
        if (F.blk_first != blk_end || F.seg_first != seg_end || F.cwseg_first != cwseg_end) return "a frame's table ranges do not follow the one before";
        if (F.blk_count != P.blocks.size() || F.seg_count != P.segs.size() || F.cwseg_count != P.cwsegs.size()) return "a frame's table ranges have the wrong length";
        file_end = F.file_off + F.file_len; arena_end = F.arena_off + F.arena_len; coef_end = F.coef_off + frame_words;
        blk_end += F.blk_count; seg_end += F.seg_count; cwseg_end += F.cwseg_count;
        if (file_end > M.file_bytes || arena_end > M.arena_bytes) return "a frame reaches past the merged file bytes or arena";
        if (blk_end > M.blocks.size() || seg_end > M.segs.size() || cwseg_end > M.cwsegs.size()) return "a frame's table range leaves the merged table";
        // every codeword piece: from the frame's own bytes into the frame's own arena
        for (size_t i = 0; i < F.seg_count; ++i) {
            const DecSeg &s = M.segs[F.seg_first + i], &o = P.segs[i];
            if (s.src < F.file_off || s.src + s.len > F.file_off + F.file_len) return "a codeword piece outside its frame's bytes";
            if (s.dst < F.arena_off || s.dst + s.len > F.arena_off + F.arena_len) return "a codeword piece outside its frame's arena";
            if (s.src - F.file_off != o.src || s.dst - F.arena_off != o.dst || s.len != o.len) return "a codeword piece is not the plan's";
        }
        // every block: its frame, its bytes inside the frame's arena, decode_plan.h's padding, its segments inside the frame's range
        std::vector<std::pair<uint64_t, uint64_t>> spans;
        for (size_t i = 0; i < F.blk_count; ++i) {
            const DecBlock &b = M.blocks[F.blk_first + i], &o = P.blocks[i];
            if (M.frame_of[F.blk_first + i] != f) return "a block of the wrong frame";
            if (b.cw_off % 16) return "a block's codewords are not 16-byte aligned";
            if (b.cw_off < F.arena_off || b.cw_off + b.cw_len > F.arena_off + F.arena_len) return "a block's codewords outside its frame's arena";
            if (cw_arena_bytes(cw_arena_next(b.cw_off + b.cw_len)) > F.arena_off + F.arena_len) return "no slack and closing bytes behind a block's codewords";
            if (b.nsegs && (b.seg_first < F.cwseg_first || (uint64_t)b.seg_first + b.nsegs > F.cwseg_first + F.cwseg_count)) return "a block's codeword segments outside its frame's range";
            DecBlock back = b;
            back.cw_off -= F.arena_off;
            if (back.nsegs) back.seg_first -= (uint32_t)F.cwseg_first;
            if (!same_block(back, o)) return "a block is not the plan's";
            spans.emplace_back(b.cw_off, b.cw_off + b.cw_len);
        }
        std::sort(spans.begin(), spans.end());
        for (size_t i = 1; i < spans.size(); ++i)
            if (spans[i].first < cw_arena_next(spans[i - 1].second)) return "two blocks' codewords closer than the arena's padding";
        for (size_t i = 0; i < F.cwseg_count; ++i)
            if (M.cwsegs[F.cwseg_first + i] != P.cwsegs[i]) return "a codeword segment word is not the plan's";
    }
    if (blk_end != M.blocks.size() || seg_end != M.segs.size() || cwseg_end != M.cwsegs.size()) return "entries of the merged tables that belong to no frame";
    if (M.arena_bytes < arena_end || M.file_bytes < file_end) return "the merged totals are short";
    return nullptr;
}

int main(int argc, char **argv)
{
    int merged = 0, frames = 0, skipped = 0;
    for (int a = 1; a < argc; ++a) {
        std::ifstream f(argv[a], std::ios::binary);
        const std::vector<uint8_t> data((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        if (data.empty()) { std::fprintf(stderr, "cannot read %s\n", argv[a]); return 1; }
        FileHeader H;
        try { H = parse_headers(data.data(), data.size()); }
        catch (const Error &x) {
            if (x.code != J2K_HIP_ERR_UNSUPPORTED) { std::fprintf(stderr, "%s does not parse: %s\n", argv[a], x.what()); return 1; }
            ++skipped;
            continue;
        }
        bool any = false;
        for (uint32_t reduce = 0; reduce < 2 && reduce < H.cod.numres; ++reduce) {
            // the frames: exact-size heap blocks, so that a read past a cut file's end trips ASan
            std::vector<std::vector<uint8_t>> files;
            std::vector<DecodePlan> plans;
            std::vector<size_t> lens;
            for (size_t cut : {data.size(), data.size() * 7 / 10, data.size() * 35 / 100}) {
                std::vector<uint8_t> copy(data.begin(), data.begin() + (ptrdiff_t)cut);
                try {
                    plans.push_back(plan_decode(copy.data(), copy.size(), reduce));
                } catch (const Error &) {
                    continue; // (a cut this reader turns away: not a frame of the call)
                }
                if (!frames_differ(plans[0].hdr, plans.back().hdr, true).empty()) { std::fprintf(stderr, "a cut copy of %s differs from the file\n", argv[a]); return 1; }
                files.push_back(std::move(copy));
                lens.push_back(cut);
            }
            if (plans.empty()) { std::fprintf(stderr, "%s does not plan\n", argv[a]); return 1; }
            const uint64_t frame_words = (uint64_t)H.cod.width * H.cod.height * H.cod.ncomp_out() + 64;
            // a merge of one frame is that frame's plan
            {
                std::vector<DecodePlan> one(1, plans[0]), keep(1, plans[0]);
                const MergedPlan M = merge_plans(one.data(), 1, lens.data(), frame_words);
                if (const char *why = merge_fault(M, keep, std::vector<size_t>(1, lens[0]), frame_words)) { std::fprintf(stderr, "one frame of %s: %s\n", argv[a], why); return 1; }
                if (M.arena_bytes != keep[0].arena_bytes || M.frames[0].file_off || M.frames[0].arena_off || M.frames[0].coef_off || M.frames[0].cwseg_first)
                    { std::fprintf(stderr, "one frame of %s: bases that are not zero\n", argv[a]); return 1; }
                for (size_t i = 0; i < M.blocks.size(); ++i)
                    if (!same_block(M.blocks[i], keep[0].blocks[i])) { std::fprintf(stderr, "one frame of %s: a block moved\n", argv[a]); return 1; }
            }
            // the frames of one call, and the same frames in reverse order
            for (int rev = 0; rev < 2; ++rev) {
                std::vector<DecodePlan> work = plans, keep = plans;
                std::vector<size_t> l = lens;
                if (rev) { std::reverse(work.begin(), work.end()); std::reverse(keep.begin(), keep.end()); std::reverse(l.begin(), l.end()); }
                const MergedPlan M = merge_plans(work.data(), work.size(), l.data(), frame_words);
                if (const char *why = merge_fault(M, keep, l, frame_words)) { std::fprintf(stderr, "%s (%zu frames%s, reduce %u): %s\n", argv[a], keep.size(), rev ? ", reversed" : "", reduce, why); return 1; }
                frames += (int)keep.size();
            }
            any = true;
        }
        merged += any;
    }
    std::printf("merged %d files (%d frames), %d left to the fallback\n", merged, frames, skipped);
    return 0;
}
