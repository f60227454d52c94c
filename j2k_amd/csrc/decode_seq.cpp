// decode_seq.cpp -- see decode_seq.h
#include "decode_seq.h"

#include <cstring>

namespace j2k_hip {

std::string frames_differ(const FileHeader &a, const FileHeader &b, bool rgba)
{
    const Coding &p = a.cod, &q = b.cod;
    if (p.width != q.width || p.height != q.height || p.img_x0 != q.img_x0 || p.img_y0 != q.img_y0 || p.tile_w != q.tile_w ||
        p.tile_h != q.tile_h || p.tile_x0 != q.tile_x0 || p.tile_y0 != q.tile_y0 || p.ntx != q.ntx || p.nty != q.nty)
        return "image or tile geometry (SIZ)";
    if (p.ncomp != q.ncomp) return "number of components (SIZ)";
    for (uint32_t c = 0; c < p.ncomp && c < Coding::kMaxComps; ++c)
        if (p.cprec[c] != q.cprec[c] || p.csgnd[c] != q.csgnd[c] || p.cdx[c] != q.cdx[c] || p.cdy[c] != q.cdy[c])
            return "precision, sign or sub-sampling of component " + std::to_string(c) + " (SIZ)";
    if (p.numres != q.numres) return "number of resolutions (COD)";
    if (p.cbw != q.cbw || p.cbh != q.cbh) return "code-block size (COD)";
    if (a.cblk_style != b.cblk_style) return "code-block style (COD)";
    if (p.reversible != q.reversible) return "wavelet (COD)";
    if (p.mct != q.mct) return "component transform (COD)";
    if (p.prog != q.prog) return "progression order (COD)";
    if (p.layers != q.layers) return "number of layers (COD)";
    if (p.user_precincts != q.user_precincts || std::memcmp(p.ppx, q.ppx, sizeof p.ppx) != 0 || std::memcmp(p.ppy, q.ppy, sizeof p.ppy) != 0)
        return "precinct sizes (COD)";
    if (a.guard != b.guard || a.qstyle != b.qstyle || a.expn != b.expn || a.mant != b.mant) return "quantisation (QCD)";
    for (uint32_t c = 0; c < Coding::kMaxComps; ++c) {
        const FileHeader::Quant &x = a.qcc[c], &y = b.qcc[c];
        if (x.present != y.present || (x.present && (x.guard != y.guard || x.qstyle != y.qstyle || x.expn != y.expn || x.mant != y.mant)))
            return "quantisation of component " + std::to_string(c) + " (QCC)";
    }
    if (std::memcmp(a.roishift, b.roishift, sizeof a.roishift) != 0) return "region of interest (RGN)";
    if (a.poc.size() != b.poc.size()) return "progression order changes (POC)";
    for (size_t i = 0; i < a.poc.size(); ++i) {
        const PocEntry &x = a.poc[i], &y = b.poc[i];
        if (x.res0 != y.res0 || x.comp0 != y.comp0 || x.layer_end != y.layer_end || x.res_end != y.res_end || x.comp_end != y.comp_end || x.prog != y.prog)
            return "progression order changes (POC)";
    }
    if (rgba) { // what decides the mode, the opacity channel and the palette (rgba_plan.cpp: classify_rgba)
        if (a.enumcs != b.enumcs || (a.icc_len != 0) != (b.icc_len != 0)) return "colour space";
        if (a.alpha_mask != b.alpha_mask) return "opacity channel (cdef)";
        if (a.pal_entries != b.pal_entries || a.pal_columns != b.pal_columns || a.palette != b.palette ||
            std::memcmp(a.pal_column_of, b.pal_column_of, sizeof a.pal_column_of) != 0)
            return "palette";
    }
    return std::string();
}

MergedPlan merge_plans(DecodePlan *plans, size_t n, const size_t *file_len, uint64_t frame_words)
{
    MergedPlan M;
    M.frames.resize(n);
    size_t nb = 0, nseg = 0, ncw = 0;
    for (size_t f = 0; f < n; ++f) {
        SeqFrame &F = M.frames[f];
        F.file_off = M.file_bytes; F.file_len = file_len[f];
        M.file_bytes = (F.file_off + F.file_len + 63) & ~(uint64_t)63; // the next file starts 64-byte aligned
        F.arena_off = M.arena_bytes; F.arena_len = plans[f].arena_bytes;
        M.arena_bytes = (F.arena_off + F.arena_len + 15) & ~(uint64_t)15; // (a plan's arena is a multiple of 16 already)
        F.coef_off = (uint64_t)f * frame_words;
        F.blk_first = nb; F.blk_count = plans[f].blocks.size(); nb += F.blk_count;
        F.seg_first = nseg; F.seg_count = plans[f].segs.size(); nseg += F.seg_count;
        F.cwseg_first = ncw; F.cwseg_count = plans[f].cwsegs.size(); ncw += F.cwseg_count;
    }
    if (ncw > 0xffffffffull) throw Error(J2K_HIP_ERR_PARAM, "more codeword segments in one call than a block's 32-bit index reaches");
    if (n == 1) { // the frame's own plan: nothing to offset
        M.blocks = std::move(plans[0].blocks);
        M.segs = std::move(plans[0].segs);
        M.cwsegs = std::move(plans[0].cwsegs);
        M.frame_of.assign(nb, 0);
        return M;
    }
    M.blocks.reserve(nb); M.frame_of.reserve(nb); M.segs.reserve(nseg); M.cwsegs.reserve(ncw);
    for (size_t f = 0; f < n; ++f) {
        const SeqFrame &F = M.frames[f];
        for (DecBlock b : plans[f].blocks) {
            b.cw_off += F.arena_off;
            if (b.nsegs) b.seg_first += (uint32_t)F.cwseg_first;
            M.blocks.push_back(b);
            M.frame_of.push_back((uint32_t)f);
        }
        for (DecSeg s : plans[f].segs) {
            s.src += F.file_off; s.dst += F.arena_off;
            M.segs.push_back(s);
        }
        M.cwsegs.insert(M.cwsegs.end(), plans[f].cwsegs.begin(), plans[f].cwsegs.end());
        std::vector<DecBlock>().swap(plans[f].blocks);
        std::vector<DecSeg>().swap(plans[f].segs);
        std::vector<uint32_t>().swap(plans[f].cwsegs);
    }
    return M;
}

} // namespace j2k_hip
