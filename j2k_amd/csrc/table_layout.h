// table_layout.h -- the layouts of the device tables the encode path fills: one definition each, for the frames (encoder.cpp),
// the stage hooks (stage_hooks.cpp) and the rate control's device side (rate_device.h) alike.  Plain C++, no HIP header: a host
// program can include it (tests/native/table_layout_host.cpp).  The launch structs (kernels.h: T1Args, GatherArgs) are template
// parameters here for that reason.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "common.h"

namespace j2k_hip {

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// The Tier-1 results of nb code-blocks, as words of 32 bits.
//   meta       [numbps | npasses | len | nsym | err]: four columns of nb words, the kernels' error word behind them
//   passes     [decisions | nmsedec | rate]: three columns of [nb][kMaxPasses] (= kDevMaxPasses, kernels.h)
//   h_passes   what the host reads of `passes`: [nmsedec | rate] under rate control, the rate column alone for a styled frame
// The column accessors take the base of a device arena or of its host image.
struct T1Tables {
    size_t nb;
    explicit T1Tables(size_t nblks) : nb(nblks) {}
    static size_t row(size_t i) { return i * (size_t)kMaxPasses; }
    static constexpr size_t kColumns = 4;                              // of meta: a range of blocks is kColumns pieces ...
    size_t column_bytes() const { return nb * sizeof(uint32_t); }      // ... this far apart

    size_t meta_words() const { return 4 * nb + 1; } // the columns and the error word: what a reader copies
    size_t meta_bytes() const { return (4 * std::max<size_t>(1, nb) + 4) * sizeof(uint32_t); } // the arena, device and pinned
    size_t passes_words() const { return 3 * row(nb); }
    size_t passes_bytes() const { return 3 * row(std::max<size_t>(1, nb)) * sizeof(uint32_t); }
    size_t h_passes_bytes() const { return 2 * row(nb) * sizeof(uint32_t); }
    size_t h_rates_bytes() const { return row(nb) * sizeof(uint32_t); }

    template <class W> W *numbps(W *meta) const { return meta; }
    template <class W> W *npasses(W *meta) const { return meta + nb; }
    template <class W> W *len(W *meta) const { return meta + 2 * nb; }
    template <class W> W *nsym(W *meta) const { return meta + 3 * nb; }
    template <class W> W *err(W *meta) const { return meta + 4 * nb; }

    template <class W> W *pass_nsym(W *passes) const { return passes; }
    template <class W> W *pass_nmsedec(W *passes) const { return passes + row(nb); } // (signed sums in unsigned words)
    template <class W> W *pass_rate(W *passes) const { return passes + 2 * row(nb); }
    // the host image under rate control: one copy of the two columns from pass_nmsedec() on -- nmsedec at its base, then rate
    template <class W> W *h_rate(W *h_passes) const { return h_passes + row(nb); }

    // the eight table pointers of a T1Args
    template <class Args> void fill(Args &ta, uint32_t *meta, uint32_t *passes) const
    {
        ta.numbps = numbps(meta); ta.npasses = npasses(meta); ta.len = len(meta); ta.nsym = nsym(meta); ta.err = err(meta);
        ta.pass_nsym = pass_nsym(passes);
        ta.pass_nmsedec = reinterpret_cast<int *>(pass_nmsedec(passes));
        ta.pass_rate = pass_rate(passes);
    }
};

// The gather plan of one frame, device and pinned host alike:
// [blob][hdr_dst nh][cblk_dst nbd][seg_dst nseg][seg_src nseg] (64-bit) [hdr_src nh][hdr_len nh][seg_len nseg] (32-bit)
struct GatherTables {
    unsigned long long *hdr_dst, *cblk_dst, *seg_dst, *seg_src;
    unsigned int *hdr_src, *hdr_len, *seg_len;
};
struct GatherPlan {
    size_t nh = 0, nbd = 0, nseg = 0, blob_sz = 0, total = 0;
    GatherPlan() = default;
    GatherPlan(size_t blob_bytes, size_t nhdr, size_t nblks, size_t nsegs) : nh(nhdr), nbd(nblks), nseg(nsegs)
    {
        blob_sz = round_up(blob_bytes + 8, 16);
        total = round_up(blob_sz + nh * (8 + 4 + 4) + nbd * 8 + nseg * (8 + 8 + 4) + 64, 64);
    }
    GatherTables tables(uint8_t *base) const // (base: aligned to 8 bytes)
    {
        GatherTables t;
        t.hdr_dst = reinterpret_cast<unsigned long long *>(base + blob_sz);
        t.cblk_dst = t.hdr_dst + nh;
        t.seg_dst = t.cblk_dst + nbd; t.seg_src = t.seg_dst + nseg;
        t.hdr_src = reinterpret_cast<unsigned int *>(t.seg_src + nseg);
        t.hdr_len = t.hdr_src + nh; t.seg_len = t.hdr_len + nh;
        return t;
    }
    // what of a GatherArgs the plan decides, from the plan's device copy
    template <class Args> void fill(Args &ga, uint8_t *base) const
    {
        const GatherTables t = tables(base);
        ga.blob = base;
        ga.hdr_dst = t.hdr_dst; ga.cblk_dst = t.cblk_dst; ga.seg_dst = t.seg_dst; ga.seg_src = t.seg_src;
        ga.hdr_src = t.hdr_src; ga.hdr_len = t.hdr_len; ga.seg_len = t.seg_len;
        ga.nhdr = (int)nh; ga.nseg = (int)nseg;
    }
};

} // namespace j2k_hip
