// decoder.cpp -- orchestration of the MI355X DECODE path and its C ABI (include/j2k_hip.h, "decode" section).
//
// Replaces OpenJPEGCodec::ReadFile / GetFileInfo (reference: src/common/j2k_openjpeg_codec.cpp:451-586, :222-426):
//
//   file bytes (host)  ->  host Tier-2: boxes, headers, packet headers (decode_plan.cpp)
//   -> [H2D file]  ->  gather of every block's codeword pieces into one arena (gather.hip)
//   -> t1_decode (MQ decoder + bit modelling, one wavefront per code-block)  ->  t1_assemble (+ dequantisation)
//   -> inverse DWT, lowest resolution first, stopping `reduce` resolutions early (cp_reduce, :501)
//   -> inverse RCT / ICT, DC shift, clamp, CopyBuffer's depth conversion into the destination channels (:571)
//   -> [D2H into the host's strided channels]
//
// There is no CPU fallback: without a usable HIP device every entry point fails.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>
#include <limits>
#include <thread>

#include "decode_plan.h"
#include "decode_seq.h"
#include "handle.h"
#include "xyz_tables.h"

using namespace j2k_hip;

namespace {

// decode calls in progress per device, and the runtime's number of hardware queues (its own environment knob, read once)
constexpr int kMaxDevices = 64;
std::atomic<int> g_decoding[kMaxDevices];
struct Decoding {
    std::atomic<int> &c;
    int count;
    explicit Decoding(int device) : c(g_decoding[(device >= 0 && device < kMaxDevices) ? device : 0]) { count = c.fetch_add(1) + 1; }
    ~Decoding() { c.fetch_sub(1); }
    Decoding(const Decoding &) = delete;
    Decoding &operator=(const Decoding &) = delete;
};
// A table of the X'Y'Z' -> R'G'B' output stage on the device (j2k_hip_decode_set_xyz_to_rgb): the handle's copy, made and
// uploaded on s where the handle has none yet.  target 0: code -> linear light of component depth `depth`; 1..3: the thresholds
// of that target at destination depth `depth`, padded with +infinity.  Both hold max(2^depth, 4) words (whole float4s).
const float *xyz_inverse_device_table(j2k_hip_encoder *e, uint32_t target, uint32_t depth, hipStream_t s)
{
    for (const auto &t : e->xyz_inverse_tables)
        if (t->source == target && t->depth == depth) return t->dev.as<float>();
    auto t = std::make_unique<j2k_hip_encoder::XyzTable>();
    t->source = target; t->depth = depth;
    const size_t words = std::max<size_t>((size_t)1 << depth, 4);
    if (target) {
        t->host = xyz_othr_table(target, depth);
        t->host.resize(words, std::numeric_limits<float>::infinity());
    } else {
        t->host = xyz_delin_table(depth);
        t->host.resize(words, 0.0f);
    }
    t->dev.ensure(words * sizeof(float));
    HIP_CHECK(hipMemcpyAsync(t->dev.p, t->host.data(), words * sizeof(float), hipMemcpyHostToDevice, s));
    e->xyz_inverse_tables.push_back(std::move(t));
    return e->xyz_inverse_tables.back()->dev.as<float>();
}
// ... and what decode_rgba_args leaves to the owner of the tables: their device addresses and the matrix
void add_xyz_to_rgb(j2k_hip_encoder *e, DecRgbaArgs &a, hipStream_t s)
{
    if (!a.xyz_to_rgb) return;
    a.xyz_dl = xyz_inverse_device_table(e, 0, (uint32_t)a.cprec[0], s);
    a.xyz_othr = xyz_inverse_device_table(e, (uint32_t)a.xyz_to_rgb, (uint32_t)a.depth, s);
    xyz_inverse_matrix(a.xyz_n);
}

// rows [0, rows) split over a few host threads (strided per-sample copies of a large frame)
template <typename F> void parallel_rows(int rows, size_t work, F &&fn)
{
    const unsigned nt = work < (4u << 20) ? 1u : std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    if (nt <= 1) { fn(0, rows); return; }
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t) {
        const int a = (int)((long long)rows * t / nt), b = (int)((long long)rows * (t + 1) / nt);
        if (b > a) th.emplace_back([=, &fn] { fn(a, b); });
    }
    for (auto &t : th) t.join();
}

// The lane-per-block Tier-1 kernel's tables (t1_dec_lane.h), for decode_impl and the stage hook alike.  Blocks [0, n) form
// groups of 64 in their order (one wave each); a group's loop bounds are the maxima over its blocks, its output planes
// ([plane][stripe 16][8][lane 64] words) one more than the planes its longest block reaches.  Returns the words of all planes.
size_t lane_groups(const DecBlkDev *blk, size_t n, std::vector<DecGroupDev> &groups)
{
    size_t plane_words = 0;
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        DecGroupDev &G = groups[gi];
        G.plane_off = plane_words;
        for (size_t i = gi * 64; i < std::min(n, gi * 64 + 64); ++i) {
            G.maxpasses = std::max<unsigned>(G.maxpasses, blk[i].npasses);
            G.maxstripes = std::max<unsigned>(G.maxstripes, (unsigned)(blk[i].h + 3) / 4);
        }
        plane_words += (size_t)((G.maxpasses + 1) / 3 + 1) * 16 * 8 * 64;
    }
    return plane_words;
}
// per group: 16 x 64 x 64 state words + 16 x 4 x 64 edge words (t1lane::kGroupWords per lane), zero before the launch
size_t lane_state_bytes(size_t ngroups) { return std::max<size_t>(ngroups, 1) * ((16 * 64 + 16 * 4) * 64) * sizeof(uint32_t); }
size_t lane_planes_bytes(size_t plane_words) { return round_up(std::max<size_t>(plane_words, 64) * sizeof(uint32_t), 64); }

// The output stage's arguments, for decode_impl and the stage hook alike: everything launch_decode_output reads except
// dst[] (where the channels lie on the device is the caller's: a decode lays out spans, the hook has one buffer).
// Enforces kernels.h's preconditions on what it is given; the component planes' and the channels' extents are the caller's.
struct OutComp { const void *plane; uint32_t prec, sub_x, sub_y; };
void check_outplane(const j2k_hip_outplane &p)
{
    check_sample_type(p.sample_bits, p.depth, p.base, p.colbytes, p.rowbytes);
}
// (org_x, org_y: a region decode's window origin -- width and height are then the window's)
DecOutArgs decode_output_args(bool reversible, bool mct, int width, int height, long long stride, const OutComp *comps, uint32_t ncomp,
                              const j2k_hip_outplane *planes, uint32_t nplanes, int org_x = 0, int org_y = 0)
{
    if (ncomp < 1 || ncomp > 4 || !planes || nplanes < 1 || nplanes > 4) throw Error(J2K_HIP_ERR_PARAM, "1..4 components and destination channels");
    for (uint32_t c = 0; c < ncomp; ++c) {
        if (comps[c].prec < 1 || comps[c].prec > 16) throw Error(J2K_HIP_ERR_PARAM, "component precision outside 1..16");
        if (comps[c].sub_x < 1 || comps[c].sub_x > 255 || comps[c].sub_y < 1 || comps[c].sub_y > 255) throw Error(J2K_HIP_ERR_PARAM, "sub-sampling factor outside 1..255");
    }
    if (mct && ncomp < 3) throw Error(J2K_HIP_ERR_PARAM, "component transform on fewer than 3 components");
    if (mct)
        for (int c = 1; c < 3; ++c)
            if (comps[c].prec != comps[0].prec || comps[c].sub_x != comps[0].sub_x || comps[c].sub_y != comps[0].sub_y)
                throw Error(J2K_HIP_ERR_PARAM, "component transform on components of unlike precision or sub-sampling");
    DecOutArgs oa{};
    oa.stride = stride; oa.ncomp = (int)ncomp; oa.width = width; oa.height = height; oa.prec = (int)comps[0].prec;
    oa.reversible = reversible; oa.mct = mct; oa.org_x = org_x; oa.org_y = org_y;
    for (int c = 0; c < 4; ++c) { oa.cprec[c] = (int)comps[0].prec; oa.sub_x[c] = oa.sub_y[c] = 1; }
    for (uint32_t c = 0; c < ncomp; ++c) {
        oa.comp[c] = comps[c].plane;
        oa.cprec[c] = (int)comps[c].prec; oa.sub_x[c] = (int)comps[c].sub_x; oa.sub_y[c] = (int)comps[c].sub_y;
    }
    oa.nout = (int)std::min<uint32_t>(nplanes, ncomp); // reference: min(image->numcomps, channels), :532 and CopyBuffer's loop
    for (int c = 0; c < oa.nout; ++c) {
        const j2k_hip_outplane &p = planes[c];
        check_outplane(p);
        oa.colbytes[c] = p.colbytes; oa.rowbytes[c] = p.rowbytes;
        oa.dst_bytes[c] = (int)p.sample_bits / 8; oa.dst_depth[c] = (int)p.depth;
        oa.dst_w[c] = (int)std::min<uint32_t>(p.width, (uint32_t)width); oa.dst_h[c] = (int)std::min<uint32_t>(p.height, (uint32_t)height);
    }
    return oa;
}

// One job of a windowed inverse DWT launch: resolution rectangle `res` of a tile-component whose origin is word `off`, and
// what region_footprints found for it (absolute coordinates -> the region's own)
IdwtWinJob window_job(const IRect &res, const ResFootprint &f, long long off)
{
    IdwtWinJob j{};
    j.off = off;
    j.rw = res.x1 - res.x0; j.rh = res.y1 - res.y0; j.casx = res.x0 & 1; j.casy = res.y0 & 1;
    j.wx0 = f.win.x0 - res.x0; j.wx1 = f.win.x1 - res.x0; j.wy0 = f.win.y0 - res.y0; j.wy1 = f.win.y1 - res.y0;
    const int low0 = (res.y0 + 1) >> 1, high0 = res.y0 >> 1; // the bands' first rows
    j.ly0 = f.ly0 - low0; j.ly1 = f.ly1 - low0; j.hy0 = f.hy0 - high0; j.hy1 = f.hy1 - high0;
    return j;
}

// ---- The decode, for one frame and for the frames of a sequence call alike, in pieces that take a frame's base offsets:
// plan a frame (decode_plan.h) -- merge the plans of a group of frames (decode_seq.h) -- build the tables of the merged
// blocks -- launch gather, Tier-1 and the inverse DWT once for the group -- output and download frame by frame.  The
// single-frame entry points are a call of one frame in one group.

// a failure that belongs to one frame of a sequence call: the text begins with "frame k: "
struct FrameError : Error {
    uint32_t frame;
    FrameError(int c, uint32_t f, const std::string &m) : Error(c, "frame " + std::to_string(f) + ": " + m), frame(f) {}
};

// region (optional): the window of a region decode.  Null: the whole image, by the launches of every decode before regions.
// rgba (optional, one per frame): the output stage goes straight to R, G, B, A (rgba_out.hip); the frame's planes are then
// rgba's r, g, b[, a], already checked.  Everything before the last launch is the same decode.
// seq: a sequence entry point -- failures name their frame, and the output stage is the sequence kernels' one launch.
struct DecodeCall {
    const j2k_hip_file *files; uint32_t nframes;
    uint32_t subsample;
    const j2k_hip_rect *region;
    const j2k_hip_outplane *planes; uint32_t nplanes; // frame f: planes[f * nplanes + i]
    const j2k_hip_rgba_dst *rgba;
    bool on_device, seq;
};

// what the frames of a call share (they have one geometry): the decoded resolution and the layout of a frame's planes
struct Shape {
    uint32_t reduce = 0, R = 0, nd = 0; // resolutions dropped, highest resolution decoded, components decoded
    int ow = 0, oh = 0;                 // the image at the decoded resolution
    int pox[4] = {0, 0, 0, 0}, poy[4] = {0, 0, 0, 0};
    size_t stride = 0, plane_elems = 0;
    size_t frame_words() const { return plane_elems * nd; }
};
Shape frame_shape(const Coding &cod, uint32_t reduce)
{
    Shape S;
    S.reduce = reduce;
    S.R = cod.numres - 1 - reduce;
    // the image at the decoded resolution (opj_image_comp_header_update: both edges of the area are scaled, then subtracted)
    reduced_size(cod, reduce, S.ow, S.oh);
    if (S.ow <= 0 || S.oh <= 0) throw Error(J2K_HIP_ERR_PARAM, "Error reading file: nothing left of the image at this resolution");
    // origin of every component's plane: the image area's origin on the component's grid at the decoded resolution
    S.nd = cod.ncomp_out(); // components decoded: the first four (reference: min(numcomps, J2K_CODEC_MAX_CHANNELS), :278, :530)
    for (uint32_t c = 0; c < S.nd; ++c) {
        S.pox[c] = ceildivpow2((int)((cod.img_x0 + cod.cdx[c] - 1) / cod.cdx[c]), (int)reduce);
        S.poy[c] = ceildivpow2((int)((cod.img_y0 + cod.cdy[c] - 1) / cod.cdy[c]), (int)reduce);
    }
    S.stride = round_up((size_t)S.ow, 64);
    S.plane_elems = S.stride * (size_t)S.oh;
    return S;
}

// The destination channels' extents in the caller's address space.  Channels whose extents overlap (the samples of
// interleaved pixels) form one span that keeps its layout on the device; channels that lie apart (planar buffers,
// wherever they were allocated) are spans of their own.  dev: where a host destination's span lies in its frame's staged image
// (a span keeps its address modulo 256: the samples stay aligned as on the host).
struct Span { const uint8_t *lo, *hi; int ch[4]; int n; size_t dev; };
struct SpanLayout { Span spans[4]; int nspans = 0; size_t dev_bytes = 0, max_span = 0, base = 0; };
SpanLayout layout_spans(const DecOutArgs &oa, const j2k_hip_outplane *planes)
{
    SpanLayout L;
    struct Ext { const uint8_t *lo, *hi; int c; } ext[4];
    int ne = 0;
    for (int c = 0; c < oa.nout; ++c) {
        const j2k_hip_outplane &p = planes[c];
        if (oa.dst_w[c] <= 0 || oa.dst_h[c] <= 0) continue;
        const uint8_t *b = static_cast<const uint8_t *>(p.base);
        const uint8_t *corners[4] = {b, b + (ptrdiff_t)(oa.dst_h[c] - 1) * p.rowbytes, b + (ptrdiff_t)(oa.dst_w[c] - 1) * p.colbytes,
                                     b + (ptrdiff_t)(oa.dst_h[c] - 1) * p.rowbytes + (ptrdiff_t)(oa.dst_w[c] - 1) * p.colbytes};
        Ext x{corners[0], corners[0] + oa.dst_bytes[c], c};
        for (const uint8_t *q : corners) { x.lo = std::min(x.lo, q); x.hi = std::max(x.hi, q + oa.dst_bytes[c]); }
        ext[ne++] = x;
    }
    if (!ne) throw Error(J2K_HIP_ERR_PARAM, "no destination channel has any sample");
    std::sort(ext, ext + ne, [](const Ext &x, const Ext &y) { return x.lo < y.lo; });
    for (int i = 0; i < ne; ++i) {
        if (L.nspans && ext[i].lo < L.spans[L.nspans - 1].hi) {
            Span &S = L.spans[L.nspans - 1];
            S.hi = std::max(S.hi, ext[i].hi); S.ch[S.n++] = ext[i].c;
        } else {
            Span &S = L.spans[L.nspans++];
            S = Span{ext[i].lo, ext[i].hi, {ext[i].c, 0, 0, 0}, 1, 0};
        }
    }
    for (int k = 0; k < L.nspans; ++k) {
        L.spans[k].dev = round_up(L.dev_bytes, 256) + (reinterpret_cast<uintptr_t>(L.spans[k].lo) & 255);
        L.dev_bytes = L.spans[k].dev + (size_t)(L.spans[k].hi - L.spans[k].lo);
        L.max_span = std::max(L.max_span, (size_t)(L.spans[k].hi - L.spans[k].lo));
    }
    return L;
}

// One frame's samples from its staged image on the device (dimg) into the host's channels: queued behind the output launch on
// s.  staged: the pinned staging buffer has been used since the stream was last idle (it is one span's at a time).
void download_spans(j2k_hip_encoder *e, const DecOutArgs &oa, const j2k_hip_outplane *planes, const SpanLayout &L, const uint8_t *dimg,
                    bool &staged, hipStream_t s)
{
    std::vector<hipEvent_t> band_ev;
    struct EvGuard { std::vector<hipEvent_t> &v; ~EvGuard() { for (hipEvent_t x : v) if (x) (void)hipEventDestroy(x); } } ev_guard{band_ev};
    for (int k = 0; k < L.nspans; ++k) {
        const Span &S = L.spans[k];
        const uint8_t *lo = S.lo;
        const size_t span = (size_t)(S.hi - S.lo);
        const uint8_t *dbase = dimg + S.dev;
        const int c0 = S.ch[0];
        // Do the span's channels cover every byte of it (interleaved pixels with every sample decoded, or one planar
        // channel, no row padding)?  Then it goes straight into the host's buffer.  Otherwise only the channel samples
        // may be written (the reference's CopyBuffer touches nothing else): through a staging copy.
        bool same = true;
        const long long P0 = oa.colbytes[c0];
        long long covered = 0;
        for (int i = 0; i < S.n; ++i) {
            const int c = S.ch[i];
            same = same && oa.colbytes[c] == P0 && oa.rowbytes[c] == oa.rowbytes[c0] && oa.dst_w[c] == oa.dst_w[c0] && oa.dst_h[c] == oa.dst_h[c0];
            covered += oa.dst_bytes[c];
        }
        const bool full = same && P0 > 0 && covered == P0 && oa.rowbytes[c0] == P0 * oa.dst_w[c0] && span == (size_t)(oa.rowbytes[c0] * oa.dst_h[c0]);
        if (full) {
            HIP_CHECK(hipMemcpyAsync(const_cast<uint8_t *>(lo), dbase, span, hipMemcpyDeviceToHost, s));
            continue;
        }
        if (staged) HIP_CHECK(hipStreamSynchronize(s)); // (the staging buffer is one span's at a time)
        staged = true;
        e->h_outimg.ensure(L.max_span + 16);
        const uint8_t *stg = e->h_outimg.as<uint8_t>();
        // Two layouts get whole-word copies: the channels of one interleaved pixel of 4 or 8 bytes (After Effects'
        // ARGB32 / ARGB64 with R, G, B decoded and A kept: one masked word per pixel) and planar rows.
        bool pixels = same && (P0 == 4 || P0 == 8) && oa.rowbytes[c0] > 0;
        // a pixel-sized window starting at the lowest channel's sample holds one sample of every channel (its remaining
        // bytes belong to samples that are not decoded: they pass through)
        uint64_t mask = 0;
        for (int i = 0; i < S.n && pixels; ++i) {
            const int c = S.ch[i];
            const ptrdiff_t off = static_cast<const uint8_t *>(planes[c].base) - lo;
            pixels = off >= 0 && off + oa.dst_bytes[c] <= P0;
            if (pixels) mask |= (oa.dst_bytes[c] == 1 ? 0xffull : (oa.dst_bytes[c] == 2 ? 0xffffull : 0xffffffffull)) << (8 * off);
        }
        // The download comes in row bands; the host merges band k while band k + 1 is on its way (a frame of pixels:
        // the rows of the span in order; other layouts: one piece).
        const int bands = pixels ? (int)std::max<size_t>(1, std::min<size_t>({(size_t)8, span >> 25, (size_t)oa.dst_h[c0]})) : 1;
        auto band_row = [&](int b) { return (int)((long long)oa.dst_h[c0] * b / bands); };
        const size_t ev0 = band_ev.size();
        for (int b = 0; b < bands; ++b) {
            const size_t b0 = bands > 1 ? (size_t)band_row(b) * (size_t)oa.rowbytes[c0] : 0;
            const size_t b1 = (bands > 1 && b + 1 < bands) ? (size_t)band_row(b + 1) * (size_t)oa.rowbytes[c0] : span;
            HIP_CHECK(hipMemcpyAsync(e->h_outimg.as<uint8_t>() + b0, dbase + b0, b1 - b0, hipMemcpyDeviceToHost, s));
            band_ev.push_back(nullptr);
            HIP_CHECK(hipEventCreateWithFlags(&band_ev.back(), hipEventDisableTiming));
            HIP_CHECK(hipEventRecord(band_ev.back(), s));
        }
        if (pixels) {
            const int w = oa.dst_w[c0];
            const long long rb = oa.rowbytes[c0];
            const bool wide = P0 == 8;
            for (int b = 0; b < bands; ++b) {
                const int band0 = band_row(b), hgt = band_row(b + 1) - band0;
                HIP_CHECK(hipEventSynchronize(band_ev[ev0 + (size_t)b]));
                parallel_rows(hgt, (size_t)w * hgt, [&](int y0, int y1) {
                    for (int y = band0 + y0; y < band0 + y1; ++y) {
                        const uint8_t *sp = stg + (long long)y * rb;
                        uint8_t *dp = const_cast<uint8_t *>(lo) + (long long)y * rb;
                        if (wide) {
                            for (int x = 0; x + 1 < w; ++x) {
                                uint64_t u, v;
                                std::memcpy(&u, dp + 8 * (size_t)x, 8); std::memcpy(&v, sp + 8 * (size_t)x, 8);
                                u = (u & ~mask) | (v & mask);
                                std::memcpy(dp + 8 * (size_t)x, &u, 8);
                            }
                        } else {
                            const uint32_t m32 = (uint32_t)mask;
                            for (int x = 0; x + 1 < w; ++x) {
                                uint32_t u, v;
                                std::memcpy(&u, dp + 4 * (size_t)x, 4); std::memcpy(&v, sp + 4 * (size_t)x, 4);
                                u = (u & ~m32) | (v & m32);
                                std::memcpy(dp + 4 * (size_t)x, &u, 4);
                            }
                        }
                        // the row's last pixel sample by sample: its window would reach past the row
                        const size_t last = (size_t)(w - 1) * (size_t)P0;
                        for (int i = 0; i < S.n; ++i) {
                            const int c = S.ch[i];
                            const ptrdiff_t off = static_cast<const uint8_t *>(planes[c].base) - lo;
                            std::memcpy(dp + last + off, sp + last + off, (size_t)oa.dst_bytes[c]);
                        }
                    }
                });
            }
        } else {
            HIP_CHECK(hipEventSynchronize(band_ev[ev0]));
            for (int i = 0; i < S.n; ++i) {
                const int c = S.ch[i];
                uint8_t *ub = static_cast<uint8_t *>(planes[c].base);
                const ptrdiff_t off = ub - lo;
                const int w = oa.dst_w[c], hgt = oa.dst_h[c], sb = oa.dst_bytes[c];
                const long long cb = oa.colbytes[c], rb = oa.rowbytes[c];
                parallel_rows(hgt, (size_t)w * hgt, [&](int y0, int y1) {
                    for (int y = y0; y < y1; ++y) {
                        const uint8_t *sp = stg + off + (long long)y * rb;
                        uint8_t *dp = ub + (long long)y * rb;
                        if (cb == sb) std::memcpy(dp, sp, (size_t)w * sb); // a planar channel: the row is contiguous
                        else if (sb == 1) for (int x = 0; x < w; ++x) dp[(long long)x * cb] = sp[(long long)x * cb];
                        else if (sb == 2) for (int x = 0; x < w; ++x) std::memcpy(dp + (long long)x * cb, sp + (long long)x * cb, 2);
                        else for (int x = 0; x < w; ++x) std::memcpy(dp + (long long)x * cb, sp + (long long)x * cb, 4);
                    }
                });
            }
        }
    }
}

// Waves of the lane-per-block kernel the chip holds at once (kernels.h): a group of a sequence call has at most this many.
int lane_waves_resident()
{
    static const int w = t1_decode_lanes_resident_waves();
    return w;
}
// a group's arenas (files, codewords, two plane sets, state / planes / masks, staged output) stay under this share of the
// device memory that is free, counting what the handle's arenas hold already
constexpr double kSeqMemoryShare = 0.5;

// One group: frames [first, first + nf) of the call, plans[0 .. nf) theirs.  file_uploaded: the (single) file is on its way to
// d_file already and EV_START is recorded.  Adds to st.
void decode_group(j2k_hip_encoder *e, const DecodeCall &call, const Shape &S, DecodePlan *plans, uint32_t first, uint32_t nf,
                  const Decoding &decoding, bool file_uploaded, j2k_hip_stats &st)
{
    hipStream_t s = e->stream;
    const FileHeader &H = plans[0].hdr;
    const Coding &cod = H.cod;
    const Geometry &g = plans[0].geo; // (one geometry, and one set of windows, for every frame)
    const uint32_t reduce = S.reduce, R = S.R, nd = S.nd, nplanes = call.nplanes;
    const size_t stride = S.stride, plane_elems = S.plane_elems, frame_words = S.frame_words();
    const j2k_hip_rect *const region = call.region;

    // ---- the frames' plans as one, and their files back to back on the device
    std::vector<size_t> lens(nf);
    for (uint32_t f = 0; f < nf; ++f) lens[f] = call.files[first + f].len;
    MergedPlan M = merge_plans(plans, nf, lens.data(), frame_words);
    if (!file_uploaded) {
        HIP_CHECK(hipEventRecord(e->ev[EV_START], s));
        e->d_file.ensure(M.file_bytes + 64);
        for (uint32_t f = 0; f < nf; ++f)
            HIP_CHECK(hipMemcpyAsync(e->d_file.as<uint8_t>() + M.frames[f].file_off, call.files[first + f].data, lens[f], hipMemcpyHostToDevice, s));
    }
    const size_t plane_bytes = frame_words * sizeof(int32_t) * nf;
    e->Z.ensure(plane_bytes);
    e->Q.ensure(plane_bytes);
    e->geo_valid = false; e->seq_valid = false; // the encode path's cached geometry belongs to other planes

    // ---- where every frame's samples go: the channels' geometry, their spans, and for host destinations the staged images
    const int out_w = region ? (int)region->w : S.ow, out_h = region ? (int)region->h : S.oh;
    const int org_x = region ? (int)region->x : 0, org_y = region ? (int)region->y : 0;
    RgbaClass cls;
    if (call.rgba) cls = classify_rgba(H);
    std::vector<DecOutArgs> oas(nf);
    std::vector<SpanLayout> lay(nf);
    std::vector<OutComp> ocs((size_t)nf * 4);
    size_t out_bytes = 0;
    for (uint32_t f = 0; f < nf; ++f) {
        const j2k_hip_outplane *planes = call.planes + (size_t)(first + f) * nplanes;
        OutComp *oc = &ocs[(size_t)f * 4];
        for (uint32_t c = 0; c < nd; ++c) oc[c] = OutComp{e->Z.as<int32_t>() + f * frame_words + c * plane_elems, cod.cprec[c], cod.cdx[c], cod.cdy[c]};
        DecOutArgs &oa = oas[f];
        if (call.rgba) { // the channels' geometry alone, for the spans: the RGBA kernel's arguments need the channels' device addresses
            oa.nout = (int)nplanes;
            for (int c = 0; c < oa.nout; ++c) {
                const j2k_hip_outplane &p = planes[c];
                oa.colbytes[c] = p.colbytes; oa.rowbytes[c] = p.rowbytes; oa.dst_bytes[c] = (int)p.sample_bits / 8;
                oa.dst_w[c] = (int)std::min<uint32_t>(p.width, (uint32_t)out_w); oa.dst_h[c] = (int)std::min<uint32_t>(p.height, (uint32_t)out_h);
            }
        } else oa = decode_output_args(cod.reversible, cod.mct, out_w, out_h, (long long)stride, oc, nd, planes, nplanes, org_x, org_y);
        try {
            lay[f] = layout_spans(oa, planes);
        } catch (const Error &x) {
            if (call.seq) throw FrameError(x.code, first + f, x.what());
            throw;
        }
        if (!call.on_device) {
            lay[f].base = round_up(out_bytes, 256);
            out_bytes = lay[f].base + lay[f].dev_bytes;
        }
    }
    if (!call.on_device) e->d_outimg.ensure(out_bytes + 16);
    for (uint32_t f = 0; f < nf; ++f) {
        const j2k_hip_outplane *planes = call.planes + (size_t)(first + f) * nplanes;
        if (call.on_device) {
            for (int c = 0; c < oas[f].nout; ++c) oas[f].dst[c] = static_cast<uint8_t *>(planes[c].base);
            continue;
        }
        for (int k = 0; k < lay[f].nspans; ++k)
            for (int i = 0; i < lay[f].spans[k].n; ++i) {
                const int c = lay[f].spans[k].ch[i];
                oas[f].dst[c] = e->d_outimg.as<uint8_t>() + lay[f].base + lay[f].spans[k].dev + (static_cast<const uint8_t *>(planes[c].base) - lay[f].spans[k].lo);
            }
    }
    // the output stage's arguments (a sequence call: what the frames share, and the descriptor of each)
    std::vector<DecRgbaArgs> ras;
    std::vector<DecSeqFrameDev> desc(call.seq ? nf : 0);
    if (call.rgba) {
        ras.resize(nf);
        for (uint32_t f = 0; f < nf; ++f) {
            j2k_hip_rgba_dst d = call.rgba[first + f];
            j2k_hip_outplane *const ch[4] = {&d.r, &d.g, &d.b, &d.a};
            for (int c = 0; c < oas[f].nout; ++c) ch[c]->base = oas[f].dst[c];
            RgbaComp rc[4] = {};
            for (int c = 0; c < cls.ncomp; ++c) rc[c] = RgbaComp{ocs[(size_t)f * 4 + c].plane, ocs[(size_t)f * 4 + c].prec, ocs[(size_t)f * 4 + c].sub_x, ocs[(size_t)f * 4 + c].sub_y};
            ras[f] = decode_rgba_args(cod.reversible, cod.mct, out_w, out_h, (long long)stride, rc, cls, d, nplanes == 4, org_x, org_y, e->dec_xyz_to_rgb);
        }
        add_xyz_to_rgb(e, ras[0], s); // (the launch reads frame 0's arguments; the tables go up on s ahead of it)
        for (uint32_t f = 1; f < nf; ++f) // one record form for the launch: the packed one only where every frame has it, slots alike
            if (!ras[f].packed || std::memcmp(ras[f].slot, ras[0].slot, sizeof ras[0].slot) != 0) ras[0].packed = 0;
    }
    for (uint32_t f = 0; f < nf && call.seq; ++f) {
        DecSeqFrameDev &D = desc[f];
        D = DecSeqFrameDev{};
        D.comp_off = (unsigned long long)f * frame_words;
        for (int c = 0; c < 4; ++c) {
            if (call.rgba) {
                D.dst[c] = ras[f].dst[c]; D.colbytes[c] = ras[f].colbytes[c]; D.rowbytes[c] = ras[f].rowbytes[c];
                D.dst_w[c] = ras[f].dst_w[c]; D.dst_h[c] = ras[f].dst_h[c];
            } else {
                D.dst[c] = oas[f].dst[c]; D.colbytes[c] = oas[f].colbytes[c]; D.rowbytes[c] = oas[f].rowbytes[c];
                D.dst_w[c] = oas[f].dst_w[c]; D.dst_h[c] = oas[f].dst_h[c];
            }
        }
        if (call.rgba) { D.pix = ras[f].pix; D.pix_rowbytes = ras[f].pix_rowbytes; }
    }

    // ---- a file cut short: the tiles for which no tile-part arrived.  Their samples are component value 0 (decode_plan.h), so
    // behind the inverse DWT their rectangles of the planes get the word the output stage turns into 0: minus the DC level it
    // adds.  A signed component's 0 is a zero coefficient already (the output stage adds the offset the host's conversion
    // wants), and behind the inverse component transform components 1 and 2 are differences: zero.  The rectangles are the
    // inverse DWT's jobs of the top resolution.  Complete files: no job, no launch.
    std::vector<FillJob> fills;
    int fill_w = 0, fill_h = 0;
    for (uint32_t f = 0; f < nf; ++f) {
        if (!plans[f].tiles_missing) continue;
        for (size_t t = 0; t < g.tiles.size(); ++t) {
            if (plans[f].tile_arrived[t]) continue;
            for (uint32_t c = 0; c < nd; ++c) {
                if (cod.csgnd[c] || (cod.mct && (c == 1 || c == 2))) continue;
                const TileComp &TC = g.tiles[t].comps[c];
                const Resolution &Rs = TC.res[R];
                FillJob j{};
                j.w = Rs.x1 - Rs.x0; j.h = Rs.y1 - Rs.y0;
                if (j.w <= 0 || j.h <= 0) continue;
                j.off = (long long)(f * frame_words) + (long long)c * (long long)plane_elems +
                        (long long)(ceildivpow2(TC.y0, (int)reduce) - S.poy[c]) * (long long)stride + (ceildivpow2(TC.x0, (int)reduce) - S.pox[c]);
                const int dc = 1 << (cod.cprec[c] - 1);
                if (cod.reversible) j.word = (unsigned)-dc;
                else { const float v = -(float)dc; std::memcpy(&j.word, &v, sizeof v); }
                fills.push_back(j);
                fill_w = std::max(fill_w, j.w); fill_h = std::max(fill_h, j.h);
            }
        }
    }

    // ---- tables to the device
    const size_t nb = M.blocks.size(), nseg = M.segs.size();
    // Tier-1 kernel.  A lane per block (t1_dec_lane.h): all its waves are resident at once, so the launch lasts as long as
    // its longest wave -- about 1.35 ms per coding pass of 64 x 64 blocks, whatever the number of blocks up to ~1000 waves.
    // A wave per block (t1_decode_kernel) runs a block's chain 3-4 times faster but is bound by the CUs' scalar units in
    // bulk: ~0.75 ns per codeword byte of the whole file.  Big files take the lanes, small ones the waves
    // (t1dec_lanes: 1 = by these estimates, 2 = always lanes, 0 = never).  The frames of a sequence call count as one file:
    // their blocks share the launches, so the bulk estimate sees all their bytes and the lane estimate stays one launch's.
    uint64_t cw_bytes = 0;
    uint32_t most_passes = 0, most_rows = 0;
    for (const DecBlock &b : M.blocks) {
        cw_bytes += b.cw_len;
        most_passes = std::max(most_passes, b.npasses);
        most_rows = std::max<uint32_t>(most_rows, g.cblks[b.cblk].h);
    }
    // With other decodes in flight on the device (hosts read image sequences from several threads) the balance shifts: the
    // wave kernel's bound is the device's -- k frames take k times as long -- while lane launches of k frames run side by
    // side (a frame's lane waves fill a fraction of the SIMDs) as far as the runtime has hardware queues for their streams
    // (GPU_MAX_HW_QUEUES, 4 unless the host raised it: 4096 x 2160 frames from 8 threads: 100 frames/s with 24 queues against
    // 55 with the wave kernel; with 4 queues 47).
    const int share = std::max(1, std::min({decoding.count, hw_queues() / 3, 8}));
    const double lanes_ms = 1.35 * most_passes * ((most_rows + 3) / 4) / 16.0, waves_ms = 5.0 + 0.75e-6 * (double)cw_bytes;
    // (code-block styles other than the default are the lane kernel's alone)
    const bool lanes = H.cblk_style != 0 || tuning().t1dec_lanes == 2 || (tuning().t1dec_lanes == 1 && lanes_ms / share < waves_ms);
    // The tables are built in their final order straight into the pinned staging buffer: the order comes from sorts of
    // small keys (the file is on the device by now and the launches wait for these tables: 3 ms of sorting and copying
    // whole entries for the 49 152 blocks of an 8K frame, 0.6 ms this way).
    auto passes_of = [](const DecBlock &b) { return t1dec_passes(b.numbps, b.npasses); };
    // lane-per-block Tier-1: the blocks of a wave walk their passes in step, so blocks with the same number of coding
    // passes (then of similar codeword length) share a wave -- every lane of it ends at about the same time.
    // All lane waves are resident at once, so the launch lasts as long as its heaviest block (~8 us per codeword byte of
    // it).  The wave-per-block kernel runs one block's chain 3-4 times faster (~2.4 us per byte) and is bound by the
    // scalar units only in bulk (~0.67 ns per byte of all its blocks): the few heaviest blocks -- the tail of the
    // distribution -- go to it, on a second stream beside the lane launch (t1dec_tail = 0: never, n >= 2: 1/n of the blocks).
    // (stable counting sorts of block indices: keys descending, ties in the order they came in)
    std::vector<uint32_t> order(nb), scratch(nb), count;
    for (size_t i = 0; i < nb; ++i) order[i] = (uint32_t)i;
    auto sort_desc = [&](size_t first_k, uint32_t key_max, auto &&key_of) { // order[first_k..) by key_of(index) descending, 11 bits a pass
        for (uint32_t shift = 0; shift < 32 && (shift == 0 || (key_max >> shift) != 0); shift += 11) {
            count.assign(2049, 0);
            for (size_t k = first_k; k < nb; ++k) ++count[1 + (((key_max - key_of(order[k])) >> shift) & 2047u)];
            for (size_t d = 0; d < 2048; ++d) count[d + 1] += count[d];
            for (size_t k = first_k; k < nb; ++k) scratch[first_k + count[((key_max - key_of(order[k])) >> shift) & 2047u]++] = order[k];
            std::copy(scratch.begin() + (ptrdiff_t)first_k, scratch.end(), order.begin() + (ptrdiff_t)first_k);
        }
    };
    size_t nheavy = 0;
    if (lanes) {
        uint32_t longest = 0;
        for (const DecBlock &b : M.blocks) longest = std::max(longest, b.cw_len);
        sort_desc(0, longest, [&](uint32_t i) { return M.blocks[i].cw_len; }); // longest codeword first
        auto len_at = [&](size_t k) { return (double)M.blocks[order[k]].cw_len; };
        if (H.cblk_style != 0) nheavy = 0;
        else if (tuning().t1dec_tail >= 2) nheavy = std::min(nb, std::max<size_t>(1, nb / (size_t)tuning().t1dec_tail)); // (tests: a fixed share, whatever the sizes)
        else if (tuning().t1dec_tail && nb > 128 && decoding.count == 1) { // (frames in flight: nobody waits for one frame's tail, and a second
                                                                          //  stream per handle is a hardware queue the runtime may not have)
            const double lane_ms_per_byte = 8.1e-3, chain_ms_per_byte = 2.4e-3, bulk_ms_per_byte = 0.67e-6;
            const size_t kmax = nb / 2;
            std::vector<double> cost(kmax / 64 + 1);
            double cum = 0, best = 1e30;
            for (size_t k = 0, i = 0; k <= kmax; k += 64) {
                for (; i < k; ++i) cum += len_at(i);
                const double wave = k ? std::max(chain_ms_per_byte * len_at(0), bulk_ms_per_byte * cum) : 0.0;
                cost[k / 64] = std::max(lane_ms_per_byte * len_at(k), wave);
                best = std::min(best, cost[k / 64]);
            }
            for (size_t k = 0; k <= kmax; k += 64)
                if (cost[k / 64] <= 1.02 * best) { nheavy = k; break; } // the shortest tail that gets (nearly) all of the gain
            if (cost[0] <= 1.1 * best) nheavy = 0;                      // (a flat distribution: nothing worth a second launch)
        }
        // the lanes' blocks: most passes first (they are in the order of their codeword lengths already)
        sort_desc(nheavy, most_passes, [&](uint32_t i) { return passes_of(M.blocks[i]); });
    }
    // masks of the wave-per-block kernel's blocks (all of them, or the tail beside the lanes)
    const size_t nwave = lanes ? nheavy : nb;
    std::vector<size_t> mask_off(nwave + 1, 0);
    for (size_t k = 0; k < nwave; ++k) mask_off[k + 1] = mask_off[k] + (size_t)(M.blocks[order[k]].numbps + 1) * 64;
    const size_t mask_words = mask_off[nwave];
    const size_t nl = nb - nheavy;
    std::vector<DecGroupDev> groups(lanes ? (nl + 63) / 64 : 0);

    // one pinned table: block table | groups | seg dst | seg src | seg len | codeword segments | frame descriptors | fill jobs
    const size_t grp_base = round_up(nb * sizeof(DecBlkDev), 16);
    const size_t seg_base = grp_base + round_up(groups.size() * sizeof(DecGroupDev), 16);
    const size_t cwseg_base = round_up(seg_base + nseg * (8 + 8 + 4), 16);
    const size_t desc_base = round_up(cwseg_base + M.cwsegs.size() * sizeof(uint32_t), 16);
    const size_t fill_base = round_up(desc_base + desc.size() * sizeof(DecSeqFrameDev), 16);
    const size_t tab_bytes = fill_base + fills.size() * sizeof(FillJob) + 64;
    e->h_dtab.ensure(tab_bytes);
    e->d_dblk.ensure(tab_bytes);
    uint8_t *ht = e->h_dtab.as<uint8_t>();
    DecBlkDev *const dblk = reinterpret_cast<DecBlkDev *>(ht);
    std::vector<uint32_t> tile_pos(cod.ntiles(), 0);
    for (size_t t = 0; t < g.tiles.size(); ++t) tile_pos[g.tiles[t].index] = (uint32_t)t;
    float steps[4][3 * 32 + 2]; // 0.5 x step size of every band of every component
    const uint32_t nbands = 3 * (cod.numres - 1) + 1;
    for (uint32_t c = 0; c < nd; ++c)
        for (uint32_t bi = 0; bi < nbands && bi < 3 * 32 + 2; ++bi) steps[c][bi] = 0.5f * H.band_stepsize(bi, c);
    for (size_t k = 0; k < nb; ++k) scratch[order[k]] = (uint32_t)k; // block -> its place in the table
    auto fill = [&](size_t i0, size_t i1) { // (blocks in the plan's order: the geometry is read front to back)
        for (size_t i = i0; i < i1; ++i) {
            const DecBlock &b = M.blocks[i];
            const size_t k = scratch[i];
            const Cblk &c = g.cblks[b.cblk];
            const Tile &T = g.tiles[tile_pos[c.tile]];
            const uint32_t bandidx = c.res == 0 ? 0u : 3u * (c.res - 1) + 1u + c.band;
            DecBlkDev d{};
            d.cw_off = b.cw_off; d.cw_len = b.cw_len;
            d.mask_off = k < nwave ? mask_off[k] : 0;
            const TileComp &TC = T.comps[c.comp]; // (a sub-sampled component lives in the top-left part of its plane)
            const int tx = ceildivpow2(TC.x0, (int)reduce), ty = ceildivpow2(TC.y0, (int)reduce);
            d.coef_off = M.frames[M.frame_of[i]].coef_off + (unsigned long long)c.comp * plane_elems +
                         (unsigned long long)(ty - S.poy[c.comp] + (int)(c.py - (uint32_t)TC.y0)) * stride +
                         (unsigned long long)(tx - S.pox[c.comp] + (int)(c.px - (uint32_t)TC.x0));
            d.stepsize = steps[c.comp][bandidx];
            d.w = c.w; d.h = c.h; d.orient = c.orient;
            d.numbps = (unsigned char)b.numbps;
            d.seg_off = b.seg_first; d.nsegs = (unsigned short)b.nsegs; d.roishift = (unsigned char)b.roishift;
            d.npasses = (unsigned short)passes_of(b);
            dblk[k] = d;
        }
    };
    if (nb >= 16384) { // (a few threads for a big frame's table)
        const unsigned nt = std::min(4u, std::max(1u, std::thread::hardware_concurrency()));
        std::vector<std::thread> th;
        for (unsigned t = 1; t < nt; ++t) th.emplace_back(fill, nb * t / nt, nb * (t + 1) / nt);
        fill(0, nb / nt);
        for (auto &t : th) t.join();
    } else fill(0, nb);
    const size_t plane_words = lane_groups(dblk + nheavy, nl, groups);
    if (!groups.empty()) std::memcpy(ht + grp_base, groups.data(), groups.size() * sizeof(DecGroupDev));
    uint64_t *h_sdst = reinterpret_cast<uint64_t *>(ht + seg_base), *h_ssrc = h_sdst + nseg;
    uint32_t *h_slen = reinterpret_cast<uint32_t *>(h_ssrc + nseg);
    for (size_t i = 0; i < nseg; ++i) { h_sdst[i] = M.segs[i].dst; h_ssrc[i] = M.segs[i].src; h_slen[i] = M.segs[i].len; }
    if (!M.cwsegs.empty()) std::memcpy(ht + cwseg_base, M.cwsegs.data(), M.cwsegs.size() * sizeof(uint32_t));
    if (!desc.empty()) std::memcpy(ht + desc_base, desc.data(), desc.size() * sizeof(DecSeqFrameDev));
    if (!fills.empty()) std::memcpy(ht + fill_base, fills.data(), fills.size() * sizeof(FillJob));
    HIP_CHECK(hipMemcpyAsync(e->d_dblk.p, ht, tab_bytes, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipEventRecord(e->ev[EV_UPLOAD], s));

    // ---- codeword arena
    e->d_cw.ensure(M.arena_bytes + kCwArenaTail);
    if (nseg) {
        GatherArgs ga{};
        uint8_t *dt = e->d_dblk.as<uint8_t>();
        ga.dst = e->d_cw.as<uint8_t>();
        ga.out = e->d_file.as<uint8_t>();
        ga.seg_dst = reinterpret_cast<const unsigned long long *>(dt + seg_base);
        ga.seg_src = ga.seg_dst + nseg;
        ga.seg_len = reinterpret_cast<const unsigned int *>(ga.seg_src + nseg);
        ga.nseg = (int)nseg;
        launch_gather(ga, s);
    }

    // ---- Tier-1
    HIP_CHECK(hipMemsetAsync(e->Z.p, 0, plane_bytes, s)); // blocks without data, bands of absent packets
    T1DecArgs ta{};
    ta.cw = e->d_cw.as<uint8_t>();
    ta.coef = e->Z.p; ta.stride = (long long)stride;
    ta.blks = e->d_dblk.as<DecBlkDev>(); ta.nblks = (int)nb; ta.reversible = cod.reversible;
    ta.cwsegs = reinterpret_cast<const unsigned *>(e->d_dblk.as<uint8_t>() + cwseg_base); ta.style = H.cblk_style;
    if (lanes) {
        // per group: 16 x 64 x 64 state words (zero: nothing significant yet) and the planes' output; then the tail's masks
        const size_t state_bytes = lane_state_bytes(groups.size());
        const size_t planes_bytes = lane_planes_bytes(plane_words);
        e->d_masks.ensure(state_bytes + planes_bytes + std::max<size_t>(mask_words, 64) * 8);
        HIP_CHECK(hipMemsetAsync(e->d_masks.p, 0, state_bytes, s));
        T1DecArgs tl = ta;
        tl.blks = ta.blks + nheavy; tl.nblks = (int)(nb - nheavy);
        tl.state = e->d_masks.as<unsigned>();
        tl.planes = tl.state + state_bytes / sizeof(uint32_t);
        tl.groups = reinterpret_cast<const DecGroupDev *>(e->d_dblk.as<uint8_t>() + grp_base);
        if (nheavy) { // the tail, beside the lanes (it needs the arena and the cleared planes: fork here)
            hipStream_t s2 = coder_stream(e, 0);
            HIP_CHECK(hipEventRecord(e->ev[EV_FRONT], s));
            HIP_CHECK(hipStreamWaitEvent(s2, e->ev[EV_FRONT], 0));
            T1DecArgs th = ta;
            th.nblks = (int)nheavy;
            th.masks = reinterpret_cast<unsigned long long *>(e->d_masks.as<uint8_t>() + state_bytes + planes_bytes);
            launch_t1_decode(th, s2);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipEventRecord(e->ev[EV_DONE], s2));
        }
#ifdef T1L_STATS
        static unsigned long long *dstats = nullptr;
        if (!dstats) HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&dstats), 128));
        HIP_CHECK(hipMemsetAsync(dstats, 0, 128, s));
        tl.stats = dstats;
#endif
        launch_t1_decode_lanes(tl, s);
        if (nheavy) HIP_CHECK(hipStreamWaitEvent(s, e->ev[EV_DONE], 0));
#ifdef T1L_STATS
        {
            unsigned long long h[16];
            HIP_CHECK(hipMemcpyAsync(h, dstats, 128, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
            std::fprintf(stderr, "t1 lanes: %zu blocks (+ %zu to the wave-per-block kernel) in %llu waves, %llu decisions (%.0f per block), %llu wave steps (%.0f per wave), %llu stripe-passes with work (%.0f per wave), "
                         "%.0f cycles per wave = %.0f per step\n", nb - nheavy, nheavy, h[3], h[0], (double)h[0] / std::max<size_t>(nb - nheavy, 1), h[1], (double)h[1] / std::max<unsigned long long>(h[3], 1),
                         h[2], (double)h[2] / std::max<unsigned long long>(h[3], 1), (double)h[4] / std::max<unsigned long long>(h[3], 1), (double)h[4] / std::max<unsigned long long>(h[1], 1));
            for (int k = 0; k < 3; ++k)
                std::fprintf(stderr, "   pass type %d (%s): %llu wave steps, %.0f cycles per step in the decision loop\n", k, k == 0 ? "significance" : k == 1 ? "refinement" : "cleanup",
                             h[5 + k], (double)h[8 + k] / std::max<unsigned long long>(h[5 + k], 1));
        }
#endif
    } else {
        e->d_masks.ensure(std::max<size_t>(mask_words, 64) * 8);
        ta.masks = e->d_masks.as<unsigned long long>();
        launch_t1_decode(ta, s);
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(e->ev[EV_T1], s));

    // ---- inverse DWT: resolution 1 .. R, every frame's tile-components as jobs of the same launches
    if (region) { // the windows of the tile-components the region meets, nothing else
        std::vector<IdwtWinJob> wjobs;
        std::vector<size_t> first_job(R + 2, 0);
        std::vector<int> mh(R + 1, 0), mv(R + 1, 0);
        for (uint32_t r = 1; r <= R; ++r) {
            first_job[r] = wjobs.size();
            for (uint32_t f = 0; f < nf; ++f)
                for (size_t t = 0; t < g.tiles.size(); ++t)
                    for (uint32_t c = 0; c < nd; ++c) {
                        const std::vector<ResFootprint> &fp = plans[0].windows[t * 4 + c];
                        if (fp.empty() || fp[r].win.empty()) continue;
                        const TileComp &TC = g.tiles[t].comps[c];
                        const Resolution &Rs = TC.res[r];
                        const long long off = (long long)(f * frame_words) + (long long)c * (long long)plane_elems +
                                              (long long)(ceildivpow2(TC.y0, (int)reduce) - S.poy[c]) * (long long)stride + (ceildivpow2(TC.x0, (int)reduce) - S.pox[c]);
                        const IdwtWinJob j = window_job(IRect{Rs.x0, Rs.y0, Rs.x1, Rs.y1}, fp[r], off);
                        int hi, vi;
                        idwt_window_items(j, hi, vi);
                        wjobs.push_back(j);
                        mh[r] = std::max(mh[r], hi); mv[r] = std::max(mv[r], vi);
                    }
        }
        first_job[R + 1] = wjobs.size();
        if (!wjobs.empty()) {
            e->jobs.ensure(wjobs.size() * sizeof(IdwtWinJob));
            HIP_CHECK(hipMemcpyAsync(e->jobs.p, wjobs.data(), wjobs.size() * sizeof(IdwtWinJob), hipMemcpyHostToDevice, s));
            HIP_CHECK(hipStreamSynchronize(s)); // `wjobs` is a pageable host vector
            for (uint32_t r = 1; r <= R; ++r) {
                IdwtWinArgs ia{};
                ia.a = e->Z.p; ia.tmp = e->Q.p; ia.stride = (long long)stride;
                ia.jobs = e->jobs.as<IdwtWinJob>() + first_job[r]; ia.njobs = (int)(first_job[r + 1] - first_job[r]);
                ia.max_h_items = mh[r]; ia.max_v_items = mv[r]; ia.reversible = cod.reversible;
                launch_idwt_window_level(ia, s);
                HIP_CHECK(hipGetLastError());
            }
        }
    }
    std::vector<IdwtJob> jobs;
    std::vector<size_t> job_first(R + 2, 0);
    std::vector<int> mrw(R + 1, 0), mrh(R + 1, 0);
    for (uint32_t r = 1; r <= R && !region; ++r) {
        job_first[r] = jobs.size();
        for (uint32_t f = 0; f < nf; ++f)
            for (const Tile &T : g.tiles)
                for (uint32_t c = 0; c < nd; ++c) {
                    const Resolution &Rs = T.comps[c].res[r];
                    IdwtJob j{};
                    j.rw = Rs.x1 - Rs.x0; j.rh = Rs.y1 - Rs.y0; j.casx = Rs.x0 & 1; j.casy = Rs.y0 & 1;
                    if (j.rw <= 0 || j.rh <= 0) continue;
                    j.off = (long long)(f * frame_words) + (long long)c * (long long)plane_elems +
                            (long long)(ceildivpow2(T.comps[c].y0, (int)reduce) - S.poy[c]) * (long long)stride + (ceildivpow2(T.comps[c].x0, (int)reduce) - S.pox[c]);
                    jobs.push_back(j);
                    mrw[r] = std::max(mrw[r], j.rw); mrh[r] = std::max(mrh[r], j.rh);
                }
    }
    job_first[R + 1] = jobs.size();
    if (!jobs.empty()) {
        e->jobs.ensure(jobs.size() * sizeof(IdwtJob));
        HIP_CHECK(hipMemcpyAsync(e->jobs.p, jobs.data(), jobs.size() * sizeof(IdwtJob), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipStreamSynchronize(s)); // `jobs` is a pageable host vector
        for (uint32_t r = 1; r <= R; ++r) {
            IdwtArgs ia{};
            ia.a = e->Z.p; ia.tmp = e->Q.p; ia.stride = (long long)stride;
            ia.jobs = e->jobs.as<IdwtJob>() + job_first[r]; ia.njobs = (int)(job_first[r + 1] - job_first[r]);
            ia.max_rw = mrw[r]; ia.max_rh = mrh[r]; ia.reversible = cod.reversible;
            launch_idwt_level(ia, s);
            HIP_CHECK(hipGetLastError());
        }
    }
    if (!fills.empty()) { // tiles that never arrived (above): whole or windowed, the planes' layout is the same
        launch_fill_rects(e->Z.p, (long long)stride, reinterpret_cast<const FillJob *>(e->d_dblk.as<uint8_t>() + fill_base), (int)fills.size(), fill_w, fill_h, s);
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipEventRecord(e->ev[EV_DWT], s));

    // ---- output stage: a frame's own launch, or the sequence kernels' one launch for the group
    if (call.seq) {
        const DecSeqFrameDev *dd = reinterpret_cast<const DecSeqFrameDev *>(e->d_dblk.as<uint8_t>() + desc_base);
        if (call.rgba) launch_decode_rgba_seq(ras[0], dd, (int)nf, s);
        else launch_decode_output_seq(oas[0], dd, (int)nf, s);
    } else if (call.rgba) launch_decode_rgba(ras[0], s);
    else launch_decode_output(oas[0], s);
    HIP_CHECK(hipGetLastError()); // a launch the runtime refused must not end as a frame of zeros
    HIP_CHECK(hipEventRecord(e->ev[EV_GATHER], s));
    if (!call.on_device) {
        bool staged = false;
        for (uint32_t f = 0; f < nf; ++f)
            download_spans(e, oas[f], call.planes + (size_t)(first + f) * nplanes, lay[f], e->d_outimg.as<uint8_t>() + lay[f].base, staged, s);
    }
    HIP_CHECK(hipStreamSynchronize(s));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, e->ev[EV_START], e->ev[EV_UPLOAD])); st.ms_upload += ms;
    HIP_CHECK(hipEventElapsedTime(&ms, e->ev[EV_UPLOAD], e->ev[EV_T1])); st.ms_t1 += ms;
    HIP_CHECK(hipEventElapsedTime(&ms, e->ev[EV_T1], e->ev[EV_DWT])); st.ms_dwt += ms;
    HIP_CHECK(hipEventElapsedTime(&ms, e->ev[EV_DWT], e->ev[EV_GATHER])); st.ms_frontend += ms;
    for (uint32_t f = 0; f < nf; ++f) st.codestream_bytes += lens[f];
    st.num_codeblocks += nb;
    e->dec_lane_blocks += nl * (lanes ? 1 : 0);
    e->dec_wave_blocks += nwave;
    for (const DecBlock &b : M.blocks) e->dec_passes += passes_of(b);
    e->dec_cw_bytes += cw_bytes;
}

// What a group of frames [a, b) needs on the device, from their plans: the waves of a lane launch and the bytes of its arenas
// (an estimate from above: the lane kernel's state and planes AND the wave kernel's masks, whichever is taken).
struct GroupNeed { size_t waves = 0, bytes = 0; };
GroupNeed frame_need(const DecodePlan &P, size_t file_len, size_t frame_words, size_t out_bytes)
{
    GroupNeed n;
    uint32_t most_passes = 1;
    size_t mask_words = 0;
    for (const DecBlock &b : P.blocks) {
        most_passes = std::max(most_passes, b.npasses);
        mask_words += (size_t)(b.numbps + 1) * 64;
    }
    n.waves = (P.blocks.size() + 63) / 64;
    n.bytes = round_up(file_len, 64) + P.arena_bytes + 2 * frame_words * sizeof(int32_t) + out_bytes + mask_words * 8 +
              n.waves * ((16 * 64 + 16 * 4) * 64 * sizeof(uint32_t) + (size_t)((most_passes + 1) / 3 + 1) * 16 * 8 * 64 * sizeof(uint32_t));
    return n;
}

void decode_frames(j2k_hip_encoder *e, const DecodeCall &call)
{
    const double t_begin = now_ms();
    const uint32_t n = call.nframes, nplanes = call.nplanes;
    auto fail = [&](uint32_t f, int code, const std::string &m) {
        if (call.seq) throw FrameError(code, f, m);
        throw Error(code, m);
    };
    if (e->pend.active) throw Error(J2K_HIP_ERR_PARAM, "an encode is in progress on this handle");
    if (!call.files || !n) fail(0, J2K_HIP_ERR_PARAM, "a sequence needs at least one frame");
    for (uint32_t f = 0; f < n; ++f)
        if (!call.files[f].data || !call.files[f].len) fail(f, J2K_HIP_ERR_PARAM, "Error reading file: empty input");
    if (!call.planes || nplanes < 1 || nplanes > 4) throw Error(J2K_HIP_ERR_PARAM, "1..4 destination channels");
    const uint32_t subsample = call.subsample ? call.subsample : 1;
    const j2k_hip_rect *const region = call.region;
    const uint32_t win[4] = {region ? region->x : 0, region ? region->y : 0, region ? region->w : 0, region ? region->h : 0};
    const uint32_t *const window = region ? win : nullptr;
    const uint32_t reduce = (uint32_t)floorlog2(subsample); // reference: params.cp_reduce = log2(subsample), :501
    HIP_CHECK(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    auto bytes_of = [&](uint32_t f) { return static_cast<const uint8_t *>(call.files[f].data); };
    const Decoding decoding(e->device); // (counted for the length of the call: the frames of a sequence are one decode in flight)

    // ---- every frame's headers are read first: a file this path cannot decode, or a frame that cannot share the launches of
    // frame 0, is turned away before the device is touched.
    Coding cod0;
    {
        FileHeader first_hdr;
        for (uint32_t f = 0; f < n; ++f) {
            FileHeader early;
            try {
                early = parse_headers(bytes_of(f), call.files[f].len);
                if (call.rgba) { // (a file the fused path does not take: J2K_HIP_ERR_UNSUPPORTED, nothing written)
                    const RgbaClass k = classify_rgba(early);
                    if (e->dec_xyz_to_rgb) check_xyz_to_rgb(early, k);
                }
            } catch (const Error &x) {
                if (call.seq) throw FrameError(x.code, f, x.what());
                throw;
            }
            if (f == 0) { cod0 = early.cod; if (n > 1) first_hdr = std::move(early); continue; }
            const std::string why = frames_differ(first_hdr, early, call.rgba != nullptr);
            if (!why.empty()) throw FrameError(J2K_HIP_ERR_PARAM, f, "differs from frame 0 in its " + why + ": the frames of a sequence call share their launches");
        }
    }
    // The destinations.  (One frame: after its plan, in the order of every decode before sequences.  A sequence: before any
    // device work, with what the frames' channels must share.)
    auto check_destinations = [&] {
        for (uint32_t f = 0; f < n; ++f)
            for (uint32_t c = 0; c < nplanes; ++c) {
                const j2k_hip_outplane &p = call.planes[(size_t)f * nplanes + c];
                try {
                    if (!p.base) throw Error(J2K_HIP_ERR_PARAM, "destination channel buffer is NULL");
                    check_outplane(p);
                } catch (const Error &x) {
                    if (call.seq) throw FrameError(x.code, f, x.what());
                    throw;
                }
                if (p.sample_bits != call.planes[c].sample_bits || p.depth != call.planes[c].depth)
                    throw FrameError(J2K_HIP_ERR_PARAM, f, "channel " + std::to_string(c) + " differs from frame 0's in sample_bits or depth");
            }
        for (uint32_t f = 1; f < n && call.rgba; ++f)
            if (!call.rgba[f].demote_ae16 != !call.rgba[0].demote_ae16) throw FrameError(J2K_HIP_ERR_PARAM, f, "demote_ae16 differs from frame 0's");
    };
    Shape S;
    if (call.seq) {
        try {
            if (reduce >= cod0.numres) throw Error(J2K_HIP_ERR_PARAM, "Error reading file: cannot discard " + std::to_string(reduce) + " of " + std::to_string(cod0.numres) + " resolutions");
            S = frame_shape(cod0, reduce);
            if (region && (!region->w || !region->h || (uint64_t)region->x + region->w > (uint64_t)S.ow || (uint64_t)region->y + region->h > (uint64_t)S.oh))
                throw Error(J2K_HIP_ERR_PARAM, "region (" + std::to_string(region->x) + ", " + std::to_string(region->y) + ", " + std::to_string(region->w) + " x " +
                                                   std::to_string(region->h) + ") is empty or leaves the image of " + std::to_string(S.ow) + " x " + std::to_string(S.oh));
        } catch (const Error &x) {
            throw FrameError(x.code, 0, x.what());
        }
        check_destinations();
    }

    // ---- host Tier-2.  One frame: beside the upload of the file (the device needs nothing of the plan to receive the bytes).
    // Several: on a few host threads, all frames before the first group is cut -- a frame whose packets turn out malformed
    // fails the call when its group is reached, the groups before it are complete by then.
    j2k_hip_stats st{};
    e->dec_lane_blocks = e->dec_wave_blocks = 0;
    e->dec_passes = e->dec_cw_bytes = 0;
    const uint32_t max_layers = e->dec_max_layers; // (read once: the planning threads share it)
    std::vector<DecodePlan> plans(n);
    std::vector<std::exception_ptr> plan_err(n);
    bool file_uploaded = false;
    if (n == 1) {
        const uint8_t *fbytes = bytes_of(0);
        const size_t len = call.files[0].len;
        HIP_CHECK(hipEventRecord(e->ev[EV_START], s));
        e->d_file.ensure(len + 64);
        file_uploaded = true;
        try {
            if (len >= (4u << 20)) {
                auto fut = std::async(std::launch::async, [&] { return plan_decode(fbytes, len, reduce, window, max_layers); });
                const hipError_t up = hipMemcpyAsync(e->d_file.p, fbytes, len, hipMemcpyHostToDevice, s);
                try {
                    plans[0] = fut.get();
                } catch (...) {
                    (void)hipStreamSynchronize(s); // the copy reads the caller's buffer: not past the end of this call
                    throw;
                }
                HIP_CHECK(up);
            } else {
                plans[0] = plan_decode(fbytes, len, reduce, window, max_layers);
                HIP_CHECK(hipMemcpyAsync(e->d_file.p, fbytes, len, hipMemcpyHostToDevice, s));
            }
        } catch (const Error &x) {
            if (call.seq && !dynamic_cast<const FrameError *>(&x)) throw FrameError(x.code, 0, x.what());
            throw;
        }
    } else {
        std::atomic<uint32_t> next{0};
        auto work = [&] {
            for (uint32_t f; (f = next.fetch_add(1)) < n;) {
                try { plans[f] = plan_decode(bytes_of(f), call.files[f].len, reduce, window, max_layers); }
                catch (...) { plan_err[f] = std::current_exception(); }
            }
        };
        const unsigned nt = std::min<unsigned>(plan_threads(), n);
        std::vector<std::thread> th;
        for (unsigned t = 1; t < nt; ++t) th.emplace_back(work);
        work();
        for (auto &t : th) t.join();
    }
    const double t_plan = now_ms();
    if (!call.seq) {
        S = frame_shape(plans[0].hdr.cod, reduce);
        check_destinations();
    }

    // ---- groups of consecutive frames.  A group's lane waves fit the waves the chip holds at once (so its lane launch still
    // lasts as long as its longest wave) and its arenas a share of the free device memory; decseq_group caps the frames.
    // One frame is always a group; a frame whose plan failed starts a group, so that every frame before it is delivered.
    size_t budget = ~(size_t)0;
    const size_t waves_max = (size_t)std::max(lane_waves_resident(), 1);
    if (n > 1) {
        size_t free_b = 0, total_b = 0;
        HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        const size_t held = e->d_file.cap + e->d_cw.cap + e->Z.cap + e->Q.cap + e->d_masks.cap + e->d_outimg.cap;
        budget = (size_t)(kSeqMemoryShare * (double)(free_b + held));
    }
    const int cap = tuning().decseq_group;
    for (uint32_t first = 0; first < n;) {
        auto rethrow = [&](uint32_t f) {
            try { std::rethrow_exception(plan_err[f]); }
            catch (const Error &x) { throw FrameError(x.code, f, x.what()); }
            catch (const std::bad_alloc &) { throw; }
            catch (const std::exception &x) { throw FrameError(J2K_HIP_ERR_PARAM, f, x.what()); }
        };
        if (plan_err[first]) rethrow(first);
        uint32_t nf = 1;
        if (n > 1) {
            auto out_bytes_of = [&](uint32_t f) {
                size_t b = 0;
                if (!call.on_device)
                    for (uint32_t c = 0; c < nplanes; ++c) {
                        const j2k_hip_outplane &p = call.planes[(size_t)f * nplanes + c];
                        b += (size_t)std::llabs((long long)p.rowbytes) * std::min<uint32_t>(p.height, (uint32_t)S.oh) + 512;
                    }
                return b;
            };
            GroupNeed need = frame_need(plans[first], call.files[first].len, S.frame_words(), out_bytes_of(first));
            for (; first + nf < n && !plan_err[first + nf] && (cap <= 0 || nf < (uint32_t)cap); ++nf) {
                const GroupNeed more = frame_need(plans[first + nf], call.files[first + nf].len, S.frame_words(), out_bytes_of(first + nf));
                if (cap <= 0 && (need.waves + more.waves > waves_max || need.bytes + more.bytes > budget)) break;
                if (cap > 0 && need.bytes + more.bytes > budget) break;
                need.waves += more.waves; need.bytes += more.bytes;
            }
        }
        try {
            decode_group(e, call, S, plans.data() + first, first, nf, decoding, file_uploaded, st);
        } catch (const Error &x) {
            if (call.seq && !dynamic_cast<const FrameError *>(&x)) throw FrameError(x.code, first, x.what());
            throw;
        }
        first += nf;
    }
    st.ms_t2_host = t_plan - t_begin;
    st.ms_total = now_ms() - t_begin;
    e->stats = st;
}

// The resolutions of one plane of width x height at origin (x0, y0) with `levels` decompositions, lowest first, and the
// footprints of `window` (plane coordinates) in them -- for the footprint query and the windowed transform's stage hook.
std::vector<ResFootprint> plane_footprints(bool reversible, uint32_t width, uint32_t height, uint32_t levels, uint32_t x0, uint32_t y0,
                                           const j2k_hip_rect *window, std::vector<IRect> &res)
{
    if (!width || !height || levels > 32 || (uint64_t)x0 + width > 0x7fffffffu || (uint64_t)y0 + height > 0x7fffffffu)
        throw Error(J2K_HIP_ERR_PARAM, "bad plane for a window: size 0, more than 32 levels or an origin beyond 2^31");
    if (!window || !window->w || !window->h || (uint64_t)window->x + window->w > width || (uint64_t)window->y + window->h > height)
        throw Error(J2K_HIP_ERR_PARAM, "window is empty or leaves the plane");
    res.assign(levels + 1, IRect{});
    for (uint32_t l = 0; l <= levels; ++l)
        res[levels - l] = IRect{ceildivpow2((int)x0, (int)l), ceildivpow2((int)y0, (int)l), ceildivpow2((int)(x0 + width), (int)l), ceildivpow2((int)(y0 + height), (int)l)};
    const IRect w{(int)(x0 + window->x), (int)(y0 + window->y), (int)(x0 + window->x + window->w), (int)(y0 + window->y + window->h)};
    return region_footprints(res.data(), levels + 1, reversible, w);
}

// One frame through decode_frames: the single-frame entry points.
void decode_impl(j2k_hip_encoder *e, const void *file, size_t len, uint32_t subsample, const j2k_hip_outplane *planes,
                 uint32_t nplanes, bool planes_on_device, const j2k_hip_rect *region = nullptr, const j2k_hip_rgba_dst *rgba = nullptr)
{
    const j2k_hip_file one{file, len};
    decode_frames(e, DecodeCall{&one, 1, subsample, region, planes, nplanes, rgba, planes_on_device, false});
}

// j2k_hip_decode_rgba[_device]: the destination is checked before anything else happens, then the decode above runs with
// R, G, B[, A] as its channels and the RGBA kernel as its last launch.
void decode_rgba_impl(j2k_hip_encoder *e, const void *file, size_t len, uint32_t subsample, const j2k_hip_rect *region,
                      const j2k_hip_rgba_dst *dst, bool on_device)
{
    if (!dst) throw Error(J2K_HIP_ERR_PARAM, "no RGBA destination");
    if (dst->struct_size != sizeof(j2k_hip_rgba_dst)) throw Error(J2K_HIP_ERR_PARAM, "j2k_hip_rgba_dst.struct_size mismatch (ABI drift)");
    if (!dst->r.base || !dst->g.base || !dst->b.base) throw Error(J2K_HIP_ERR_PARAM, "destination channel buffer is NULL");
    const bool alpha = dst->a.base != nullptr;
    check_rgba_dst(*dst, alpha);
    const j2k_hip_outplane planes[4] = {dst->r, dst->g, dst->b, dst->a};
    decode_impl(e, file, len, subsample, planes, alpha ? 4 : 3, on_device, region, dst);
}

// j2k_hip_decode_sequence[_device] and the RGBA forms: every refusal that needs no plan happens in decode_frames before any
// device work (the frames' destinations are checked here first, like the single-frame RGBA call does).
void decode_sequence_impl(j2k_hip_encoder *e, const j2k_hip_file *files, uint32_t nframes, uint32_t subsample, const j2k_hip_rect *region,
                          const j2k_hip_outplane *planes, uint32_t nplanes, bool on_device)
{
    decode_frames(e, DecodeCall{files, nframes, subsample, region, planes, nplanes, nullptr, on_device, true});
}
void decode_rgba_sequence_impl(j2k_hip_encoder *e, const j2k_hip_file *files, uint32_t nframes, uint32_t subsample, const j2k_hip_rect *region,
                               const j2k_hip_rgba_dst *dsts, bool on_device)
{
    if (!files || !nframes) throw FrameError(J2K_HIP_ERR_PARAM, 0, "a sequence needs at least one frame");
    if (!dsts) throw Error(J2K_HIP_ERR_PARAM, "no RGBA destination");
    const bool alpha = dsts[0].a.base != nullptr;
    std::vector<j2k_hip_outplane> planes((size_t)nframes * 4);
    for (uint32_t f = 0; f < nframes; ++f) {
        const j2k_hip_rgba_dst &d = dsts[f];
        try {
            if (d.struct_size != sizeof(j2k_hip_rgba_dst)) throw Error(J2K_HIP_ERR_PARAM, "j2k_hip_rgba_dst.struct_size mismatch (ABI drift)");
            if (!d.r.base || !d.g.base || !d.b.base) throw Error(J2K_HIP_ERR_PARAM, "destination channel buffer is NULL");
            if ((d.a.base != nullptr) != alpha) throw Error(J2K_HIP_ERR_PARAM, "an alpha destination in some frames only");
            check_rgba_dst(d, alpha);
        } catch (const Error &x) {
            throw FrameError(x.code, f, x.what());
        }
        const j2k_hip_outplane ch[4] = {d.r, d.g, d.b, d.a};
        for (int c = 0; c < (alpha ? 4 : 3); ++c) planes[(size_t)f * (alpha ? 4 : 3) + c] = ch[c];
    }
    decode_frames(e, DecodeCall{files, nframes, subsample, region, planes.data(), alpha ? 4u : 3u, dsts, on_device, true});
}

} // namespace

extern "C" {

int j2k_hip_rgba_mode(const void *file, size_t len, uint32_t *mode)
{
    if (!mode) return J2K_HIP_ERR_PARAM;
    try {
        *mode = classify_rgba(parse_headers(static_cast<const uint8_t *>(file), len)).mode;
        return J2K_HIP_OK;
    } catch (const Error &x) {
        create_error() = x.what();
        return x.code;
    } catch (const std::exception &x) {
        create_error() = x.what();
        return J2K_HIP_ERR_PARAM;
    }
}

int j2k_hip_decode_rgba(j2k_hip_encoder *e, const void *file, size_t len, uint32_t subsample, const j2k_hip_rect *region,
                        const j2k_hip_rgba_dst *dst)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    return guarded(e, [&] { decode_rgba_impl(e, file, len, subsample, region, dst, false); });
}

int j2k_hip_decode_rgba_device(j2k_hip_encoder *e, const void *file, size_t len, uint32_t subsample, const j2k_hip_rect *region,
                               const j2k_hip_rgba_dst *dst)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    return guarded(e, [&] { decode_rgba_impl(e, file, len, subsample, region, dst, true); });
}

int j2k_hip_read_info(const void *file, size_t len, j2k_hip_file_info *info)
{
    if (!info) return J2K_HIP_ERR_PARAM;
    try {
        if (info->struct_size != sizeof(j2k_hip_file_info)) throw Error(J2K_HIP_ERR_PARAM, "j2k_hip_file_info.struct_size mismatch (ABI drift)");
        const FileHeader H = parse_headers(static_cast<const uint8_t *>(file), len);
        const Coding &c = H.cod;
        j2k_hip_file_info o{};
        o.struct_size = sizeof(o);
        o.width = c.width; o.height = c.height; o.channels = c.ncomp_out(); o.depth = c.prec; // (reference :299: min(numcomps, 4))
        o.reversible = c.reversible; o.ycc = c.mct; o.layers = c.layers; o.num_resolutions = c.numres;
        o.tile_width = c.tile_w; o.tile_height = c.tile_h; o.progression = c.prog;
        o.file_format = H.jp2 ? J2K_HIP_FMT_JP2 : J2K_HIP_FMT_J2K;
        o.color_space = H.icc_len ? (uint32_t)J2K_HIP_CS_UNSPECIFIED : cs_from_enum(H.enumcs);
        o.icc_profile_offset = H.icc_off; o.icc_profile_len = H.icc_len;
        for (uint32_t k = 0; k < c.ncomp_out(); ++k) if (H.alpha_mask & (1u << k)) { o.alpha = k + 1; break; }
        o.alpha_premultiplied = H.alpha_premultiplied;
        for (uint32_t k = 0; k < c.ncomp && k < 4; ++k) { o.sub_x[k] = c.cdx[k]; o.sub_y[k] = c.cdy[k]; o.comp_depth[k] = c.cprec[k]; o.comp_signed[k] = c.csgnd[k]; }
        if (H.pal_entries) { // FileInfo.LUT / LUTmap (reference :362-401)
            o.lut_size = H.pal_entries; o.lut_channels = H.pal_columns;
            for (uint32_t i = 0; i < H.pal_entries && i < 256; ++i)
                for (uint32_t k = 0; k < H.pal_columns && k < 4; ++k) o.lut[i][k] = H.palette[(size_t)i * H.pal_columns + k];
            for (int k = 0; k < 4; ++k) o.lut_column[k] = H.pal_column_of[k];
        }
        *info = o;
        return J2K_HIP_OK;
    } catch (const Error &x) {
        create_error() = x.what();
        return x.code;
    } catch (const std::exception &x) {
        create_error() = x.what();
        return J2K_HIP_ERR_PARAM;
    }
}

int j2k_hip_decode(j2k_hip_encoder *e, const void *file, size_t len, uint32_t subsample, const j2k_hip_outplane *planes,
                   uint32_t nplanes)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    return guarded(e, [&] { decode_impl(e, file, len, subsample, planes, nplanes, false); });
}

int j2k_hip_decode_device(j2k_hip_encoder *e, const void *file, size_t len, uint32_t subsample, const j2k_hip_outplane *planes,
                          uint32_t nplanes)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    return guarded(e, [&] { decode_impl(e, file, len, subsample, planes, nplanes, true); });
}

int j2k_hip_decode_region(j2k_hip_encoder *e, const void *file, size_t len, uint32_t subsample, const j2k_hip_rect *region,
                          const j2k_hip_outplane *planes, uint32_t nplanes)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    return guarded(e, [&] { decode_impl(e, file, len, subsample, planes, nplanes, false, region); });
}

int j2k_hip_decode_region_device(j2k_hip_encoder *e, const void *file, size_t len, uint32_t subsample, const j2k_hip_rect *region,
                                 const j2k_hip_outplane *planes, uint32_t nplanes)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    return guarded(e, [&] { decode_impl(e, file, len, subsample, planes, nplanes, true, region); });
}

int j2k_hip_decode_sequence_check(const j2k_hip_file *files, uint32_t nframes, uint32_t *bad_frame)
{
    if (bad_frame) *bad_frame = 0;
    auto failed = [&](int code, uint32_t f, const std::string &text) {
        if (bad_frame) *bad_frame = f;
        create_error() = "frame " + std::to_string(f) + ": " + text;
        return code;
    };
    if (!files || !nframes) return failed(J2K_HIP_ERR_PARAM, 0, "a sequence needs at least one frame");
    FileHeader first;
    for (uint32_t f = 0; f < nframes; ++f) {
        try {
            if (!files[f].data || !files[f].len) throw Error(J2K_HIP_ERR_PARAM, "Error reading file: empty input");
            FileHeader H = parse_headers(static_cast<const uint8_t *>(files[f].data), files[f].len);
            if (f == 0) { first = std::move(H); continue; }
            const std::string why = frames_differ(first, H, false);
            if (!why.empty()) return failed(J2K_HIP_ERR_PARAM, f, "differs from frame 0 in its " + why + ": the frames of a sequence call share their launches");
        } catch (const Error &x) {
            return failed(x.code, f, x.what());
        } catch (const std::exception &x) {
            return failed(J2K_HIP_ERR_PARAM, f, x.what());
        }
    }
    return J2K_HIP_OK;
}

int j2k_hip_decode_sequence(j2k_hip_encoder *e, const j2k_hip_file *files, uint32_t nframes, uint32_t subsample, const j2k_hip_rect *region,
                            const j2k_hip_outplane *planes, uint32_t nplanes)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    return guarded(e, [&] { decode_sequence_impl(e, files, nframes, subsample, region, planes, nplanes, false); });
}

int j2k_hip_decode_sequence_device(j2k_hip_encoder *e, const j2k_hip_file *files, uint32_t nframes, uint32_t subsample,
                                   const j2k_hip_rect *region, const j2k_hip_outplane *planes, uint32_t nplanes)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    return guarded(e, [&] { decode_sequence_impl(e, files, nframes, subsample, region, planes, nplanes, true); });
}

int j2k_hip_decode_rgba_sequence(j2k_hip_encoder *e, const j2k_hip_file *files, uint32_t nframes, uint32_t subsample,
                                 const j2k_hip_rect *region, const j2k_hip_rgba_dst *dsts)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    return guarded(e, [&] { decode_rgba_sequence_impl(e, files, nframes, subsample, region, dsts, false); });
}

int j2k_hip_decode_rgba_sequence_device(j2k_hip_encoder *e, const j2k_hip_file *files, uint32_t nframes, uint32_t subsample,
                                        const j2k_hip_rect *region, const j2k_hip_rgba_dst *dsts)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    return guarded(e, [&] { decode_rgba_sequence_impl(e, files, nframes, subsample, region, dsts, true); });
}

int j2k_hip_debug_decode_kernels(const j2k_hip_encoder *e, uint64_t *lane_blocks, uint64_t *wave_blocks)
{
    if (!e || !lane_blocks || !wave_blocks) return J2K_HIP_ERR_PARAM;
    *lane_blocks = e->dec_lane_blocks; *wave_blocks = e->dec_wave_blocks;
    return J2K_HIP_OK;
}

int j2k_hip_debug_decode_work(const j2k_hip_encoder *e, uint64_t *passes, uint64_t *codeword_bytes)
{
    if (!e || !passes || !codeword_bytes) return J2K_HIP_ERR_PARAM;
    *passes = e->dec_passes; *codeword_bytes = e->dec_cw_bytes;
    return J2K_HIP_OK;
}

int j2k_hip_decode_set_max_layers(j2k_hip_encoder *e, uint32_t max_layers)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    return guarded(e, [&] { e->dec_max_layers = max_layers; });
}

int j2k_hip_decode_get_max_layers(const j2k_hip_encoder *e, uint32_t *max_layers)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    return guarded(const_cast<j2k_hip_encoder *>(e), [&] {
        if (!max_layers) throw Error(J2K_HIP_ERR_PARAM, "no place for the layer limit");
        *max_layers = e->dec_max_layers;
    });
}

int j2k_hip_decode_set_xyz_to_rgb(j2k_hip_encoder *e, uint32_t target)
{
    if (!e) {
        create_error() = "xyz_to_rgb: no handle";
        return J2K_HIP_ERR_PARAM;
    }
    const int rc = guarded(e, [&] {
        if (e->pend.active) throw Error(J2K_HIP_ERR_PARAM, "xyz_to_rgb: an encode is in progress on this handle");
        if (target > 3) throw Error(J2K_HIP_ERR_PARAM, "xyz_to_rgb must be 0..3 (off, sRGB, Rec.709 under a 2.4 power, Rec.709 linear)");
        e->dec_xyz_to_rgb = target;
    });
    if (rc != J2K_HIP_OK && refused_handle() == e) // (a pending j2k_hip_encode_begin_borrowed: refused before the handle is touched)
        refused_text() = "xyz_to_rgb: an encode is in progress on this handle (j2k_hip_encode_begin_borrowed without its _end)";
    return rc;
}

int j2k_hip_decode_get_xyz_to_rgb(const j2k_hip_encoder *e, uint32_t *target)
{
    if (!e) {
        create_error() = "xyz_to_rgb: no handle";
        return J2K_HIP_ERR_PARAM;
    }
    return guarded(const_cast<j2k_hip_encoder *>(e), [&] {
        if (!target) throw Error(J2K_HIP_ERR_PARAM, "no place for xyz_to_rgb");
        *target = e->dec_xyz_to_rgb;
    });
}

int j2k_hip_xyz_inverse_tables(uint32_t target, uint32_t comp_depth, uint32_t dst_depth, float *dl, float *othr, float matrix[9])
{
    try {
        if (!xyz_inverse_valid(target, comp_depth, dst_depth)) throw Error(J2K_HIP_ERR_PARAM, "xyz_to_rgb tables: target must be 1..3, the depths 1..16");
        if (dl) { const std::vector<float> t = xyz_delin_table(comp_depth); std::memcpy(dl, t.data(), t.size() * sizeof(float)); }
        if (othr) { const std::vector<float> t = xyz_othr_table(target, dst_depth); std::memcpy(othr, t.data(), t.size() * sizeof(float)); }
        if (matrix) xyz_inverse_matrix(matrix);
        return J2K_HIP_OK;
    } catch (const Error &x) {
        create_error() = x.what();
        return x.code;
    } catch (const std::exception &x) {
        create_error() = x.what();
        return J2K_HIP_ERR_PARAM;
    }
}

int j2k_hip_read_profile(const void *file, size_t len, uint32_t *rsiz)
{
    if (!rsiz) return J2K_HIP_ERR_PARAM;
    try {
        *rsiz = parse_headers(static_cast<const uint8_t *>(file), len).rsiz;
        return J2K_HIP_OK;
    } catch (const Error &x) {
        create_error() = x.what();
        return x.code;
    } catch (const std::exception &x) {
        create_error() = x.what();
        return J2K_HIP_ERR_PARAM;
    }
}

int j2k_hip_region_footprint(int reversible, uint32_t width, uint32_t height, uint32_t levels, uint32_t x0, uint32_t y0,
                             const j2k_hip_rect *window, j2k_hip_rect *rects, uint32_t nrects)
{
    try {
        if (!rects || levels > 32 || nrects < 3 * levels + 1) throw Error(J2K_HIP_ERR_PARAM, "3 * levels + 1 rectangles are needed");
        std::vector<IRect> res;
        const std::vector<ResFootprint> fp = plane_footprints(reversible != 0, width, height, levels, x0, y0, window, res);
        // a band's place in the Mallat layout: behind the lower resolution's columns / rows where it is the high band
        auto put = [&](uint32_t k, const IRect &need, int bx0, int by0, int offx, int offy) {
            j2k_hip_rect o{0, 0, 0, 0};
            if (!need.empty()) o = j2k_hip_rect{(uint32_t)(need.x0 - bx0 + offx), (uint32_t)(need.y0 - by0 + offy), (uint32_t)(need.x1 - need.x0), (uint32_t)(need.y1 - need.y0)};
            rects[k] = o;
        };
        put(0, fp[0].win, res[0].x0, res[0].y0, 0, 0);
        for (uint32_t r = 1; r <= levels; ++r) {
            const int lw = res[r - 1].x1 - res[r - 1].x0, lh = res[r - 1].y1 - res[r - 1].y0;
            const int hx0 = res[r].x0 >> 1, hy0 = res[r].y0 >> 1, lx0 = (res[r].x0 + 1) >> 1, ly0 = (res[r].y0 + 1) >> 1;
            put(3 * (r - 1) + 1, fp[r].band[0], hx0, ly0, lw, 0);
            put(3 * (r - 1) + 2, fp[r].band[1], lx0, hy0, 0, lh);
            put(3 * (r - 1) + 3, fp[r].band[2], hx0, hy0, lw, lh);
        }
        return J2K_HIP_OK;
    } catch (const Error &x) {
        create_error() = x.what();
        return x.code;
    } catch (const std::exception &x) {
        create_error() = x.what();
        return J2K_HIP_ERR_PARAM;
    }
}

// ---------------------------------------------------------------------------------------- decode stages (tests)
int j2k_hip_stage_idwt_window(j2k_hip_encoder *e, int reversible, uint32_t width, uint32_t height, uint32_t nplanes, uint32_t levels,
                              uint32_t x0, uint32_t y0, const j2k_hip_rect *window, const void *d_in, void *d_out)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    return guarded(e, [&] {
        if (e->pend.active) throw Error(J2K_HIP_ERR_PARAM, "an encode is in progress on this handle");
        HIP_CHECK(hipSetDevice(e->device));
        hipStream_t s = e->stream;
        if (!nplanes || !d_in || !d_out) throw Error(J2K_HIP_ERR_PARAM, "bad inverse DWT stage arguments");
        std::vector<IRect> res;
        const std::vector<ResFootprint> fp = plane_footprints(reversible != 0, width, height, levels, x0, y0, window, res);
        const size_t plane = (size_t)width * height, bytes = plane * nplanes * 4;
        e->Q.ensure(bytes);
        e->geo_valid = false; e->seq_valid = false; // the encode path's job table and planes are overwritten
        std::vector<IdwtWinJob> jobs;
        std::vector<size_t> first(levels + 2, 0);
        std::vector<int> mh(levels + 1, 0), mv(levels + 1, 0);
        for (uint32_t r = 1; r <= levels; ++r) {
            first[r] = jobs.size();
            if (fp[r].win.empty()) continue;
            for (uint32_t c = 0; c < nplanes; ++c) {
                const IdwtWinJob j = window_job(res[r], fp[r], (long long)(c * plane));
                idwt_window_items(j, mh[r], mv[r]);
                jobs.push_back(j);
            }
        }
        first[levels + 1] = jobs.size();
        HIP_CHECK(hipMemcpyAsync(d_out, d_in, bytes, hipMemcpyDeviceToDevice, s));
        if (!jobs.empty()) {
            e->jobs.ensure(jobs.size() * sizeof(IdwtWinJob));
            HIP_CHECK(hipMemcpyAsync(e->jobs.p, jobs.data(), jobs.size() * sizeof(IdwtWinJob), hipMemcpyHostToDevice, s));
            HIP_CHECK(hipStreamSynchronize(s)); // `jobs` is a pageable host vector
            for (uint32_t r = 1; r <= levels; ++r) { // lowest resolution first
                IdwtWinArgs ia{};
                ia.a = d_out; ia.tmp = e->Q.p; ia.stride = (long long)width;
                ia.jobs = e->jobs.as<IdwtWinJob>() + first[r]; ia.njobs = (int)(first[r + 1] - first[r]);
                ia.max_h_items = mh[r]; ia.max_v_items = mv[r]; ia.reversible = reversible;
                launch_idwt_window_level(ia, s);
                HIP_CHECK(hipGetLastError());
            }
        }
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

int j2k_hip_stage_idwt(j2k_hip_encoder *e, int reversible, uint32_t width, uint32_t height, uint32_t nplanes, uint32_t levels,
                       uint32_t x0, uint32_t y0, const j2k_hip_idwt_region *regions, uint32_t nregions, const void *d_in, void *d_out)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    return guarded(e, [&] {
        if (e->pend.active) throw Error(J2K_HIP_ERR_PARAM, "an encode is in progress on this handle");
        HIP_CHECK(hipSetDevice(e->device));
        hipStream_t s = e->stream;
        if (!width || !height || !nplanes || levels > 32 || !d_in || !d_out || (nregions && !regions)) throw Error(J2K_HIP_ERR_PARAM, "bad inverse DWT stage arguments");
        const j2k_hip_idwt_region whole{0, 0, width, height, x0, y0};
        const j2k_hip_idwt_region *rg = nregions ? regions : &whole;
        const uint32_t nr = nregions ? nregions : 1;
        for (uint32_t i = 0; i < nr; ++i) {
            if (!rg[i].w || !rg[i].h || (uint64_t)rg[i].x + rg[i].w > width || (uint64_t)rg[i].y + rg[i].h > height ||
                (uint64_t)rg[i].x0 + rg[i].w > 0x7fffffffu || (uint64_t)rg[i].y0 + rg[i].h > 0x7fffffffu)
                throw Error(J2K_HIP_ERR_PARAM, "inverse DWT region outside the plane");
            for (uint32_t j = 0; j < i; ++j)
                if (rg[i].x < rg[j].x + rg[j].w && rg[j].x < rg[i].x + rg[i].w && rg[i].y < rg[j].y + rg[j].h && rg[j].y < rg[i].y + rg[i].h)
                    throw Error(J2K_HIP_ERR_PARAM, "inverse DWT regions overlap");
        }
        const size_t plane = (size_t)width * height, bytes = plane * nplanes * 4;
        e->Q.ensure(bytes);
        e->geo_valid = false; e->seq_valid = false; // the encode path's job table and planes are overwritten
        // one job per plane, region and level, as a decode builds them per component, tile and resolution: level l of a region
        // = its resolution `levels - l` (both edges of the area scaled, then subtracted; the parities of the scaled origin)
        std::vector<IdwtJob> jobs;
        std::vector<size_t> first(levels + 1, 0);
        std::vector<int> mrw(levels, 0), mrh(levels, 0);
        for (uint32_t l = 0; l < levels; ++l) {
            first[l] = jobs.size();
            for (uint32_t c = 0; c < nplanes; ++c)
                for (uint32_t i = 0; i < nr; ++i) {
                    const int ax0 = ceildivpow2((int)rg[i].x0, (int)l), ax1 = ceildivpow2((int)(rg[i].x0 + rg[i].w), (int)l);
                    const int ay0 = ceildivpow2((int)rg[i].y0, (int)l), ay1 = ceildivpow2((int)(rg[i].y0 + rg[i].h), (int)l);
                    IdwtJob j{};
                    j.rw = ax1 - ax0; j.rh = ay1 - ay0; j.casx = ax0 & 1; j.casy = ay0 & 1;
                    if (j.rw <= 0 || j.rh <= 0) continue;
                    j.off = (long long)(c * plane) + (long long)rg[i].y * width + rg[i].x;
                    jobs.push_back(j);
                    mrw[l] = std::max(mrw[l], j.rw); mrh[l] = std::max(mrh[l], j.rh);
                }
        }
        first[levels] = jobs.size();
        HIP_CHECK(hipMemcpyAsync(d_out, d_in, bytes, hipMemcpyDeviceToDevice, s));
        if (!jobs.empty()) {
            e->jobs.ensure(jobs.size() * sizeof(IdwtJob));
            HIP_CHECK(hipMemcpyAsync(e->jobs.p, jobs.data(), jobs.size() * sizeof(IdwtJob), hipMemcpyHostToDevice, s));
            HIP_CHECK(hipStreamSynchronize(s)); // `jobs` is a pageable host vector
            for (uint32_t l = levels; l-- > 0;) { // lowest resolution first
                IdwtArgs ia{};
                ia.a = d_out; ia.tmp = e->Q.p; ia.stride = (long long)width;
                ia.jobs = e->jobs.as<IdwtJob>() + first[l]; ia.njobs = (int)(first[l + 1] - first[l]);
                ia.max_rw = mrw[l]; ia.max_rh = mrh[l]; ia.reversible = reversible;
                launch_idwt_level(ia, s);
                HIP_CHECK(hipGetLastError());
            }
        }
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

int j2k_hip_stage_decode_output(j2k_hip_encoder *e, int reversible, int mct, uint32_t width, uint32_t height, const void *d_comp,
                                size_t comp_words, uint32_t stride, const j2k_hip_outcomp *comps, uint32_t ncomp, void *d_buf,
                                size_t buf_bytes, const j2k_hip_outplane *planes, uint32_t nplanes)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    return guarded(e, [&] {
        if (e->pend.active) throw Error(J2K_HIP_ERR_PARAM, "an encode is in progress on this handle");
        HIP_CHECK(hipSetDevice(e->device));
        hipStream_t s = e->stream;
        if (!width || !height || width > (1u << 30) || height > (1u << 30) || !stride || !d_comp || !comps || !d_buf || !planes)
            throw Error(J2K_HIP_ERR_PARAM, "bad output stage arguments");
        for (uint32_t c = 0; c < nplanes && c < 4; ++c) check_outplane(planes[c]); // (a decode checks the channels beyond its components too)
        OutComp oc[4] = {};
        for (uint32_t c = 0; c < ncomp && c < 4; ++c)
            oc[c] = OutComp{static_cast<const uint32_t *>(d_comp) + comps[c].offset, comps[c].prec, comps[c].sub_x, comps[c].sub_y};
        DecOutArgs oa = decode_output_args(reversible != 0, mct != 0, (int)width, (int)height, (long long)stride, oc, ncomp, planes, nplanes);
        // every word the kernel reads lies in the component buffer ...
        for (uint32_t c = 0; c < ncomp; ++c) {
            const uint64_t cw = (width + comps[c].sub_x - 1) / comps[c].sub_x, ch = (height + comps[c].sub_y - 1) / comps[c].sub_y;
            if (cw > stride || comps[c].offset > comp_words || (ch - 1) * (uint64_t)stride + cw > comp_words - comps[c].offset)
                throw Error(J2K_HIP_ERR_PARAM, "component plane outside the buffer");
        }
        // ... and every sample it writes in the channel buffer, 16-bit ones at even addresses
        for (int c = 0; c < oa.nout; ++c) {
            if (oa.dst_w[c] <= 0 || oa.dst_h[c] <= 0) continue;
            const __int128 base = (__int128)reinterpret_cast<uintptr_t>(planes[c].base);
            const __int128 dx = (__int128)(oa.dst_w[c] - 1) * oa.colbytes[c], dy = (__int128)(oa.dst_h[c] - 1) * oa.rowbytes[c];
            const __int128 lo = base + std::min<__int128>(dx, 0) + std::min<__int128>(dy, 0);
            const __int128 hi = base + std::max<__int128>(dx, 0) + std::max<__int128>(dy, 0) + oa.dst_bytes[c];
            if (lo < 0 || hi > (__int128)buf_bytes) throw Error(J2K_HIP_ERR_PARAM, "destination channel outside the buffer");
            oa.dst[c] = static_cast<uint8_t *>(d_buf) + (size_t)base;
            if (oa.dst_bytes[c] == 2 && ((reinterpret_cast<uintptr_t>(oa.dst[c]) & 1) || (oa.dst_w[c] > 1 && (oa.colbytes[c] & 1)) || (oa.dst_h[c] > 1 && (oa.rowbytes[c] & 1))))
                throw Error(J2K_HIP_ERR_PARAM, "16-bit destination channel at an odd address");
        }
        launch_decode_output(oa, s);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

int j2k_hip_stage_rgba_output(j2k_hip_encoder *e, int reversible, int mct, uint32_t width, uint32_t height, const void *d_comp,
                              size_t comp_words, uint32_t stride, const j2k_hip_outcomp *comps, uint32_t ncomp, void *d_buf,
                              size_t buf_bytes, const j2k_hip_rgba_dst *dst, const j2k_hip_rgba_stage *stage)
{
    return j2k_hip_stage_rgba_output_xyz(e, reversible, mct, width, height, d_comp, comp_words, stride, comps, ncomp, d_buf, buf_bytes, dst, stage, 0);
}

int j2k_hip_stage_rgba_output_xyz(j2k_hip_encoder *e, int reversible, int mct, uint32_t width, uint32_t height, const void *d_comp,
                                  size_t comp_words, uint32_t stride, const j2k_hip_outcomp *comps, uint32_t ncomp, void *d_buf,
                                  size_t buf_bytes, const j2k_hip_rgba_dst *dst, const j2k_hip_rgba_stage *stage, uint32_t xyz_to_rgb)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    return guarded(e, [&] {
        if (e->pend.active) throw Error(J2K_HIP_ERR_PARAM, "an encode is in progress on this handle");
        HIP_CHECK(hipSetDevice(e->device));
        hipStream_t s = e->stream;
        if (!width || !height || width > (1u << 30) || height > (1u << 30) || !stride || !d_comp || !comps || !d_buf || !dst || !stage)
            throw Error(J2K_HIP_ERR_PARAM, "bad output stage arguments");
        if (stage->struct_size != sizeof(j2k_hip_rgba_stage)) throw Error(J2K_HIP_ERR_PARAM, "j2k_hip_rgba_stage.struct_size mismatch (ABI drift)");
        if (dst->struct_size != sizeof(j2k_hip_rgba_dst)) throw Error(J2K_HIP_ERR_PARAM, "j2k_hip_rgba_dst.struct_size mismatch (ABI drift)");
        if (stage->org_x > (1u << 30) || stage->org_y > (1u << 30)) throw Error(J2K_HIP_ERR_PARAM, "window origin beyond 2^30");
        const bool alpha = dst->a.sample_bits != 0; // (the bases are offsets here: 0 is one)
        check_rgba_dst(*dst, alpha);
        RgbaClass cls = rgba_class(stage->mode, ncomp);
        if (cls.mode == J2K_HIP_RGBA_PALETTE) {
            if (stage->lut_size > 256 || stage->lut_columns > 4) throw Error(J2K_HIP_ERR_PARAM, "palette beyond 256 entries of 4 columns");
            cls.lut_size = stage->lut_size;
            for (uint32_t i = 0; i < cls.lut_size; ++i)
                for (int j = 0; j < 3; ++j) {
                    if (stage->lut_rgb[j] >= stage->lut_columns) throw Error(J2K_HIP_ERR_PARAM, "palette column beyond the table");
                    cls.lut[i] |= (uint32_t)stage->lut[i][stage->lut_rgb[j]] << (8 * j);
                }
        }
        // every word the kernel reads lies in the component buffer ...
        RgbaComp rc[4] = {};
        for (int c = 0; c < cls.ncomp; ++c) {
            if (comps[c].sub_x < 1 || comps[c].sub_y < 1) throw Error(J2K_HIP_ERR_PARAM, "sub-sampling factor outside 1..255");
            const uint64_t cw = ((uint64_t)stage->org_x + width + comps[c].sub_x - 1) / comps[c].sub_x, ch = ((uint64_t)stage->org_y + height + comps[c].sub_y - 1) / comps[c].sub_y;
            if (cw > stride || comps[c].offset > comp_words || (ch - 1) * (uint64_t)stride + cw > comp_words - comps[c].offset)
                throw Error(J2K_HIP_ERR_PARAM, "component plane outside the buffer");
            rc[c] = RgbaComp{static_cast<const uint32_t *>(d_comp) + comps[c].offset, comps[c].prec, comps[c].sub_x, comps[c].sub_y};
        }
        // ... and every sample it writes in the channel buffer, 16-bit ones at even addresses
        j2k_hip_rgba_dst d = *dst;
        j2k_hip_outplane *const chn[4] = {&d.r, &d.g, &d.b, &d.a};
        for (int c = 0; c < (alpha ? 4 : 3); ++c) {
            j2k_hip_outplane &p = *chn[c];
            const int w = (int)std::min(p.width, width), h = (int)std::min(p.height, height), sb = (int)p.sample_bits / 8;
            const __int128 base = (__int128)reinterpret_cast<uintptr_t>(p.base);
            if (base > (__int128)buf_bytes) throw Error(J2K_HIP_ERR_PARAM, "destination channel outside the buffer");
            p.base = static_cast<uint8_t *>(d_buf) + (size_t)base;
            if (w <= 0 || h <= 0) continue;
            const __int128 dx = (__int128)(w - 1) * p.colbytes, dy = (__int128)(h - 1) * p.rowbytes;
            const __int128 lo = base + std::min<__int128>(dx, 0) + std::min<__int128>(dy, 0);
            const __int128 hi = base + std::max<__int128>(dx, 0) + std::max<__int128>(dy, 0) + sb;
            if (lo < 0 || hi > (__int128)buf_bytes) throw Error(J2K_HIP_ERR_PARAM, "destination channel outside the buffer");
            if (sb == 2 && ((reinterpret_cast<uintptr_t>(p.base) & 1) || (w > 1 && (p.colbytes & 1)) || (h > 1 && (p.rowbytes & 1))))
                throw Error(J2K_HIP_ERR_PARAM, "16-bit destination channel at an odd address");
        }
        DecRgbaArgs ra = decode_rgba_args(reversible != 0, mct != 0, (int)width, (int)height, (long long)stride, rc, cls, d, alpha,
                                          (int)stage->org_x, (int)stage->org_y, xyz_to_rgb);
        add_xyz_to_rgb(e, ra, s);
        launch_decode_rgba(ra, s);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

} // extern "C"

namespace {
// Both Tier-1 decode hooks.  cblk_style and the segment tables are the styled hook's (seg_first == nullptr: no block has
// segments of its own); segs = pairs (bytes, coding passes).
int stage_t1_decode_blocks(j2k_hip_encoder *e, int kernel, int reversible, void *d_coef, uint32_t stride, uint32_t nblocks,
                           const j2k_hip_dec_block *blocks, const void *cw, size_t cw_bytes, uint32_t cblk_style,
                           const uint32_t *seg_first, const uint32_t *seg_count, const uint32_t *segs, uint32_t nsegs_total)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    return guarded(e, [&] {
        if (e->pend.active) throw Error(J2K_HIP_ERR_PARAM, "an encode is in progress on this handle");
        HIP_CHECK(hipSetDevice(e->device));
        hipStream_t s = e->stream;
        if ((kernel != 0 && kernel != 1) || !d_coef || (nblocks && !blocks)) throw Error(J2K_HIP_ERR_PARAM, "bad Tier-1 decode stage arguments");
        const uint8_t *bytes = static_cast<const uint8_t *>(cw);
        {
            // blocks that share a sample would overwrite each other: sweep over the blocks sorted by their top row
            std::vector<uint32_t> order(nblocks);
            for (uint32_t i = 0; i < nblocks; ++i) {
                const j2k_hip_dec_block &b = blocks[i];
                if (b.w == 0 || b.h == 0 || b.w > 64 || b.h > 64 || b.orient > 3) throw Error(J2K_HIP_ERR_PARAM, "bad code-block rectangle");
                if ((uint64_t)b.x + b.w > stride) throw Error(J2K_HIP_ERR_PARAM, "code-block rectangle wider than the plane's stride");
                if (b.numbps > 30 || b.roishift > 30) throw Error(J2K_HIP_ERR_PARAM, "more bit-planes than a 32-bit sample holds");
                if (b.cw_len && (!bytes || b.cw_off > cw_bytes || b.cw_len > cw_bytes - b.cw_off)) throw Error(J2K_HIP_ERR_PARAM, "codeword bytes outside the buffer");
                if (seg_first) {
                    if (seg_first[i] > nsegs_total || seg_count[i] > nsegs_total - seg_first[i]) throw Error(J2K_HIP_ERR_PARAM, "codeword segments outside the table");
                    if (seg_count[i] > 0xffffu) throw Error(J2K_HIP_ERR_PARAM, "more codeword segments than a block can have");
                    for (uint32_t k = 0; k < seg_count[i]; ++k) {
                        const uint32_t *sg = segs + 2 * (size_t)(seg_first[i] + k);
                        if (sg[0] > kCwSegMaxBytes || sg[1] > kCwSegMaxPasses) throw Error(J2K_HIP_ERR_PARAM, "codeword segment of impossible length or pass count");
                    }
                }
                order[i] = i;
            }
            std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return blocks[a].y < blocks[b].y; });
            for (size_t i = 0; i < nblocks; ++i)
                for (size_t j = i + 1; j < nblocks && blocks[order[j]].y < blocks[order[i]].y + blocks[order[i]].h; ++j) {
                    const j2k_hip_dec_block &a = blocks[order[i]], &b = blocks[order[j]];
                    if (a.x < b.x + b.w && b.x < a.x + a.w) throw Error(J2K_HIP_ERR_PARAM, "code-block rectangles overlap");
                }
        }
        // the kernels' table: the blocks that hold something, in the order given (t1dec_passes: the plan's rule and the clamp)
        std::vector<DecBlkDev> tab;
        std::vector<uint64_t> src;
        std::vector<uint32_t> cwsegs;
        const bool multiseg = (cblk_style & 5u) != 0;
        uint64_t arena = 0;
        size_t mask_words = 0;
        for (uint32_t i = 0; i < nblocks; ++i) {
            const j2k_hip_dec_block &b = blocks[i];
            const uint32_t np = t1dec_passes(b.numbps, b.npasses);
            if (!np) continue;
            DecBlkDev d{};
            d.cw_off = arena; d.cw_len = b.cw_len;
            d.mask_off = mask_words;
            d.coef_off = (unsigned long long)b.y * stride + b.x;
            d.stepsize = b.half_step;
            d.w = (unsigned short)b.w; d.h = (unsigned short)b.h; d.npasses = (unsigned short)np;
            d.orient = (unsigned char)b.orient; d.numbps = (unsigned char)b.numbps; d.roishift = (unsigned char)b.roishift;
            if (multiseg) { // the words of a file decode's plan: a segment ends where the block's bytes end
                if (!seg_first || !seg_count[i]) throw Error(J2K_HIP_ERR_PARAM, "a block with passes needs a codeword segment under bypass or termall");
                d.seg_off = (unsigned)cwsegs.size(); d.nsegs = (unsigned short)seg_count[i];
                uint64_t at = 0;
                for (uint32_t k = 0; k < seg_count[i]; ++k) {
                    const uint32_t *sg = segs + 2 * (size_t)(seg_first[i] + k);
                    cwsegs.push_back(cwseg_word(cwseg_have(sg[0], at, b.cw_len), sg[1]));
                    at += sg[0];
                }
            }
            tab.push_back(d);
            src.push_back(b.cw_off);
            arena = cw_arena_next(arena + b.cw_len);
            mask_words += (size_t)(b.numbps + 1) * 64;
        }
        const size_t nb = tab.size();
        if (!nb) return;
        const size_t arena_bytes = (size_t)cw_arena_bytes(arena) + kCwArenaTail;
        std::vector<DecGroupDev> groups(kernel == 1 ? (nb + 63) / 64 : 0);
        const size_t plane_words = lane_groups(tab.data(), nb, groups);
        // one pinned buffer: block table | groups | codeword arena.  A decode leaves the arena's slack and tail as they were; here
        // they are zeros, so that a kernel which took a byte from past a block's end (where the decoder is fed 1-bits) shows.
        const size_t grp_base = round_up(nb * sizeof(DecBlkDev), 16);
        const size_t cwseg_base = grp_base + round_up(groups.size() * sizeof(DecGroupDev), 16);
        const size_t tab_bytes = cwseg_base + round_up(cwsegs.size() * sizeof(uint32_t), 16) + 64;
        const size_t cw_base = round_up(tab_bytes, 16);
        e->h_dtab.ensure(cw_base + arena_bytes);
        uint8_t *ht = e->h_dtab.as<uint8_t>();
        std::memset(ht, 0, cw_base + arena_bytes);
        std::memcpy(ht, tab.data(), nb * sizeof(DecBlkDev));
        if (!groups.empty()) std::memcpy(ht + grp_base, groups.data(), groups.size() * sizeof(DecGroupDev));
        if (!cwsegs.empty()) std::memcpy(ht + cwseg_base, cwsegs.data(), cwsegs.size() * sizeof(uint32_t));
        for (size_t k = 0; k < nb; ++k)
            if (tab[k].cw_len) std::memcpy(ht + cw_base + tab[k].cw_off, bytes + src[k], tab[k].cw_len);
        e->d_dblk.ensure(tab_bytes);
        e->d_cw.ensure(arena_bytes);
        e->geo_valid = false; e->seq_valid = false;
        HIP_CHECK(hipMemcpyAsync(e->d_dblk.p, ht, tab_bytes, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(e->d_cw.p, ht + cw_base, arena_bytes, hipMemcpyHostToDevice, s));
        T1DecArgs ta{};
        ta.cw = e->d_cw.as<uint8_t>();
        ta.coef = d_coef; ta.stride = (long long)stride;
        ta.blks = e->d_dblk.as<DecBlkDev>(); ta.nblks = (int)nb; ta.reversible = reversible;
        ta.cwsegs = reinterpret_cast<const unsigned *>(e->d_dblk.as<uint8_t>() + cwseg_base); // (style 0: no block has segments of its own)
        ta.style = cblk_style;
        if (kernel == 1) {
            const size_t state_bytes = lane_state_bytes(groups.size()), planes_bytes = lane_planes_bytes(plane_words);
            e->d_masks.ensure(state_bytes + planes_bytes);
            HIP_CHECK(hipMemsetAsync(e->d_masks.p, 0, state_bytes, s));
            ta.state = e->d_masks.as<unsigned>();
            ta.planes = ta.state + state_bytes / sizeof(uint32_t);
            ta.groups = reinterpret_cast<const DecGroupDev *>(e->d_dblk.as<uint8_t>() + grp_base);
            launch_t1_decode_lanes(ta, s);
        } else {
            e->d_masks.ensure(std::max<size_t>(mask_words, 64) * 8);
            ta.masks = e->d_masks.as<unsigned long long>();
            launch_t1_decode(ta, s);
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(s));
    });
}
} // namespace

extern "C" {

int j2k_hip_stage_t1_decode(j2k_hip_encoder *e, int kernel, int reversible, void *d_coef, uint32_t stride, uint32_t nblocks,
                            const j2k_hip_dec_block *blocks, const void *cw, size_t cw_bytes)
{
    return stage_t1_decode_blocks(e, kernel, reversible, d_coef, stride, nblocks, blocks, cw, cw_bytes, 0, nullptr, nullptr, nullptr, 0);
}

int j2k_hip_stage_t1_decode_styled(j2k_hip_encoder *e, int reversible, void *d_coef, uint32_t stride, uint32_t nblocks,
                                   const j2k_hip_dec_block *blocks, const void *cw, size_t cw_bytes, uint32_t cblk_style,
                                   const uint32_t *seg_first, const uint32_t *seg_count, const uint32_t *segs, uint32_t nsegs_total)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    const bool multiseg = (cblk_style & 5u) != 0;
    bool bad = cblk_style > 63u || (nsegs_total && !segs) || (nblocks && multiseg && (!seg_first || !seg_count));
    if (!bad && !multiseg) { // one segment per block: a table has no meaning
        bad = nsegs_total != 0;
        for (uint32_t i = 0; !bad && seg_count && blocks && i < nblocks; ++i) bad = seg_count[i] != 0;
    }
    if (bad) return guarded(e, [&] { throw Error(J2K_HIP_ERR_PARAM, "bad code-block style or codeword segment table"); });
    return stage_t1_decode_blocks(e, 1, reversible, d_coef, stride, nblocks, blocks, cw, cw_bytes, cblk_style, multiseg ? seg_first : nullptr,
                                  seg_count, segs, nsegs_total);
}

} // extern "C"
