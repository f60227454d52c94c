// stage_hooks.cpp -- the stage hooks of the encode path (include/j2k_hip.h: j2k_hip_stage_*): single kernels, or a few of them,
// driven on buffers the caller supplies, for the tests that pin the kernels down in isolation.  They run on a handle's stream and
// arenas and through what an encode runs them with (handle.h, table_layout.h, rate_device.h): a table layout has one definition.
// Every hook that overwrites an arena of the handle leaves the tables an encode caches to be rebuilt (invalidate_cached_tables).
// The decode path's hooks are in decoder.cpp.
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "cblk_style.h"
#include "handle.h"
#include "rate_device.h"
#include "tier2.h"

using namespace j2k_hip;

// What j2k_hip_stage_t1_slots adds to the Tier-1 stage hooks: the caller's capacities, guard stripes between the slots, the
// error word instead of a failure, and both arenas whole.
struct T1Slots {
    const uint32_t *sym_cap, *out_cap;
    uint32_t guard_bytes;
    uint32_t *err, *nsym;
    void *sym_arena; size_t sym_arena_cap;
    void *out_arena; size_t out_arena_cap;
};
constexpr int kSlotFill = 0xA5; // what an arena of j2k_hip_stage_t1_slots holds wherever no kernel wrote (J2K_HIP_SLOT_FILL)
static_assert(kSlotFill == J2K_HIP_SLOT_FILL, "the header names the fill");

// the Tier-1 stage hooks are one function: pass_rate / pass_dist on request, a code-block style or none, and the slots by the
// frame's rule (at Mb = 30, back to back) or as the caller lays them out (slots)
static int stage_t1_blocks(j2k_hip_encoder *e, int reversible, void *d_coef, uint32_t stride, uint32_t nblocks,
                           const uint32_t *bx, const uint32_t *by, const uint32_t *bw, const uint32_t *bh, const uint32_t *orient,
                           const float *stepsize, uint32_t *numbps, uint32_t *npasses, uint32_t *length, uint64_t *offsets,
                           void *data, size_t data_cap, uint32_t *pass_rate, int32_t *pass_dist, uint32_t cblk_style,
                           const T1Slots *slots = nullptr)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    return guarded(e, [&] {
        // (the coder streams of a pending frame still read blks / sym / out / meta: nothing of the handle is touched)
        if (e->pend.active) throw Error(J2K_HIP_ERR_PARAM, "the previous j2k_hip_encode_begin on this handle has not been finished");
        // the styles a frame refuses (geometry.cpp)
        if (cblk_style & kStyleVcausal) throw Error(J2K_HIP_ERR_PARAM, "cblk_style: vertically causal contexts (bit 8) are not written");
        if (cblk_style & ~(uint32_t)(kStylesEncoded | kStyleVcausal)) throw Error(J2K_HIP_ERR_PARAM, "cblk_style: unknown code-block style bits");
        if (slots) {
            if (!slots->sym_cap || !slots->out_cap || !slots->err || !slots->nsym || !slots->sym_arena || !slots->out_arena || !numbps || !npasses || !length)
                throw Error(J2K_HIP_ERR_PARAM, "Tier-1 slots: an array is NULL");
            if (slots->guard_bytes % 16) throw Error(J2K_HIP_ERR_PARAM, "Tier-1 slots: guard_bytes must be a multiple of 16");
        }
        HIP_CHECK(hipSetDevice(e->device));
        hipStream_t s = e->stream;
        const size_t guard = slots ? slots->guard_bytes : 0;
        const size_t nb = nblocks;
        std::vector<CblkDev> blks(nb);
        size_t sym_off = guard, out_off = guard; // (a guard stripe in front of every slot and behind the last)
        for (size_t i = 0; i < nb; ++i) {
            if (bw[i] == 0 || bh[i] == 0 || bw[i] > 64 || bh[i] > 64 || orient[i] > 3) throw Error(J2K_HIP_ERR_PARAM, "bad code-block rectangle");
            CblkDev d{};
            d.coef_off = (unsigned long long)by[i] * stride + bx[i];
            const size_t area = (size_t)bw[i] * bh[i];
            const CblkCaps caps = cblk_capacities(area, 30, cblk_style); // (Mb = 30: no band is known here; a frame's are smaller)
            size_t symcap = caps.sym, outcap = caps.out;
            if (slots) {
                symcap = slots->sym_cap[i]; outcap = slots->out_cap[i];
                if (symcap % 16 || outcap % 16 || symcap < 16 || outcap < 16 || symcap > caps.sym || outcap > caps.out)
                    throw Error(J2K_HIP_ERR_PARAM, "Tier-1 slots: a capacity must be a multiple of 16, at least 16 and at most the rule's at Mb = 30");
            }
            d.sym_off = sym_off; d.sym_cap = (unsigned)symcap; d.out_off = out_off; d.out_cap = (unsigned)outcap;
            d.stepsize = stepsize ? stepsize[i] : 1.0f;
            d.w = (unsigned short)bw[i]; d.h = (unsigned short)bh[i]; d.orient = (unsigned char)orient[i]; d.Mb = 30;
            sym_off += symcap + guard; out_off += outcap + guard;
            blks[i] = d;
        }
        if (slots && (sym_off > slots->sym_arena_cap || out_off > slots->out_arena_cap)) throw Error(J2K_HIP_ERR_OVERFLOW, "Tier-1 slots: an arena buffer is too small");
        {
            // The modeller rewrites every block of d_coef in place (scaled magnitudes, transposed bit-planes): two blocks that
            // share a sample would read each other's scratch.  Sweep over the blocks sorted by their top row.
            std::vector<uint32_t> order(nb);
            for (uint32_t i = 0; i < nb; ++i) order[i] = i;
            std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return by[a] < by[b]; });
            for (size_t i = 0; i < nb; ++i)
                for (size_t j = i + 1; j < nb && by[order[j]] < by[order[i]] + bh[order[i]]; ++j) {
                    const uint32_t a = order[i], b = order[j];
                    if (bx[a] < bx[b] + bw[b] && bx[b] < bx[a] + bw[a]) throw Error(J2K_HIP_ERR_PARAM, "code-block rectangles overlap");
                }
            for (size_t i = 0; i < nb; ++i)
                if ((uint64_t)bx[i] + bw[i] > stride) throw Error(J2K_HIP_ERR_PARAM, "code-block rectangle wider than the plane's stride");
        }
        invalidate_cached_tables(e); // the block table and the Tier-1 results of the handle's last frame are overwritten
        const T1Tables tt(nb);
        e->blks.ensure(std::max<size_t>(1, nb) * sizeof(CblkDev));
        if (nb) HIP_CHECK(hipMemcpyAsync(e->blks.p, blks.data(), nb * sizeof(CblkDev), hipMemcpyHostToDevice, s));
        e->sym.ensure(sym_off + 1024); e->out.ensure(out_off + 64);
        e->meta.ensure(tt.meta_bytes());
        e->passes.ensure(tt.passes_bytes());
        T1Args ta{};
        ta.coef = d_coef; ta.stride = stride; ta.blks = e->blks.as<CblkDev>(); ta.nblks = (int)nb; ta.reversible = reversible;
        t1_arena_args(e, tt, ta);
        ta.want_dist = pass_dist != nullptr; // the distortion sums cost LDS and issue slots: only on request
        ta.want_rates = pass_rate || pass_dist; // the coder's per-pass byte counts: whenever the pass tables are read back
        ta.sparse = tuning().t1_sparse;
        ta.mq_window = tuning().mq_window;
        ta.style = cblk_style;
#ifdef J2K_T1_COUNTERS
        t1_counters(ta);
#endif
        HIP_CHECK(hipMemsetAsync(ta.err, 0, sizeof(uint32_t), s));
        if (slots) { // guards and slots alike: a byte that no kernel wrote comes back as the fill
            HIP_CHECK(hipMemsetAsync(e->sym.p, kSlotFill, sym_off, s));
            HIP_CHECK(hipMemsetAsync(e->out.p, kSlotFill, out_off, s));
        }
        launch_t1_model(ta, s);
        launch_t1_mq(ta, s);
        if (cblk_style) launch_t1_rate_fixup(ta, s); // as a styled frame has them: on the device, behind the styled coder
        std::vector<uint32_t> hm(tt.meta_words());
        HIP_CHECK(hipMemcpyAsync(hm.data(), e->meta.p, hm.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        if (slots) {
            HIP_CHECK(hipMemcpyAsync(slots->sym_arena, e->sym.p, sym_off, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipMemcpyAsync(slots->out_arena, e->out.p, out_off, hipMemcpyDeviceToHost, s));
        }
        HIP_CHECK(hipStreamSynchronize(s));
        if (slots) *slots->err = *tt.err(hm.data()); // (the caller's to judge: a block that does not fit is what this hook is for)
        else if (*tt.err(hm.data())) throw Error(J2K_HIP_ERR_OVERFLOW, "Tier-1 kernel reported error " + std::to_string(*tt.err(hm.data())));
        size_t pos = 0;
        for (size_t i = 0; i < nb; ++i) {
            numbps[i] = tt.numbps(hm.data())[i]; npasses[i] = tt.npasses(hm.data())[i]; length[i] = tt.len(hm.data())[i];
            if (slots) { slots->nsym[i] = tt.nsym(hm.data())[i]; continue; } // (the codewords are in the arena)
            offsets[i] = pos;
            if (pos + length[i] > data_cap) throw Error(J2K_HIP_ERR_OVERFLOW, "data buffer too small");
            if (length[i]) HIP_CHECK(hipMemcpy(static_cast<uint8_t *>(data) + pos, e->out.as<uint8_t>() + blks[i].out_off, length[i], hipMemcpyDeviceToHost));
            pos += length[i];
        }
        if (pass_rate || pass_dist) {
            std::vector<uint32_t> hp(tt.passes_words());
            HIP_CHECK(hipMemcpy(hp.data(), e->passes.p, hp.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < nb; ++i) {
                const uint32_t np = npasses[i];
                uint32_t *rate = tt.pass_rate(hp.data()) + tt.row(i);
                const uint32_t *nmsedec = tt.pass_nmsedec(hp.data()) + tt.row(i);
                if (!cblk_style && !(slots && length[i] > blks[i].out_cap)) { // (a codeword that did not fit has no bytes to look at)
                    // the reference's fix-ups of the per-pass byte counts: an estimate never exceeds what
                    // follows it, and a pass never ends on 0xFF  (under a style the kernel above has applied them)
                    uint32_t last = length[i];
                    for (uint32_t p = np; p > 0;) { --p; if (rate[p] > last) rate[p] = last; else last = rate[p]; }
                    const uint8_t *bytes = slots ? static_cast<const uint8_t *>(slots->out_arena) + blks[i].out_off : static_cast<const uint8_t *>(data) + offsets[i];
                    for (uint32_t p = 0; p < np; ++p)
                        if (rate[p] > 0 && bytes[rate[p] - 1] == 0xff) --rate[p];
                }
                for (uint32_t p = 0; p < (uint32_t)kDevMaxPasses; ++p) {
                    if (pass_rate) pass_rate[tt.row(i) + p] = p < np ? rate[p] : 0;
                    if (pass_dist) pass_dist[tt.row(i) + p] = p < np ? (int32_t)nmsedec[p] : 0;
                }
            }
        }
    });
}

extern "C" {

int j2k_hip_stage_frontend(j2k_hip_encoder *e, const j2k_hip_params *params, const j2k_hip_plane *planes_device, void *d_out)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    return guarded(e, [&] {
        if (e->pend.active) throw Error(J2K_HIP_ERR_PARAM, "the previous j2k_hip_encode_begin on this handle has not been finished");
        HIP_CHECK(hipSetDevice(e->device));
        const Coding cod = normalise(params);
        FrontendArgs fa = make_frontend_args(cod, planes_device, 0, 0, (int)cod.width, (int)cod.height);
        if (cod.subsampled() || cod.rgb_to_sycc || cod.rgb_to_xyz) {
            // components of their own sizes, and X'Y'Z' (run_frontend holds its tables): into planes of a common, aligned row stride as an encode has them, then dense to d_out
            const PlaneLayout lay = plane_layout(cod, 0, 0, (int)cod.width, (int)cod.height);
            e->P.ensure(lay.frame_elems * sizeof(int32_t));
            run_frontend(e, cod, fa, e->P.as<int32_t>(), lay.comp_off, lay.stride, e->stream);
            HIP_CHECK(hipGetLastError());
            uint8_t *out = static_cast<uint8_t *>(d_out);
            for (uint32_t c = 0; c < cod.ncomp; ++c) {
                const size_t cw = (size_t)lay.cw[c], chh = (size_t)lay.ch[c];
                HIP_CHECK(hipMemcpy2DAsync(out, cw * 4, e->P.as<int32_t>() + lay.comp_off[c], lay.stride * 4, cw * 4, chh, hipMemcpyDeviceToDevice, e->stream));
                out += cw * chh * 4;
            }
            HIP_CHECK(hipStreamSynchronize(e->stream));
            return;
        }
        for (uint32_t c = 0; c < cod.ncomp; ++c) fa.dst[c] = static_cast<int32_t *>(d_out) + (size_t)c * cod.width * cod.height;
        fa.dst_stride = cod.width;
        launch_frontend(fa, e->stream);
        HIP_CHECK(hipStreamSynchronize(e->stream));
    });
}

int j2k_hip_stage_dwt(j2k_hip_encoder *e, int reversible, uint32_t width, uint32_t height, uint32_t nplanes, uint32_t levels,
                      uint32_t x0, uint32_t y0, const void *d_in, void *d_out, uint32_t repeat, double *ms_out)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    return guarded(e, [&] {
        if (e->pend.active) throw Error(J2K_HIP_ERR_PARAM, "the previous j2k_hip_encode_begin on this handle has not been finished");
        HIP_CHECK(hipSetDevice(e->device));
        if (!width || !height || !nplanes || levels > 32) throw Error(J2K_HIP_ERR_PARAM, "bad DWT stage arguments");
        const size_t plane = (size_t)width * height;
        e->P.ensure(plane * nplanes * 4);
        e->Q.ensure(plane * nplanes * 4);
        std::vector<std::vector<DwtJob>> jobs(levels);
        std::vector<int> mrw(levels, 0), mrh(levels, 0);
        size_t total = 0;
        for (uint32_t l = 0; l < levels; ++l)
            for (uint32_t c = 0; c < nplanes; ++c) {
                DwtJob j{};
                const int ax0 = ceildivpow2((int)x0, (int)l), ax1 = ceildivpow2((int)(x0 + width), (int)l);
                const int ay0 = ceildivpow2((int)y0, (int)l), ay1 = ceildivpow2((int)(y0 + height), (int)l);
                j.rw = ax1 - ax0; j.rh = ay1 - ay0; j.casx = ax0 & 1; j.casy = ay0 & 1;
                j.src_off = j.ll_off = j.z_off = (long long)(c * plane);
                if (j.rw <= 0 || j.rh <= 0) continue;
                jobs[l].push_back(j); mrw[l] = std::max(mrw[l], j.rw); mrh[l] = std::max(mrh[l], j.rh);
                ++total;
            }
        e->jobs.ensure(std::max<size_t>(1, total) * sizeof(DwtJob));
        size_t pos = 0;
        for (auto &v : jobs) {
            if (!v.empty()) HIP_CHECK(hipMemcpyAsync(e->jobs.as<DwtJob>() + pos, v.data(), v.size() * sizeof(DwtJob), hipMemcpyHostToDevice, e->stream));
            pos += v.size();
        }
        invalidate_cached_tables(e); // the job table was overwritten
        if (levels == 0) HIP_CHECK(hipMemcpyAsync(d_out, d_in, plane * nplanes * 4, hipMemcpyDeviceToDevice, e->stream));
        if (repeat == 0) repeat = 1;
        HIP_CHECK(hipEventRecord(e->ev[EV_START], e->stream));
        for (uint32_t r = 0; r < repeat; ++r) {
            pos = 0;
            for (uint32_t l = 0; l < levels; ++l) {
                DwtLevelArgs da{};
                da.src = l == 0 ? d_in : ((l & 1) ? e->Q.p : e->P.p); da.src_stride = width;
                const bool last = l == levels - 1;
                da.ll = last ? d_out : ((l & 1) ? e->P.p : e->Q.p); da.ll_stride = width;
                da.z = d_out; da.z_stride = width;
                da.jobs = e->jobs.as<DwtJob>() + pos; da.njobs = (int)jobs[l].size();
                da.max_rw = mrw[l]; da.max_rh = mrh[l]; da.reversible = reversible;
                launch_dwt_level(da, e->stream);
                pos += jobs[l].size();
            }
        }
        HIP_CHECK(hipEventRecord(e->ev[EV_DONE], e->stream));
        HIP_CHECK(hipStreamSynchronize(e->stream));
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, e->ev[EV_START], e->ev[EV_DONE]));
        if (ms_out) *ms_out = ms / repeat;
    });
}

// j2k_hip_stage_dwt with jobs of different sizes, origins and offsets in one launch per level: every (plane, region) is a
// DwtJob of its own, as every tile-component of a frame is (the mirror of the region form of j2k_hip_stage_idwt).
int j2k_hip_stage_dwt_regions(j2k_hip_encoder *e, int reversible, uint32_t width, uint32_t height, uint32_t nplanes, uint32_t levels,
                              const j2k_hip_idwt_region *regions, uint32_t nregions, const void *d_in, void *d_out)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    return guarded(e, [&] {
        if (e->pend.active) throw Error(J2K_HIP_ERR_PARAM, "the previous j2k_hip_encode_begin on this handle has not been finished");
        if (!width || !height || !nplanes || levels > 32 || !d_in || !d_out || !regions || !nregions)
            throw Error(J2K_HIP_ERR_PARAM, "bad DWT region stage arguments");
        const j2k_hip_idwt_region *rg = regions;
        for (uint32_t i = 0; i < nregions; ++i) {
            if (!rg[i].w || !rg[i].h || (uint64_t)rg[i].x + rg[i].w > width || (uint64_t)rg[i].y + rg[i].h > height ||
                (uint64_t)rg[i].x0 + rg[i].w > 0x7fffffffu || (uint64_t)rg[i].y0 + rg[i].h > 0x7fffffffu)
                throw Error(J2K_HIP_ERR_PARAM, "DWT region empty or outside the plane");
            for (uint32_t j = 0; j < i; ++j)
                if (rg[i].x < rg[j].x + rg[j].w && rg[j].x < rg[i].x + rg[i].w && rg[i].y < rg[j].y + rg[j].h && rg[j].y < rg[i].y + rg[i].h)
                    throw Error(J2K_HIP_ERR_PARAM, "DWT regions overlap");
        }
        HIP_CHECK(hipSetDevice(e->device));
        hipStream_t s = e->stream;
        const size_t plane = (size_t)width * height, bytes = plane * nplanes * 4;
        e->P.ensure(bytes);
        e->Q.ensure(bytes);
        std::vector<DwtJob> jobs;
        std::vector<size_t> first(levels + 1, 0);
        std::vector<int> mrw(levels, 0), mrh(levels, 0);
        for (uint32_t l = 0; l < levels; ++l) {
            first[l] = jobs.size();
            for (uint32_t c = 0; c < nplanes; ++c)
                for (uint32_t i = 0; i < nregions; ++i) {
                    DwtJob j{};
                    const int ax0 = ceildivpow2((int)rg[i].x0, (int)l), ax1 = ceildivpow2((int)(rg[i].x0 + rg[i].w), (int)l);
                    const int ay0 = ceildivpow2((int)rg[i].y0, (int)l), ay1 = ceildivpow2((int)(rg[i].y0 + rg[i].h), (int)l);
                    j.rw = ax1 - ax0; j.rh = ay1 - ay0; j.casx = ax0 & 1; j.casy = ay0 & 1;
                    if (j.rw <= 0 || j.rh <= 0) continue; // (a single odd-phase sample is all high-pass: nothing is left of it)
                    j.src_off = j.ll_off = j.z_off = (long long)(c * plane) + (long long)rg[i].y * width + rg[i].x;
                    jobs.push_back(j); mrw[l] = std::max(mrw[l], j.rw); mrh[l] = std::max(mrh[l], j.rh);
                }
        }
        first[levels] = jobs.size();
        invalidate_cached_tables(e); // the job table and the planes are overwritten
        HIP_CHECK(hipMemcpyAsync(d_out, d_in, bytes, hipMemcpyDeviceToDevice, s)); // words outside every region stay
        if (!jobs.empty()) {
            e->jobs.ensure(jobs.size() * sizeof(DwtJob));
            HIP_CHECK(hipMemcpyAsync(e->jobs.p, jobs.data(), jobs.size() * sizeof(DwtJob), hipMemcpyHostToDevice, s));
            HIP_CHECK(hipStreamSynchronize(s)); // `jobs` is a pageable host vector
        }
        for (uint32_t l = 0; l < levels; ++l) {
            DwtLevelArgs da{};
            da.src = l == 0 ? d_in : ((l & 1) ? e->Q.p : e->P.p); da.src_stride = width;
            const bool last = l == levels - 1;
            da.ll = last ? d_out : ((l & 1) ? e->P.p : e->Q.p); da.ll_stride = width;
            da.z = d_out; da.z_stride = width;
            da.jobs = e->jobs.as<DwtJob>() + first[l]; da.njobs = (int)(first[l + 1] - first[l]);
            da.max_rw = mrw[l]; da.max_rh = mrh[l]; da.reversible = reversible;
            launch_dwt_level(da, s);
            HIP_CHECK(hipGetLastError());
        }
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

// The front end and the DWT launches of an encode, and nothing behind them: encode_begin's own steps up to the last level
// (device frames, one frame), with a level optionally launched in pieces over row-pair ranges.
int j2k_hip_stage_transform(j2k_hip_encoder *e, const j2k_hip_params *params, const j2k_hip_plane *planes_device,
                            const uint32_t *cuts, const uint32_t *ncuts, uint32_t ncut_levels, int descending, void *d_out)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    return guarded(e, [&] {
        if (e->pend.active) throw Error(J2K_HIP_ERR_PARAM, "the previous j2k_hip_encode_begin on this handle has not been finished");
        if (!planes_device || !d_out) throw Error(J2K_HIP_ERR_PARAM, "planes or d_out is NULL");
        if (ncut_levels && (!ncuts || !cuts)) throw Error(J2K_HIP_ERR_PARAM, "cut points announced but not given");
        HIP_CHECK(hipSetDevice(e->device));
        const Tuning tn = tuning();
        const Coding cod = normalise(params);
        prepare_geometry(e, cod, 0, cod.ntiles());
        // The handle's geometry is this call's now while last_fa still describes an earlier call's channels: nothing may
        // replay them against it (j2k_hip_debug_dwt_time), so the next call builds its geometry afresh.
        invalidate_cached_tables(e);
        const Geometry &g = e->geo;
        hipStream_t s = e->stream;
        const size_t S = e->stride;
        const int NL = (int)cod.levels();
        if (ncut_levels > (uint32_t)NL) throw Error(J2K_HIP_ERR_PARAM, "cut points for more levels than the transform has");
        // row-pair ranges per level: [0, c_1), [c_1, c_2), .., [c_n, end)
        std::vector<std::vector<int>> bounds((size_t)NL);
        const uint32_t *cp = cuts;
        for (int l = 0; l < NL; ++l) {
            int npy = 0; // row pairs of the level's tallest job
            for (const DwtJob &j : e->h_jobs[(size_t)l]) npy = std::max(npy, (j.rh + j.casy + 1) >> 1);
            std::vector<int> &b = bounds[(size_t)l];
            b.push_back(0);
            for (uint32_t i = 0; (uint32_t)l < ncut_levels && i < ncuts[l]; ++i, ++cp) {
                if (*cp >= (uint32_t)npy || (int)*cp <= b.back()) throw Error(J2K_HIP_ERR_PARAM, "cut points must increase and lie inside the level's row pairs");
                b.push_back((int)*cp);
            }
            b.push_back(npy);
        }
        const int y0 = e->box_y0, x0 = e->box_x0;
        int y1 = 0, x1 = 0;
        for (const Tile &T : g.tiles) { y1 = std::max(y1, T.y1); x1 = std::max(x1, T.x1); }
        FrontendArgs fa = make_frontend_args(cod, planes_device, x0, y0, x1, y1);
        const bool fused = fuse_frontend(cod, fa, tn);
        const size_t plane_bytes = e->frame_elems * sizeof(int32_t);
        // (the planes are filled first: a word that no launch writes shows as 0xA5A5A5A5 instead of an earlier call's result)
        if (!fused || NL >= 3) { e->P.ensure(plane_bytes); HIP_CHECK(hipMemsetAsync(e->P.p, 0xA5, plane_bytes, s)); }
        if (NL >= 1) { e->Z.ensure(plane_bytes); HIP_CHECK(hipMemsetAsync(e->Z.p, 0xA5, plane_bytes, s)); }
        if (NL >= 2) { e->Q.ensure(plane_bytes); HIP_CHECK(hipMemsetAsync(e->Q.p, 0xA5, plane_bytes, s)); }
        if (!fused) {
            fa.dst_x0 = x0; fa.dst_y0 = y0;
            run_frontend(e, cod, fa, e->P.as<int32_t>(), e->comp_off, S, s);
        }
        for (int l = 0; l < NL; ++l) {
            const std::vector<int> &b = bounds[(size_t)l];
            const int n = (int)b.size() - 1;
            for (int i = 0; i < n; ++i) {
                const int k = descending ? n - 1 - i : i;
                DwtLevelArgs da = dwt_level_args(e, cod, fa, fused, 0, l);
                if (n > 1) { da.pair0 = b[(size_t)k]; da.pair1 = b[(size_t)k + 1]; }
                launch_dwt_level(da, s);
                HIP_CHECK(hipGetLastError());
            }
        }
        // the coefficient planes without their stride padding (zero levels: the front end's output)
        const uint8_t *from = NL >= 1 ? e->Z.as<uint8_t>() : e->P.as<uint8_t>();
        uint8_t *out = static_cast<uint8_t *>(d_out);
        for (uint32_t c = 0; c < cod.ncomp; ++c) { // (every component at its own size: the box on the component's grid)
            const int sx = cod.cdx[c], sy = cod.cdy[c];
            const size_t W = (size_t)((x1 + sx - 1) / sx - (x0 + sx - 1) / sx), H = (size_t)((y1 + sy - 1) / sy - (y0 + sy - 1) / sy);
            HIP_CHECK(hipMemcpy2DAsync(out, W * 4, from + e->comp_off[c] * 4, S * 4, W * 4, H, hipMemcpyDeviceToDevice, s));
            out += W * H * 4;
        }
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

int j2k_hip_stage_t1(j2k_hip_encoder *e, int reversible, void *d_coef, uint32_t stride, uint32_t nblocks,
                     const uint32_t *bx, const uint32_t *by, const uint32_t *bw, const uint32_t *bh, const uint32_t *orient,
                     const float *stepsize, uint32_t *numbps, uint32_t *npasses, uint32_t *length, uint64_t *offsets,
                     void *data, size_t data_cap)
{
    return j2k_hip_stage_t1_passes(e, reversible, d_coef, stride, nblocks, bx, by, bw, bh, orient, stepsize, numbps, npasses,
                                   length, offsets, data, data_cap, nullptr, nullptr);
}

int j2k_hip_stage_t1_passes(j2k_hip_encoder *e, int reversible, void *d_coef, uint32_t stride, uint32_t nblocks,
                            const uint32_t *bx, const uint32_t *by, const uint32_t *bw, const uint32_t *bh, const uint32_t *orient,
                            const float *stepsize, uint32_t *numbps, uint32_t *npasses, uint32_t *length, uint64_t *offsets,
                            void *data, size_t data_cap, uint32_t *pass_rate, int32_t *pass_dist)
{
    return stage_t1_blocks(e, reversible, d_coef, stride, nblocks, bx, by, bw, bh, orient, stepsize, numbps, npasses, length,
                           offsets, data, data_cap, pass_rate, pass_dist, 0);
}

// No pass_dist here, and so no branch that refuses it under bypass: launch_t1_model picks the distortion instantiation
// (want_dist) before it looks at the bypass bit, and a block modelled that way would hand the raw passes sign XOR
// prediction.  A style excludes rate control in a frame too (geometry.cpp).
int j2k_hip_stage_t1_styled(j2k_hip_encoder *e, int reversible, void *d_coef, uint32_t stride, uint32_t nblocks,
                            const uint32_t *bx, const uint32_t *by, const uint32_t *bw, const uint32_t *bh, const uint32_t *orient,
                            const float *stepsize, uint32_t *numbps, uint32_t *npasses, uint32_t *length, uint64_t *offsets,
                            void *data, size_t data_cap, uint32_t *pass_rate, uint32_t cblk_style)
{
    return stage_t1_blocks(e, reversible, d_coef, stride, nblocks, bx, by, bw, bh, orient, stepsize, numbps, npasses, length,
                           offsets, data, data_cap, pass_rate, nullptr, cblk_style);
}

int j2k_hip_stage_t1_slots(j2k_hip_encoder *e, int reversible, void *d_coef, uint32_t stride, uint32_t nblocks,
                           const uint32_t *bx, const uint32_t *by, const uint32_t *bw, const uint32_t *bh, const uint32_t *orient,
                           const float *stepsize, uint32_t cblk_style, const uint32_t *sym_cap, const uint32_t *out_cap,
                           uint32_t guard_bytes, uint32_t *err, uint32_t *numbps, uint32_t *npasses, uint32_t *nsym, uint32_t *length,
                           uint32_t *pass_rate, void *sym_arena, size_t sym_arena_cap, void *out_arena, size_t out_arena_cap)
{
    const T1Slots slots{sym_cap, out_cap, guard_bytes, err, nsym, sym_arena, sym_arena_cap, out_arena, out_arena_cap};
    return stage_t1_blocks(e, reversible, d_coef, stride, nblocks, bx, by, bw, bh, orient, stepsize, numbps, npasses, length,
                           nullptr, nullptr, 0, pass_rate, nullptr, cblk_style, &slots);
}

// The rate control's kernels alone (rate.hip), on tables the caller supplies, through the objects an encode drives them with:
// the tables go where T1Tables puts a frame's, rate_args lays out the device memory, launch_rate_prepare runs where encode_begin
// queues it, and a HipRateDevice over the uploaded tables answers begin_layer / ahead / scan / scan_sums / fetch -- slot layout,
// copy sizes, memsets and the running sums over `delta` included.  The layouts are the encode's by construction: each has one
// definition (table_layout.h, rate_device.h).
int j2k_hip_stage_rate(j2k_hip_encoder *e, uint32_t nblocks, const double *weight, const uint8_t *comp, const uint32_t *numbps,
                       const uint32_t *npasses, const uint32_t *pass_rate, const int32_t *pass_dist, double *disto, float *reach,
                       double *bounds, uint32_t first, uint32_t count, const uint8_t *done, const double *ahead, uint32_t K,
                       uint64_t *body, const j2k_hip_rate_scan *scans, uint32_t nscans, j2k_hip_rate_taken *taken, uint32_t *bytes,
                       uint64_t *sums)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    return guarded(e, [&] {
        static_assert(sizeof(j2k_hip_rate_taken) == sizeof(Taken), "the scan's records go out as they are");
        static_assert(J2K_HIP_MAX_PASSES == kDevMaxPasses, "the header's row length is the tables'");
        if (e->pend.active) throw Error(J2K_HIP_ERR_PARAM, "the previous j2k_hip_encode_begin on this handle has not been finished");
        const size_t nb = nblocks;
        if (!nb || !weight || !comp || !numbps || !npasses || !pass_rate || !pass_dist || !disto || !reach || !bounds)
            throw Error(J2K_HIP_ERR_PARAM, "rate stage: no blocks, or a table is NULL");
        for (size_t i = 0; i < nb; ++i) {
            if (comp[i] > 3) throw Error(J2K_HIP_ERR_PARAM, "rate stage: component above 3");
            if (numbps[i] > 31) throw Error(J2K_HIP_ERR_PARAM, "rate stage: more than 31 bit-planes");
            if (npasses[i] > (uint32_t)kDevMaxPasses || (npasses[i] && npasses[i] + 2 > 3 * numbps[i]))
                throw Error(J2K_HIP_ERR_PARAM, "rate stage: more passes than the bit-planes hold");
        }
        if (first > nb || count > nb - first) throw Error(J2K_HIP_ERR_PARAM, "rate stage: block range outside the blocks");
        if (K > 128) throw Error(J2K_HIP_ERR_PARAM, "rate stage: more than 128 thresholds ahead");
        if ((K || nscans) && !count) throw Error(J2K_HIP_ERR_PARAM, "rate stage: queries over an empty block range");
        if ((K && (!ahead || !body)) || (nscans && (!scans || !taken || !bytes || !sums)))
            throw Error(J2K_HIP_ERR_PARAM, "rate stage: a query without its arrays");
        for (uint32_t i = 0; done && i < count; ++i)
            if (done[i] > npasses[first + i]) throw Error(J2K_HIP_ERR_PARAM, "rate stage: more passes done than the block has");
        for (uint32_t k = 1; k < K; ++k)
            if (!(ahead[k] <= ahead[k - 1])) throw Error(J2K_HIP_ERR_PARAM, "rate stage: thresholds ahead must descend");
        {
            // a slot whose fetch is put off must still hold its scan at the end
            bool held[3] = {false, false, false};
            for (uint32_t i = 0; i < nscans; ++i) {
                const j2k_hip_rate_scan &q = scans[i];
                if (q.mode > J2K_HIP_RATE_SUMS_FETCH_LAST || (q.mode != J2K_HIP_RATE_SCAN && q.slot > 2))
                    throw Error(J2K_HIP_ERR_PARAM, "rate stage: unknown scan mode or slot");
                const uint32_t k = q.mode == J2K_HIP_RATE_SCAN ? 0u : q.slot;
                if (held[k]) throw Error(J2K_HIP_ERR_PARAM, "rate stage: a scan into a slot whose fetch is still to come");
                if (q.mode == J2K_HIP_RATE_SUMS_FETCH_LAST) held[k] = true;
            }
        }
        HIP_CHECK(hipSetDevice(e->device));
        hipStream_t s = e->stream;
        invalidate_cached_tables(e); // tables of the handle's last frame are overwritten
        // the Tier-1 results where a frame's coder leaves them
        const T1Tables tt(nb);
        const size_t rows = tt.row(nb);
        e->meta.ensure(tt.meta_bytes());
        e->passes.ensure(tt.passes_bytes());
        uint32_t *meta = e->meta.as<uint32_t>();
        uint32_t *pn = e->passes.as<uint32_t>();
        HIP_CHECK(hipMemcpyAsync(tt.numbps(meta), numbps, nb * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(tt.npasses(meta), npasses, nb * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(tt.pass_nmsedec(pn), pass_dist, rows * sizeof(int32_t), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(tt.pass_rate(pn), pass_rate, rows * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        HipRateDevice dev(e, tt);
        const RateArgs &ra = dev.a;
        std::vector<uint8_t> wc(nb * sizeof(double) + nb); // the blocks' components behind their weights, as encode_begin stages them
        std::memcpy(wc.data(), weight, nb * sizeof(double));
        std::memcpy(wc.data() + nb * sizeof(double), comp, nb);
        HIP_CHECK(hipMemcpyAsync(e->rc_weight.p, wc.data(), wc.size(), hipMemcpyHostToDevice, s));
        // (filled first: what the kernel leaves alone -- the rows' entries beyond npasses -- comes back as 0xA5 bytes)
        HIP_CHECK(hipMemsetAsync(ra.disto, 0xA5, rows * sizeof(double), s));
        HIP_CHECK(hipMemsetAsync(ra.reach, 0xA5, rows * sizeof(float), s));
        HIP_CHECK(hipMemsetAsync(e->rc_small.p, 0xA5, dev.lay.total, s));
        launch_rate_prepare(ra, s);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(e->h_rc_bounds.p, ra.bounds, 3 * nb * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(disto, ra.disto, rows * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(reach, ra.reach, rows * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        std::memcpy(bounds, dev.bmin(), nb * sizeof(double));
        std::memcpy(bounds + nb, dev.bmax(), nb * sizeof(double));
        std::memcpy(bounds + 2 * nb, dev.steepest(), nb * sizeof(double));
        if (!K && !nscans) return;
        dev.begin_layer(first, count, done);
        if (K) dev.ahead(first, count, ahead, K, body);
        auto keep = [&](uint32_t i, const Taken *t, const uint32_t *b) {
            std::memcpy(taken + (size_t)i * count, t, (size_t)count * sizeof(Taken));
            std::memcpy(bytes + (size_t)i * count, b, (size_t)count * sizeof(uint32_t));
        };
        for (uint32_t i = 0; i < nscans; ++i) {
            const j2k_hip_rate_scan &q = scans[i];
            const Taken *t = nullptr;
            const uint32_t *b = nullptr;
            if (q.mode == J2K_HIP_RATE_SCAN) {
                dev.scan(first, count, q.thresh, &t, &b, sums + (size_t)i * kRateSums);
                keep(i, t, b);
                continue;
            }
            dev.scan_sums(first, count, q.thresh, (int)q.slot, sums + (size_t)i * kRateSums);
            if (q.mode == J2K_HIP_RATE_SUMS_FETCH) { dev.fetch((int)q.slot, count, &t, &b); keep(i, t, b); }
        }
        for (uint32_t i = 0; i < nscans; ++i) {
            if (scans[i].mode != J2K_HIP_RATE_SUMS_FETCH_LAST) continue;
            const Taken *t = nullptr;
            const uint32_t *b = nullptr;
            dev.fetch((int)scans[i].slot, count, &t, &b);
            keep(i, t, b);
        }
    });
}

// rate_layers_kernel alone, on tables the caller supplies: they go where T1Tables puts a frame's, the launch is the one
// encode_begin queues behind the coder (launch_rate_layers over a RateLayersArgs), the counts come back as encode_end reads them.
int j2k_hip_stage_rate_layers(j2k_hip_encoder *e, uint32_t nblocks, const double *weight, uint32_t nweights, const uint32_t *numbps,
                              const uint32_t *npasses, const uint32_t *pass_rate, const int32_t *pass_dist, const double *slopes,
                              uint32_t layers, uint8_t *passes, uint32_t *bytes, uint32_t *rate_back, int32_t *dist_back)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    return guarded(e, [&] {
        if (e->pend.active) throw Error(J2K_HIP_ERR_PARAM, "the previous j2k_hip_encode_begin on this handle has not been finished");
        const size_t nb = nblocks, L = layers;
        if (!nb || !weight || !numbps || !npasses || !pass_rate || !pass_dist || !slopes || !passes || !bytes)
            throw Error(J2K_HIP_ERR_PARAM, "rate layers stage: no blocks, or a table is NULL");
        if (!nweights || nweights > nb) throw Error(J2K_HIP_ERR_PARAM, "rate layers stage: nweights must be 1..nblocks");
        if (!L || L > kRateMaxLayers) throw Error(J2K_HIP_ERR_PARAM, "rate layers stage: layers must be 1..100");
        for (size_t l = 0; l < L; ++l)
            if (!std::isfinite(slopes[l])) throw Error(J2K_HIP_ERR_PARAM, "rate layers stage: a slope is not finite");
        for (size_t i = 0; i < nb; ++i) {
            if (numbps[i] > 31) throw Error(J2K_HIP_ERR_PARAM, "rate layers stage: more than 31 bit-planes");
            if (npasses[i] > (uint32_t)kDevMaxPasses || (npasses[i] && npasses[i] + 2 > 3 * numbps[i]))
                throw Error(J2K_HIP_ERR_PARAM, "rate layers stage: more passes than the bit-planes hold");
        }
        HIP_CHECK(hipSetDevice(e->device));
        hipStream_t s = e->stream;
        invalidate_cached_tables(e); // tables of the handle's last frame are overwritten
        const T1Tables tt(nb);
        const size_t rows = tt.row(nb);
        e->meta.ensure(tt.meta_bytes());
        e->passes.ensure(tt.passes_bytes());
        uint32_t *meta = e->meta.as<uint32_t>();
        uint32_t *pn = e->passes.as<uint32_t>();
        HIP_CHECK(hipMemcpyAsync(tt.numbps(meta), numbps, nb * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(tt.npasses(meta), npasses, nb * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(tt.pass_nmsedec(pn), pass_dist, rows * sizeof(int32_t), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(tt.pass_rate(pn), pass_rate, rows * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        e->rc_weight.ensure((size_t)nweights * sizeof(double));
        HIP_CHECK(hipMemcpyAsync(e->rc_weight.p, weight, (size_t)nweights * sizeof(double), hipMemcpyHostToDevice, s));
        // (filled first: what the launch leaves alone -- the spare entries behind the last block's -- comes back as 0xA5 bytes)
        const size_t nl = (nb + J2K_HIP_RATE_LAYERS_SPARE) * L, counts = round_up(nl, 256);
        e->rc_layers.ensure(counts + nl * sizeof(uint32_t));
        HIP_CHECK(hipMemsetAsync(e->rc_layers.p, 0xA5, counts + nl * sizeof(uint32_t), s));
        RateLayersArgs la = {};
        la.nblks = (unsigned)nb; la.layers = (unsigned)L; la.nweights = nweights;
        la.weight = e->rc_weight.as<double>();
        la.numbps = tt.numbps(meta); la.npasses = tt.npasses(meta);
        la.pass_nmsedec = reinterpret_cast<const int *>(tt.pass_nmsedec(pn)); la.pass_rate = tt.pass_rate(pn);
        la.passes = e->rc_layers.as<unsigned char>(); la.bytes = reinterpret_cast<unsigned *>(e->rc_layers.as<unsigned char>() + counts);
        launch_rate_layers(la, slopes, s);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(passes, la.passes, nl, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(bytes, la.bytes, nl * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        if (rate_back) HIP_CHECK(hipMemcpyAsync(rate_back, tt.pass_rate(pn), rows * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        if (dist_back) HIP_CHECK(hipMemcpyAsync(dist_back, tt.pass_nmsedec(pn), rows * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

// rate_curve_kernel alone, on tables the caller supplies, read as nframes frames: the tables go where T1Tables puts a call's, the
// launch is the one the budget search makes (launch_rate_curve over a RateCurveArgs), the sums come back whole.
int j2k_hip_stage_rate_curve(j2k_hip_encoder *e, uint32_t nblocks, const double *weight, uint32_t nweights, const uint32_t *numbps,
                             const uint32_t *npasses, const uint32_t *pass_rate, const int32_t *pass_dist, uint32_t nframes,
                             const int32_t *cap, int32_t base, uint32_t step, uint32_t K, uint64_t *sums, uint32_t *rate_back,
                             int32_t *dist_back)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    return guarded(e, [&] {
        static_assert(J2K_HIP_RATE_CURVE_MAX == kRateCurveMax, "the header's candidate count is the kernel's");
        static_assert(J2K_HIP_SLOPE_K_MIN == kSlopeKMin && J2K_HIP_SLOPE_K_MAX == kSlopeKMax && J2K_HIP_SLOPE_ALL == kSlopeAll, "one grid");
        if (e->pend.active) throw Error(J2K_HIP_ERR_PARAM, "the previous j2k_hip_encode_begin on this handle has not been finished");
        const size_t nb = nblocks, F = nframes;
        if (!nb || !weight || !numbps || !npasses || !pass_rate || !pass_dist || !cap || !sums)
            throw Error(J2K_HIP_ERR_PARAM, "rate curve stage: no blocks, or a table is NULL");
        if (!F || nb % F) throw Error(J2K_HIP_ERR_PARAM, "rate curve stage: nframes must divide nblocks");
        if (!nweights || nweights > nb) throw Error(J2K_HIP_ERR_PARAM, "rate curve stage: nweights must be 1..nblocks");
        if (!K || K > kRateCurveMax) throw Error(J2K_HIP_ERR_PARAM, "rate curve stage: K must be 1..64");
        if (!step) throw Error(J2K_HIP_ERR_PARAM, "rate curve stage: step must not be 0");
        if (base < kSlopeAll || base > kSlopeKMax) throw Error(J2K_HIP_ERR_PARAM, "rate curve stage: base outside the slope grid");
        for (size_t f = 0; f < F; ++f)
            if (cap[f] < kSlopeAll || cap[f] > kSlopeKMax) throw Error(J2K_HIP_ERR_PARAM, "rate curve stage: a cap outside the slope grid");
        for (size_t i = 0; i < nb; ++i) {
            if (numbps[i] > 31) throw Error(J2K_HIP_ERR_PARAM, "rate curve stage: more than 31 bit-planes");
            if (npasses[i] > (uint32_t)kDevMaxPasses || (npasses[i] && npasses[i] + 2 > 3 * numbps[i]))
                throw Error(J2K_HIP_ERR_PARAM, "rate curve stage: more passes than the bit-planes hold");
        }
        HIP_CHECK(hipSetDevice(e->device));
        hipStream_t s = e->stream;
        invalidate_cached_tables(e); // tables of the handle's last frame are overwritten
        const T1Tables tt(nb);
        const size_t rows = tt.row(nb);
        e->meta.ensure(tt.meta_bytes());
        e->passes.ensure(tt.passes_bytes());
        uint32_t *meta = e->meta.as<uint32_t>();
        uint32_t *pn = e->passes.as<uint32_t>();
        HIP_CHECK(hipMemcpyAsync(tt.numbps(meta), numbps, nb * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(tt.npasses(meta), npasses, nb * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(tt.pass_nmsedec(pn), pass_dist, rows * sizeof(int32_t), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(tt.pass_rate(pn), pass_rate, rows * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        e->rc_weight.ensure((size_t)nweights * sizeof(double));
        HIP_CHECK(hipMemcpyAsync(e->rc_weight.p, weight, (size_t)nweights * sizeof(double), hipMemcpyHostToDevice, s));
        // [sums F x K x 2][spare][caps F]: the spare entries are filled and come back, the sums proper start at zero
        const size_t nsums = F * K * 2, all = nsums + J2K_HIP_RATE_LAYERS_SPARE, caps_at = round_up(all * sizeof(uint64_t), 256);
        e->rc_layers.ensure(caps_at + F * sizeof(int32_t));
        uint8_t *d = e->rc_layers.as<uint8_t>();
        HIP_CHECK(hipMemsetAsync(d, 0xA5, all * sizeof(uint64_t), s));
        HIP_CHECK(hipMemsetAsync(d, 0, nsums * sizeof(uint64_t), s));
        HIP_CHECK(hipMemcpyAsync(d + caps_at, cap, F * sizeof(int32_t), hipMemcpyHostToDevice, s));
        RateCurveArgs ca = {};
        ca.nblks = (unsigned)nb; ca.nb1 = (unsigned)(nb / F); ca.nweights = nweights;
        ca.K = K; ca.step = step; ca.base = base;
        ca.weight = e->rc_weight.as<double>();
        ca.numbps = tt.numbps(meta); ca.npasses = tt.npasses(meta);
        ca.pass_nmsedec = reinterpret_cast<const int *>(tt.pass_nmsedec(pn)); ca.pass_rate = tt.pass_rate(pn);
        ca.cap = reinterpret_cast<const int *>(d + caps_at);
        ca.sums = reinterpret_cast<unsigned long long *>(d);
        launch_rate_curve(ca, s);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(sums, d, all * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        if (rate_back) HIP_CHECK(hipMemcpyAsync(rate_back, tt.pass_rate(pn), rows * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        if (dist_back) HIP_CHECK(hipMemcpyAsync(dist_back, tt.pass_nmsedec(pn), rows * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

// One launch_gather over pieces the caller supplies: the plan is laid out and its GatherArgs filled by the GatherPlan an encode
// uses (table_layout.h) -- encode_end's table order by construction -- with block pieces as a CblkDev table, the blocks' lengths
// in the `len` column of T1Tables and cblk_dst, as a frame has them, and segments alone as the decoder has them.
int j2k_hip_stage_gather(j2k_hip_encoder *e, const void *src, size_t src_bytes, const void *blob, size_t blob_bytes, void *dst,
                         size_t dst_bytes, const j2k_hip_gather_piece *blocks, uint32_t nblocks, const j2k_hip_gather_piece *headers,
                         uint32_t nheaders, const j2k_hip_gather_piece *segments, uint32_t nsegments)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    return guarded(e, [&] {
        if (e->pend.active) throw Error(J2K_HIP_ERR_PARAM, "the previous j2k_hip_encode_begin on this handle has not been finished");
        if ((src_bytes && !src) || (blob_bytes && !blob) || (dst_bytes && !dst) || (nblocks && !blocks) || (nheaders && !headers) ||
            (nsegments && !segments))
            throw Error(J2K_HIP_ERR_PARAM, "gather stage: a buffer or a piece list is NULL");
        const size_t nbd = nblocks, nh = nheaders, nseg = nsegments;
        if (nbd + nh + nseg > (size_t)INT32_MAX) throw Error(J2K_HIP_ERR_PARAM, "gather stage: too many pieces");
        std::vector<std::pair<uint64_t, uint64_t>> spans; // destination [begin, end) of every piece that writes
        auto piece = [&](const j2k_hip_gather_piece &p, size_t from_bytes) {
            if (p.src > from_bytes || p.len > from_bytes - p.src) throw Error(J2K_HIP_ERR_PARAM, "gather stage: a piece reads outside its source");
            if (p.dst > dst_bytes || p.len > dst_bytes - p.dst) throw Error(J2K_HIP_ERR_PARAM, "gather stage: a piece writes outside the destination");
            if (p.len) spans.emplace_back(p.dst, p.dst + p.len);
        };
        for (size_t i = 0; i < nbd; ++i) {
            if (blocks[i].src & 3) throw Error(J2K_HIP_ERR_PARAM, "gather stage: a block's source is not 4-byte aligned");
            piece(blocks[i], src_bytes);
        }
        for (size_t i = 0; i < nh; ++i) {
            if (headers[i].src > UINT32_MAX) throw Error(J2K_HIP_ERR_PARAM, "gather stage: a header's source offset needs more than 32 bits");
            piece(headers[i], blob_bytes);
        }
        for (size_t i = 0; i < nseg; ++i) piece(segments[i], src_bytes);
        std::sort(spans.begin(), spans.end());
        for (size_t i = 1; i < spans.size(); ++i)
            if (spans[i].first < spans[i - 1].second) throw Error(J2K_HIP_ERR_PARAM, "gather stage: destinations overlap");
        if (!(nbd + nh + nseg)) return;
        HIP_CHECK(hipSetDevice(e->device));
        hipStream_t s = e->stream;
        invalidate_cached_tables(e); // the block table is overwritten
        const GatherPlan lay(blob_bytes, nh, nbd, nseg);
        std::vector<uint8_t> hplan(lay.total, 0);
        if (blob_bytes) std::memcpy(hplan.data(), blob, blob_bytes);
        const GatherTables h = lay.tables(hplan.data());
        for (size_t i = 0; i < nh; ++i) { h.hdr_dst[i] = headers[i].dst; h.hdr_src[i] = (uint32_t)headers[i].src; h.hdr_len[i] = headers[i].len; }
        for (size_t i = 0; i < nseg; ++i) { h.seg_dst[i] = segments[i].dst; h.seg_src[i] = segments[i].src; h.seg_len[i] = segments[i].len; }
        std::vector<CblkDev> blks(std::max<size_t>(1, nbd));
        std::vector<uint32_t> lens(std::max<size_t>(1, nbd));
        for (size_t i = 0; i < nbd; ++i) { h.cblk_dst[i] = blocks[i].dst; blks[i] = CblkDev{}; blks[i].out_off = blocks[i].src; lens[i] = blocks[i].len; }
        const T1Tables tt(nbd);
        e->plan.ensure(lay.total);
        e->cs.ensure(dst_bytes + 64);
        e->out.ensure(src_bytes + 64); // (as a frame's: a misaligned piece's last source word may end up to three bytes behind it)
        e->blks.ensure(blks.size() * sizeof(CblkDev));
        e->meta.ensure(tt.meta_bytes());
        HIP_CHECK(hipMemcpyAsync(e->plan.p, hplan.data(), lay.total, hipMemcpyHostToDevice, s));
        if (src_bytes) HIP_CHECK(hipMemcpyAsync(e->out.p, src, src_bytes, hipMemcpyHostToDevice, s));
        if (dst_bytes) HIP_CHECK(hipMemcpyAsync(e->cs.p, dst, dst_bytes, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(e->blks.p, blks.data(), blks.size() * sizeof(CblkDev), hipMemcpyHostToDevice, s));
        uint32_t *len = tt.len(e->meta.as<uint32_t>());
        HIP_CHECK(hipMemcpyAsync(len, lens.data(), lens.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        GatherArgs ga{};
        lay.fill(ga, e->plan.as<uint8_t>());
        ga.dst = e->cs.as<uint8_t>();
        ga.out = e->out.as<uint8_t>(); ga.blks = e->blks.as<CblkDev>(); ga.len = len; ga.nblks = (int)nbd;
        launch_gather(ga, s);
        HIP_CHECK(hipGetLastError());
        if (dst_bytes) HIP_CHECK(hipMemcpyAsync(dst, e->cs.p, dst_bytes, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

int j2k_hip_stage_pack_offsets(j2k_hip_encoder *e, const uint32_t *len, uint32_t n, uint64_t base, uint64_t *dst)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    return guarded(e, [&] {
        if (e->pend.active) throw Error(J2K_HIP_ERR_PARAM, "the previous j2k_hip_encode_begin on this handle has not been finished");
        if (!n) return;
        if (!len || !dst || n > (uint32_t)INT32_MAX) throw Error(J2K_HIP_ERR_PARAM, "pack offsets stage: an array is NULL, or too many lengths");
        HIP_CHECK(hipSetDevice(e->device));
        hipStream_t s = e->stream;
        e->meta.ensure(((size_t)n + 4) * sizeof(uint32_t));
        e->pack_dst.ensure((size_t)n * sizeof(uint64_t));
        invalidate_cached_tables(e); // (a band-pipelined call's destinations are overwritten)
        HIP_CHECK(hipMemcpyAsync(e->meta.p, len, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        launch_pack_offsets(e->meta.as<unsigned>(), (int)n, base, e->pack_dst.as<unsigned long long>(), s);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(dst, e->pack_dst.p, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

} // extern "C"

// ---- host-only hooks (no handle, no device): a frame's code-block table and host Tier-2 on block results the caller supplies
namespace {
template <typename F> int host_guarded(F &&f)
{
    try {
        f();
        return J2K_HIP_OK;
    } catch (const Error &x) {
        create_error() = x.what();
        return x.code;
    } catch (const std::exception &x) {
        create_error() = x.what();
        return J2K_HIP_ERR_PARAM;
    }
}
} // namespace

extern "C" {

int j2k_hip_debug_cblk_capacities(uint32_t area, uint32_t Mb, uint32_t cblk_style, uint64_t *decisions, uint64_t *codeword)
{
    return host_guarded([&] {
        if (!area || area > 4096 || Mb > 37) throw Error(J2K_HIP_ERR_PARAM, "code-block capacities: area must be 1..4096, Mb at most 37");
        const CblkCaps caps = cblk_capacities(area, Mb, cblk_style);
        if (decisions) *decisions = caps.sym;
        if (codeword) *codeword = caps.out;
    });
}

int j2k_hip_debug_blocks(const j2k_hip_params *params, uint32_t *rows, size_t cap, size_t *nblocks)
{
    return host_guarded([&] {
        const Coding cod = normalise(params);
        const Geometry g = build_geometry(cod, 0, cod.ntiles());
        if (nblocks) *nblocks = g.cblks.size();
        if (!rows) return;
        if (g.cblks.size() > cap) throw Error(J2K_HIP_ERR_OVERFLOW, "block table too small");
        for (size_t i = 0; i < g.cblks.size(); ++i) {
            const Cblk &c = g.cblks[i];
            const uint32_t r[10] = {c.tile, c.comp, c.res, c.band, c.orient, c.px, c.py, c.w, c.h, c.Mb};
            std::memcpy(rows + 10 * i, r, sizeof r);
        }
    });
}

int j2k_hip_guard_bits_needed(const j2k_hip_params *params, const uint32_t *numbps, size_t nblocks, uint32_t *g)
{
    return host_guarded([&] {
        if (!numbps || !g) throw Error(J2K_HIP_ERR_PARAM, "guard bits needed: an argument is NULL");
        const Coding cod = normalise(params);
        const Geometry geo = build_geometry(cod, 0, cod.ntiles());
        if (nblocks != geo.cblks.size()) throw Error(J2K_HIP_ERR_PARAM, "guard bits needed: the frame has " + std::to_string(geo.cblks.size()) + " code-blocks");
        std::vector<CblkResult> res(nblocks);
        for (size_t i = 0; i < nblocks; ++i) res[i] = CblkResult{numbps[i], 0, 0};
        *g = guard_bits_needed(geo, res);
    });
}

int j2k_hip_debug_tier2(const j2k_hip_params *params, const uint32_t *numbps, const uint32_t *npasses, const uint32_t *length,
                        size_t nblocks, int pricer, uint64_t *total_len)
{
    return j2k_hip_debug_tier2_guard(params, numbps, npasses, length, nblocks, pricer, total_len, nullptr);
}

int j2k_hip_debug_tier2_guard(const j2k_hip_params *params, const uint32_t *numbps, const uint32_t *npasses, const uint32_t *length,
                              size_t nblocks, int pricer, uint64_t *total_len, uint32_t *guard_bits)
{
    return host_guarded([&] {
        if (!numbps || !npasses || !length) throw Error(J2K_HIP_ERR_PARAM, "Tier-2 hook: an array is NULL");
        const Coding cod = normalise(params);
        if (cod.cblk_style) throw Error(J2K_HIP_ERR_PARAM, "Tier-2 hook: no code-block style (a styled block needs its per-pass byte counts)");
        const Geometry g = build_geometry(cod, 0, cod.ntiles());
        if (nblocks != g.cblks.size()) throw Error(J2K_HIP_ERR_PARAM, "Tier-2 hook: the frame has " + std::to_string(g.cblks.size()) + " code-blocks");
        std::vector<CblkResult> res(nblocks);
        for (size_t i = 0; i < nblocks; ++i) res[i] = CblkResult{numbps[i], npasses[i], length[i]};
        auto run = [&](const Geometry &gg) {
            uint64_t total = 0;
            if (pricer) {
                for (const Tile &T : gg.tiles) { TilePricer tp(gg, T, res); total += tp.committed(); }
            } else {
                total = plan_codestream(gg, res, true, true).total_len;
            }
            return total;
        };
        // (an encode's own path: at the guard bits of the parameters, and under J2K_HIP_GUARD_AUTO once more on an excess)
        uint64_t total = 0;
        uint32_t guard = cod.guard;
        try { total = run(g); }
        catch (const GuardExcess &) {
            if (!cod.guard_auto) throw;
            guard = guard_bits_needed(g, res);
            total = run(with_guard_bits(g, guard));
        }
        if (total_len) *total_len = total;
        if (guard_bits) *guard_bits = guard;
    });
}

int j2k_hip_debug_tier2_plan(const j2k_hip_params *params, const uint32_t *numbps, const uint32_t *npasses, const uint32_t *length,
                             size_t nblocks, const uint32_t *pass_rate, const uint32_t *alloc_np, const uint32_t *alloc_len,
                             const uint32_t *alloc_off, uint32_t alloc_layers, uint32_t nworkers, j2k_hip_tier2_plan *out)
{
    return host_guarded([&] {
        if (!numbps || !npasses || !length || !out) throw Error(J2K_HIP_ERR_PARAM, "Tier-2 plan hook: an array is NULL");
        const Coding cod = normalise(params);
        if (cod.cblk_style && !pass_rate) throw Error(J2K_HIP_ERR_PARAM, "Tier-2 plan hook: a code-block style needs the per-pass byte counts");
        if (!cod.cblk_style && pass_rate) throw Error(J2K_HIP_ERR_PARAM, "Tier-2 plan hook: per-pass byte counts without a code-block style");
        const bool with_alloc = alloc_np || alloc_len || alloc_off;
        if (with_alloc && !(alloc_np && alloc_len && alloc_off)) throw Error(J2K_HIP_ERR_PARAM, "Tier-2 plan hook: a layer allocation is np, len and off");
        if (with_alloc && alloc_layers != cod.layers) throw Error(J2K_HIP_ERR_PARAM, "Tier-2 plan hook: the allocation's layers are not the parameters'");
        if (nworkers > 64) throw Error(J2K_HIP_ERR_PARAM, "Tier-2 plan hook: more than 64 workers");
        const Geometry g = build_geometry(cod, 0, cod.ntiles());
        if (nblocks != g.cblks.size()) throw Error(J2K_HIP_ERR_PARAM, "Tier-2 plan hook: the frame has " + std::to_string(g.cblks.size()) + " code-blocks");
        std::vector<CblkResult> res(nblocks);
        for (size_t i = 0; i < nblocks; ++i) {
            res[i] = CblkResult{numbps[i], npasses[i], length[i]};
            if (npasses[i] > (uint32_t)kMaxPasses) throw Error(J2K_HIP_ERR_PARAM, "Tier-2 plan hook: more passes than the pass tables hold");
            if (pass_rate) {
                const uint32_t *r = pass_rate + i * (size_t)kMaxPasses;
                for (uint32_t p = 0; p < npasses[i]; ++p)
                    if (r[p] > length[i] || (p && r[p] < r[p - 1])) throw Error(J2K_HIP_ERR_PARAM, "Tier-2 plan hook: per-pass byte counts must not decrease nor pass the length");
                res[i].rates = r;
            }
        }
        LayerAlloc alloc;
        if (with_alloc) {
            const size_t n = nblocks * (size_t)alloc_layers;
            alloc.layers = alloc_layers;
            alloc.np.assign(alloc_np, alloc_np + n); alloc.len.assign(alloc_len, alloc_len + n); alloc.off.assign(alloc_off, alloc_off + n);
            for (size_t i = 0; i < nblocks; ++i) {
                uint64_t passes = 0;
                for (uint32_t l = 0; l < alloc_layers; ++l) {
                    const size_t k = i * alloc_layers + l;
                    passes += alloc.np[k];
                    if (alloc.np[k] && (alloc.off[k] > length[i] || alloc.len[k] > length[i] - alloc.off[k]))
                        throw Error(J2K_HIP_ERR_PARAM, "Tier-2 plan hook: a layer's bytes lie outside the block's");
                }
                if (passes > npasses[i]) throw Error(J2K_HIP_ERR_PARAM, "Tier-2 plan hook: the layers hold more passes than the block has");
            }
        }
        std::unique_ptr<Workers> workers;
        if (nworkers) workers.reset(new Workers(nworkers));
        auto run = [&](const Geometry &gg) { return plan_codestream(gg, res, true, true, with_alloc ? &alloc : nullptr, workers.get()); };
        // (an encode's own path, as j2k_hip_debug_tier2_guard walks it)
        Tier2Plan plan;
        uint32_t guard = cod.guard;
        try { plan = run(g); }
        catch (const GuardExcess &) {
            if (!cod.guard_auto) throw;
            guard = guard_bits_needed(g, res);
            plan = run(with_guard_bits(g, guard));
        }
        out->total_len = plan.total_len;
        out->guard_bits = guard;
        out->blob_bytes = plan.blob.size();
        out->nheaders = plan.hdr_segs.size();
        out->ncblk_dst = plan.cblk_dst.size();
        out->nbodies = plan.body_segs.size();
        if (out->blob) {
            if (out->blob_cap < plan.blob.size()) throw Error(J2K_HIP_ERR_OVERFLOW, "Tier-2 plan hook: blob buffer too small");
            if (!plan.blob.empty()) std::memcpy(out->blob, plan.blob.data(), plan.blob.size());
        }
        if (out->hdr_dst || out->hdr_src || out->hdr_len) {
            if (!(out->hdr_dst && out->hdr_src && out->hdr_len)) throw Error(J2K_HIP_ERR_PARAM, "Tier-2 plan hook: header pieces are hdr_dst, hdr_src and hdr_len");
            if (out->hdr_cap < plan.hdr_segs.size()) throw Error(J2K_HIP_ERR_OVERFLOW, "Tier-2 plan hook: header piece arrays too small");
            for (size_t i = 0; i < plan.hdr_segs.size(); ++i) {
                out->hdr_dst[i] = plan.hdr_segs[i].dst; out->hdr_src[i] = plan.hdr_segs[i].src; out->hdr_len[i] = plan.hdr_segs[i].len;
            }
        }
        if (out->cblk_dst) {
            if (out->cblk_cap < plan.cblk_dst.size()) throw Error(J2K_HIP_ERR_OVERFLOW, "Tier-2 plan hook: cblk_dst array too small");
            std::copy(plan.cblk_dst.begin(), plan.cblk_dst.end(), out->cblk_dst);
        }
        if (out->body_dst || out->body_cblk || out->body_off || out->body_len) {
            if (!(out->body_dst && out->body_cblk && out->body_off && out->body_len))
                throw Error(J2K_HIP_ERR_PARAM, "Tier-2 plan hook: body pieces are body_dst, body_cblk, body_off and body_len");
            if (out->body_cap < plan.body_segs.size()) throw Error(J2K_HIP_ERR_OVERFLOW, "Tier-2 plan hook: body piece arrays too small");
            for (size_t i = 0; i < plan.body_segs.size(); ++i) {
                const BodySeg &b = plan.body_segs[i];
                out->body_dst[i] = b.dst; out->body_cblk[i] = b.cblk; out->body_off[i] = b.off; out->body_len[i] = b.len;
            }
        }
    });
}

} // extern "C"
