// compare.cpp -- j2k_hip_compare and its relatives (include/j2k_hip.h, "compare a file with its source frame"): what did a
// file lose against the frame it was written from?
//
//   file bytes (host) -> j2k_hip_decode_device, as it is, into dense 16-bit component planes of the file's depth (cmp_dec)
//   source planes (host: uploaded like an encode's; device: read in place)
//   -> compare_kernel (compare.hip): source samples made as the encode's front end makes them, against the decoded planes
//   -> a few 64-bit sums per component -> host: j2k_hip_diff
//
// Where the source samples come from.  Components that share the image's grid are read straight from the caller's planes, all
// of them in one launch.  Sub-sampled components given as planes of their own (comp_sub_x / _y) are read straight too, one
// launch per component, as the front end runs them.  rgb_to_sycc is the exception: the existing Y Cb Cr front-end kernel runs
// into the handle's working planes (as for a reversible frame: integers) and the compare reads those -- its decimation keeps
// one definition.  rgb_to_xyz likewise: the X'Y'Z' front-end kernel (its tables on the handle) writes the codes the compare reads.
// The decoded image is never downloaded.
#include <algorithm>
#include <cmath>
#include <limits>

#include "decode_plan.h"
#include "handle.h"

using namespace j2k_hip;

namespace {

// What of j2k_hip_params defines the source samples and their geometry, normalised; the coding fields are not read.
struct Source {
    Coding cod;
    uint32_t cw[4] = {0, 0, 0, 0}, ch[4] = {0, 0, 0, 0}; // every component's own grid
};
Source source_of(const j2k_hip_params *p)
{
    if (!p) throw Error(J2K_HIP_ERR_PARAM, "params is NULL");
    if (!params_size_ok(p)) throw Error(J2K_HIP_ERR_PARAM, "j2k_hip_params.struct_size mismatch (ABI drift)");
    j2k_hip_params q{};
    q.struct_size = sizeof(q);
    q.width = p->width; q.height = p->height; q.channels = p->channels; q.depth = p->depth;
    q.promote_ae16 = p->promote_ae16;
    for (int c = 0; c < 4; ++c) { q.comp_sub_x[c] = p->comp_sub_x[c]; q.comp_sub_y[c] = p->comp_sub_y[c]; }
    q.rgb_to_sycc = p->rgb_to_sycc; q.rgb_to_xyz = p->rgb_to_xyz;
    q.reversible = 1; q.num_resolutions = 1; q.comment = ""; // (integers out of the Y Cb Cr front end; no limit from a wavelet)
    Source s;
    s.cod = normalise(&q);
    for (uint32_t c = 0; c < s.cod.ncomp; ++c) {
        s.cw[c] = (s.cod.width + s.cod.cdx[c] - 1) / s.cod.cdx[c];
        s.ch[c] = (s.cod.height + s.cod.cdy[c] - 1) / s.cod.cdy[c];
        if ((uint64_t)s.cw[c] * s.ch[c] >= (1ull << 32))
            throw Error(J2K_HIP_ERR_PARAM, "width x height: component " + std::to_string(c) + " has 2^32 samples or more (sum_sq could not hold their squares)");
    }
    return s;
}

// Does the file describe the image of the parameters?  J2K_HIP_ERR_PARAM, the text naming the field.
void check_agreement(const Source &s, const FileHeader &H)
{
    const Coding &f = H.cod, &p = s.cod;
    auto differs = [](const char *field, const std::string &file, const std::string &params) {
        throw Error(J2K_HIP_ERR_PARAM, std::string(field) + ": the file has " + file + ", the parameters " + params);
    };
    if (f.width != p.width) differs("width", std::to_string(f.width), std::to_string(p.width));
    if (f.height != p.height) differs("height", std::to_string(f.height), std::to_string(p.height));
    if (f.ncomp_out() != p.ncomp) differs("channels", std::to_string(f.ncomp_out()), std::to_string(p.ncomp));
    for (uint32_t c = 0; c < p.ncomp; ++c) {
        const std::string comp = " for component " + std::to_string(c);
        if (f.cdx[c] != p.cdx[c] || f.cdy[c] != p.cdy[c])
            differs("comp_sub_x / comp_sub_y", "(" + std::to_string(f.cdx[c]) + ", " + std::to_string(f.cdy[c]) + ")" + comp,
                    "(" + std::to_string(p.cdx[c]) + ", " + std::to_string(p.cdy[c]) + ")");
        if (f.csgnd[c]) throw Error(J2K_HIP_ERR_PARAM, "comp_signed: component " + std::to_string(c) + " of the file is signed, source samples are unsigned");
        if (f.cprec[c] != p.prec) differs("depth", std::to_string((unsigned)f.cprec[c]) + " bits" + comp, std::to_string(p.prec));
    }
}

FileHeader checked_header(const Source &s, const void *file, size_t len)
{
    if (!file || !len) throw Error(J2K_HIP_ERR_PARAM, "Error reading file: empty input");
    FileHeader H = parse_headers(static_cast<const uint8_t *>(file), len);
    check_agreement(s, H);
    return H;
}

void check_diffs(const Source &s, const j2k_hip_diff *diffs, uint32_t ndiffs)
{
    if (!diffs || !ndiffs) throw Error(J2K_HIP_ERR_PARAM, "no place for the results");
    for (uint32_t c = 0; c < ndiffs && c < s.cod.ncomp; ++c)
        if (diffs[c].struct_size != sizeof(j2k_hip_diff)) throw Error(J2K_HIP_ERR_PARAM, "j2k_hip_diff.struct_size mismatch (ABI drift)");
}

// every channel a dense plane of 8- or 16-bit samples that four-sample loads may read
bool wide_planes(const FrontendArgs &fa)
{
    if (fa.interleaved) return false;
    for (int c = 0; c < fa.ncomp; ++c) {
        const long long sb = fa.sample_bytes[c];
        if ((sb != 1 && sb != 2) || fa.colbytes[c] != sb || reinterpret_cast<uintptr_t>(fa.src[c]) % (uintptr_t)(4 * sb) || fa.rowbytes[c] % (4 * sb)) return false;
    }
    return true;
}

// Decoded component c: dense 16-bit samples at row stride `stride`, the component's sample (x, y) at (x * sx, y * sy).
struct Decoded { const uint16_t *plane[4]; long long stride[4]; int sx[4], sy[4]; };

// The launches and the results: dplanes are the source's channel views on the device.
void reduce(j2k_hip_encoder *e, const Source &src, const j2k_hip_plane *dplanes, const Decoded &D, j2k_hip_diff *diffs, uint32_t ndiffs)
{
    const Coding &cod = src.cod;
    hipStream_t s = e->stream;
    const size_t acc_bytes = (size_t)kCompareSets * 4 * kCompareWords * sizeof(unsigned long long);
    e->cmp_acc.ensure(acc_bytes);
    e->h_cmp.ensure(acc_bytes);
    HIP_CHECK(hipMemsetAsync(e->cmp_acc.p, 0, acc_bytes, s));
    FrontendArgs fa = make_frontend_args(cod, dplanes, 0, 0, (int)cod.width, (int)cod.height);
    CompareArgs base{};
    base.acc = e->cmp_acc.as<unsigned long long>();
    auto decoded = [&](CompareArgs &a, int k, uint32_t c) {
        a.dec[k] = D.plane[c]; a.dec_stride[k] = D.stride[c]; a.dec_sx[k] = D.sx[c]; a.dec_sy[k] = D.sy[c]; a.slot[k] = (int)c;
    };
    if (cod.rgb_to_sycc || cod.rgb_to_xyz) {
        // Y, Cb, Cr[, A] -- or X', Y', Z'[, A] -- by the front end's own kernel into the working planes; components of one grid share a launch
        const PlaneLayout lay = plane_layout(cod, 0, 0, (int)cod.width, (int)cod.height);
        e->P.ensure(lay.frame_elems * sizeof(int32_t));
        run_frontend(e, cod, fa, e->P.as<int32_t>(), lay.comp_off, lay.stride, s);
        HIP_CHECK(hipGetLastError());
        bool done[4] = {false, false, false, false};
        for (uint32_t c = 0; c < cod.ncomp; ++c) {
            if (done[c]) continue;
            CompareArgs a = base;
            a.plane_stride = (long long)lay.stride; a.plane_dc = 1 << (cod.prec - 1);
            a.width = (int)src.cw[c]; a.height = (int)src.ch[c];
            for (uint32_t k = c; k < cod.ncomp; ++k)
                if (!done[k] && src.cw[k] == src.cw[c] && src.ch[k] == src.ch[c]) {
                    a.planes[a.ncomp] = e->P.as<int32_t>() + lay.comp_off[k];
                    decoded(a, a.ncomp++, k);
                    done[k] = true;
                }
            launch_compare(a, s);
        }
    } else if (!cod.subsampled()) {
        CompareArgs a = base;
        a.src = fa; a.wide = wide_planes(fa);
        a.ncomp = (int)cod.ncomp; a.width = (int)cod.width; a.height = (int)cod.height;
        for (uint32_t c = 0; c < cod.ncomp; ++c) decoded(a, (int)c, c);
        launch_compare(a, s);
    } else {
        // planes of the components' own sizes: every component is a frame of its own, as the front end runs them
        for (uint32_t c = 0; c < cod.ncomp; ++c) {
            CompareArgs a = base;
            FrontendArgs &f1 = a.src;
            f1 = fa;
            f1.ncomp = 1; f1.interleaved = 0;
            f1.src[0] = fa.src[c]; f1.colbytes[0] = fa.colbytes[c]; f1.rowbytes[0] = fa.rowbytes[c];
            f1.sample_bytes[0] = fa.sample_bytes[c]; f1.src_depth[0] = fa.src_depth[c];
            a.wide = wide_planes(f1);
            a.ncomp = 1; a.width = (int)src.cw[c]; a.height = (int)src.ch[c];
            decoded(a, 0, c);
            launch_compare(a, s);
        }
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(e->h_cmp.p, e->cmp_acc.p, acc_bytes, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    const unsigned long long *sets = e->h_cmp.as<unsigned long long>();
    const double top = (double)((1u << cod.prec) - 1u);
    for (uint32_t c = 0; c < ndiffs && c < cod.ncomp; ++c) {
        unsigned long long w[5] = {0, 0, 0, 0, 0}; // the sets of accumulators folded: sums, maxima
        for (int k = 0; k < kCompareSets; ++k) {
            const unsigned long long *v = sets + (size_t)kCompareWords * (4 * k + c);
            w[0] += v[0]; w[1] += v[1]; w[2] += v[2];
            w[3] = std::max(w[3], v[3]); w[4] = std::max(w[4], v[4]);
        }
        j2k_hip_diff d{};
        d.struct_size = sizeof(d);
        d.samples = (uint64_t)src.cw[c] * src.ch[c];
        d.sum_sq = w[0]; d.sum_abs = w[1]; d.differing = w[2]; d.max_abs = (uint32_t)w[3];
        if (d.differing) {
            const unsigned long long first = ~w[4];
            d.first_x = (uint32_t)(first % src.cw[c]); d.first_y = (uint32_t)(first / src.cw[c]);
        }
        d.mse = (double)d.sum_sq / (double)d.samples;
        d.psnr = d.sum_sq ? 10.0 * std::log10((top * top) / d.mse) : std::numeric_limits<double>::infinity();
        diffs[c] = d;
    }
}

void compare_file(j2k_hip_encoder *e, const j2k_hip_params *params, const j2k_hip_plane *planes, bool on_device, const void *file,
                  size_t len, j2k_hip_diff *diffs, uint32_t ndiffs)
{
    if (e->pend.active) throw Error(J2K_HIP_ERR_PARAM, "an encode is in progress on this handle");
    const Source src = source_of(params);
    (void)checked_header(src, file, len);
    check_diffs(src, diffs, ndiffs);
    if (!planes) throw Error(J2K_HIP_ERR_PARAM, "planes is NULL");
    const Coding &cod = src.cod;
    (void)make_frontend_args(cod, planes, 0, 0, (int)cod.width, (int)cod.height); // (the channel views are checked before any device work)
    HIP_CHECK(hipSetDevice(e->device));
    // the decode as it is: component planes of the file's depth, full size (a sub-sampled component arrives replicated)
    const size_t plane = (size_t)cod.width * cod.height;
    e->cmp_dec.ensure(plane * cod.ncomp * sizeof(uint16_t) + 16);
    j2k_hip_outplane out[4];
    Decoded D{};
    for (uint32_t c = 0; c < cod.ncomp; ++c) {
        uint16_t *p = e->cmp_dec.as<uint16_t>() + plane * c;
        out[c] = j2k_hip_outplane{p, 2, (ptrdiff_t)cod.width * 2, 16, cod.prec, cod.width, cod.height};
        D.plane[c] = p; D.stride[c] = (long long)cod.width; D.sx[c] = cod.cdx[c]; D.sy[c] = cod.cdy[c];
    }
    const int rc = j2k_hip_decode_device(e, file, len, 1, out, cod.ncomp);
    if (rc != J2K_HIP_OK) throw Error(rc, e->err);
    j2k_hip_plane dplanes[4];
    for (uint32_t c = 0; c < cod.ncomp; ++c) dplanes[c] = planes[c];
    if (!on_device) upload_planes(e, cod, planes, 0, (int)cod.height, dplanes, e->stream);
    reduce(e, src, dplanes, D, diffs, ndiffs);
}

} // namespace

extern "C" {

int j2k_hip_compare_check(const j2k_hip_params *params, const void *file, size_t len)
{
    try {
        (void)checked_header(source_of(params), file, len);
        return J2K_HIP_OK;
    } catch (const Error &x) {
        create_error() = x.what();
        return x.code;
    } catch (const std::exception &x) {
        create_error() = x.what();
        return J2K_HIP_ERR_PARAM;
    }
}

int j2k_hip_compare(j2k_hip_encoder *e, const j2k_hip_params *params, const j2k_hip_plane *planes, const void *file, size_t len,
                    j2k_hip_diff *diffs, uint32_t ndiffs)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    return guarded(e, [&] { compare_file(e, params, planes, false, file, len, diffs, ndiffs); });
}

int j2k_hip_compare_device(j2k_hip_encoder *e, const j2k_hip_params *params, const j2k_hip_plane *planes, const void *file,
                           size_t len, j2k_hip_diff *diffs, uint32_t ndiffs)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    return guarded(e, [&] { compare_file(e, params, planes, true, file, len, diffs, ndiffs); });
}

int j2k_hip_stage_compare(j2k_hip_encoder *e, const j2k_hip_params *params, const j2k_hip_plane *planes_device, const void *d_decoded,
                          j2k_hip_diff *diffs, uint32_t ndiffs)
{
    if (!e) return J2K_HIP_ERR_PARAM;
    return guarded(e, [&] {
        if (e->pend.active) throw Error(J2K_HIP_ERR_PARAM, "an encode is in progress on this handle");
        const Source src = source_of(params);
        check_diffs(src, diffs, ndiffs);
        if (!planes_device) throw Error(J2K_HIP_ERR_PARAM, "planes is NULL");
        if (!d_decoded || reinterpret_cast<uintptr_t>(d_decoded) % 2) throw Error(J2K_HIP_ERR_PARAM, "the decoded planes are NULL or at an odd address");
        HIP_CHECK(hipSetDevice(e->device));
        Decoded D{};
        const uint16_t *p = static_cast<const uint16_t *>(d_decoded);
        for (uint32_t c = 0; c < src.cod.ncomp; ++c) {
            D.plane[c] = p; D.stride[c] = (long long)src.cw[c]; D.sx[c] = D.sy[c] = 1;
            p += (size_t)src.cw[c] * src.ch[c];
        }
        reduce(e, src, planes_device, D, diffs, ndiffs);
    });
}

} // extern "C"
