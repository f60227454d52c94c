// rate_device.h -- rate control on the device (rate.hip; rate_control.h: RateDevice): the layout of the handle's rate arenas, the
// launch arguments over them, and the bisection's calls into the device.  One definition for an encode (encoder.cpp) and for the
// rate stage hook (stage_hooks.cpp).  Internal to libj2k_hip.
#pragma once

#include <cstdio>
#include <cstring>

#include "handle.h"
#include "rate_block.h"
#include "rate_control.h"

namespace j2k_hip {

// rc_small, device and pinned host alike: [done nb][ahead 128 doubles][delta 4 x 128 x 8][three slots of scan results]
struct RcLayout {
    // a scan's results, three slots of them: [sums kRateSums x 8][bytes nb x 4][taken nb x 16]
    size_t done, ahead, delta, slot0, slot_bytes, slot_taken, slot_stride, total;
    explicit RcLayout(size_t nb)
    {
        done = 0;
        ahead = round_up(nb, 256);
        delta = ahead + 128 * sizeof(double);
        slot0 = delta + 4 * 128 * sizeof(long long);
        slot_bytes = kRateSums * sizeof(uint64_t);
        slot_taken = slot_bytes + round_up(nb * sizeof(uint32_t), 256);
        slot_stride = round_up(slot_taken + nb * sizeof(Taken), 256);
        total = slot0 + 3 * slot_stride;
    }
    size_t slot(int k) const { return slot0 + (size_t)k * slot_stride; }
};

// The rate kernels' arguments over the Tier-1 results of t.nb blocks in the handle's `meta` and `passes` arenas; sizes the rate arenas.
inline RateArgs rate_args(j2k_hip_encoder *e, const T1Tables &t)
{
    const uint32_t *meta = e->meta.as<uint32_t>();
    const size_t nb = t.nb;
    const RcLayout lay(nb);
    e->rc_weight.ensure(nb * sizeof(double) + nb); // (the blocks' components behind their weights)
    e->rc_disto.ensure(nb * kDevMaxPasses * sizeof(double));
    e->rc_reach.ensure(nb * kDevMaxPasses * sizeof(float));
    e->rc_bounds.ensure(3 * nb * sizeof(double));
    e->rc_small.ensure(lay.total);
    e->h_rc_bounds.ensure(3 * nb * sizeof(double));
    e->h_rc_small.ensure(lay.total);
    RateArgs a = {};
    a.nblks = (unsigned)nb;
    a.weight = e->rc_weight.as<double>();
    a.comp_of = e->rc_weight.as<unsigned char>() + nb * sizeof(double);
    a.numbps = t.numbps(meta); a.npasses = t.npasses(meta);
    a.pass_nmsedec = reinterpret_cast<const int *>(t.pass_nmsedec(e->passes.as<uint32_t>())); a.pass_rate = t.pass_rate(e->passes.as<uint32_t>());
    a.disto = e->rc_disto.as<double>(); a.reach = e->rc_reach.as<float>(); a.bounds = e->rc_bounds.as<double>();
    uint8_t *sm = e->rc_small.as<uint8_t>();
    a.done = sm + lay.done;
    a.ahead = reinterpret_cast<const double *>(sm + lay.ahead);
    a.delta = reinterpret_cast<long long *>(sm + lay.delta);
    a.scan_sums = nullptr; a.scan_bytes = nullptr; a.scan_taken = nullptr; // (per launch: one of the slots)
    return a;
}

// The bisection's calls into the device, one round trip each on the handle's stream (the prepare kernel and the copy of the
// bounds were queued behind the coder by encode_begin and are through when encode_end has waited for the stream).
struct HipRateDevice : RateDevice {
    j2k_hip_encoder *e;
    size_t nb;
    RcLayout lay;
    RateArgs a;
    hipStream_t s;
    uint8_t *hs, *ds;
    HipRateDevice(j2k_hip_encoder *enc, const T1Tables &t)
        : e(enc), nb(t.nb), lay(t.nb), a(rate_args(enc, t)), s(enc->stream), hs(enc->h_rc_small.as<uint8_t>()), ds(enc->rc_small.as<uint8_t>())
    {
    }
    const double *bmin() override { return e->h_rc_bounds.as<double>(); }
    const double *bmax() override { return e->h_rc_bounds.as<double>() + nb; }
    const double *steepest() override { return e->h_rc_bounds.as<double>() + 2 * nb; }
    void begin_layer(uint32_t first, uint32_t count, const uint8_t *done) override
    {
        if (!done) { HIP_CHECK(hipMemsetAsync(ds + lay.done + first, 0, count, s)); return; }
        std::memcpy(hs + lay.done + first, done, count);
        HIP_CHECK(hipMemcpyAsync(ds + lay.done + first, hs + lay.done + first, count, hipMemcpyHostToDevice, s));
    }
    const bool trace = std::getenv("J2K_RATE_TRACE") != nullptr; // each round trip's time to stderr
    struct Trace {
        const char *what; bool on; double t0;
        Trace(const char *w, bool o) : what(w), on(o), t0(o ? now_ms() : 0) {}
        ~Trace() { if (on) std::fprintf(stderr, "rate device: %s %.3f ms\n", what, now_ms() - t0); }
    };
    void ahead(uint32_t first, uint32_t count, const double *ah, uint32_t K, uint64_t *body) override
    {
        Trace tr("ahead", trace);
        if (K > 128) throw Error(J2K_HIP_ERR_PARAM, "internal: more than 128 thresholds ahead");
        std::memcpy(hs + lay.ahead, ah, K * sizeof(double));
        HIP_CHECK(hipMemcpyAsync(ds + lay.ahead, hs + lay.ahead, K * sizeof(double), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemsetAsync(ds + lay.delta, 0, 4 * 128 * sizeof(long long), s));
        launch_rate_ahead(a, first, count, K, s);
        HIP_CHECK(hipMemcpyAsync(hs + lay.delta, ds + lay.delta, 4 * 128 * sizeof(long long), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        const long long *d = reinterpret_cast<const long long *>(hs + lay.delta);
        for (uint32_t c = 0; c < 4; ++c) {
            long long run = 0;
            for (uint32_t k = 0; k < K; ++k) { run += d[c * 128 + k]; body[(size_t)c * K + k] = (uint64_t)run; }
        }
    }
    void launch_into(int k, uint32_t first, uint32_t count, double thresh)
    {
        RateArgs r = a;
        uint8_t *d = ds + lay.slot(k);
        r.scan_sums = reinterpret_cast<unsigned long long *>(d);
        r.scan_bytes = reinterpret_cast<unsigned *>(d + lay.slot_bytes);
        r.scan_taken = reinterpret_cast<Taken *>(d + lay.slot_taken);
        HIP_CHECK(hipMemsetAsync(d, 0, kRateSums * sizeof(uint64_t), s));
        launch_rate_scan(r, first, count, thresh, s);
    }
    void scan(uint32_t first, uint32_t count, double thresh, const Taken **taken, const uint32_t **bytes, uint64_t *sums) override
    {
        Trace tr("scan", trace);
        launch_into(0, first, count, thresh);
        // (the sums and the two result arrays lie back to back but for padding: one copy)
        HIP_CHECK(hipMemcpyAsync(hs + lay.slot(0), ds + lay.slot(0), lay.slot_taken + (size_t)count * sizeof(Taken), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        std::memcpy(sums, hs + lay.slot(0), kRateSums * sizeof(uint64_t));
        *bytes = reinterpret_cast<const uint32_t *>(hs + lay.slot(0) + lay.slot_bytes);
        *taken = reinterpret_cast<const Taken *>(hs + lay.slot(0) + lay.slot_taken);
    }
    void scan_sums(uint32_t first, uint32_t count, double thresh, int slot, uint64_t *sums) override
    {
        Trace tr("scan, sums only", trace);
        launch_into(slot, first, count, thresh);
        HIP_CHECK(hipMemcpyAsync(hs + lay.slot(slot), ds + lay.slot(slot), kRateSums * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        std::memcpy(sums, hs + lay.slot(slot), kRateSums * sizeof(uint64_t));
    }
    void fetch(int slot, uint32_t count, const Taken **taken, const uint32_t **bytes) override
    {
        Trace tr("fetch", trace);
        HIP_CHECK(hipMemcpyAsync(hs + lay.slot(slot) + lay.slot_bytes, ds + lay.slot(slot) + lay.slot_bytes,
                                 (lay.slot_taken - lay.slot_bytes) + (size_t)count * sizeof(Taken), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        *bytes = reinterpret_cast<const uint32_t *>(hs + lay.slot(slot) + lay.slot_bytes);
        *taken = reinterpret_cast<const Taken *>(hs + lay.slot(slot) + lay.slot_taken);
    }
    uint32_t min_scan() const override { return (uint32_t)(tuning().rate_dev_scan == 0 ? 512 : std::max(1, tuning().rate_dev_scan)); }
    void need_tables() override
    {
        if (!e->pend.rc_tables_pending) return;
        Trace tr("wait for the pass tables", trace);
        HIP_CHECK(hipEventSynchronize(e->rc_tables));
        e->pend.rc_tables_pending = false;
    }
};

} // namespace j2k_hip
