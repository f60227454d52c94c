// handle.h -- the codec handle (j2k_hip_encoder of include/j2k_hip.h) and the small helpers its users share:
// encoder.cpp (encode path, lifetime), stage_hooks.cpp (the encode kernels' stage hooks) and decoder.cpp (decode path).
// Internal to libj2k_hip.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstdlib>
#include <future>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "bands.h"
#include "common.h"
#include "geometry.h"
#include "kernels.h"
#include "table_layout.h"

namespace j2k_hip {

#define HIP_CHECK(expr)                                                                             \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            throw Error(J2K_HIP_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));     \
    } while (0)

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); } // whatever j2k_hip_destroy's list forgets is still freed with the handle
    void ensure(size_t n)
    {
        if (n <= cap) return;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        const size_t want = n + n / 8 + 4096;
        if (hipMalloc(&p, want) != hipSuccess) {
            p = nullptr;
            throw Error(J2K_HIP_ERR_MEMORY, "hipMalloc of " + std::to_string(want) + " bytes failed");
        }
        cap = want;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};

struct PinnedBuf {
    void *p = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() { release(); }
    void ensure(size_t n)
    {
        if (n <= cap) return;
        if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
        const size_t want = n + n / 8 + 4096;
        if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) {
            p = nullptr;
            throw Error(J2K_HIP_ERR_MEMORY, "hipHostMalloc of " + std::to_string(want) + " bytes failed");
        }
        cap = want;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
    template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};

static_assert(kMaxPasses == kDevMaxPasses, "table_layout.h and the Tier-1 kernels agree on the passes per block");

// host threads of a Tier-2 planner (encode: the packet headers of a big frame; decode: the packets of a file)
inline unsigned plan_threads() { return std::max(1u, std::min(4u, std::thread::hardware_concurrency())); }

// the HIP runtime's number of hardware queues (its own environment knob GPU_MAX_HW_QUEUES, read once; 4 unless the host raised
// it): streams beyond it share queues and wait for each other
inline int hw_queues()
{
    static const int q = [] {
        const char *v = std::getenv("GPU_MAX_HW_QUEUES");
        const int n = v ? std::atoi(v) : 0;
        return n > 0 ? n : 4;
    }();
    return q;
}

inline double now_ms()
{
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

enum { EV_START, EV_UPLOAD, EV_FRONT, EV_DWT, EV_T1, EV_GATHER, EV_DONE, EV_COUNT };

constexpr int kMaxLevels = 33;


} // namespace j2k_hip

// what encode_begin leaves for encode_end
struct Pending {
    bool active = false;
    double t_begin = 0;
    size_t F = 1, nb1 = 0;
    bool framed = true, rate_control = false;
    bool rc_device = false;   // rate control: the per-block work was queued on the device behind the coder (rate.hip)
    bool rc_layers = false;   // layers at given slopes: rate_layers_kernel was queued behind the coder, its counts are on their way to h_rc_layers
    bool budget_host_cut = false; // a call to a byte budget under rate_dev = -1: the pass tables are on their way to h_passes for the final cut
    bool rc_tables_pending = false; // ... and the pass tables are coming down on a side stream: wait for rc_tables before reading h_passes
    double dwt_bytes = 0;
    uint32_t *meta = nullptr;
    const j2k_hip::CblkDev *dblk = nullptr;
    int nl = 0;
    // band-pipelined encode (bands.h): the frame came up in `stages` row bands, every stage's Tier-1 runs on its own coder stream
    bool banded = false;
    int stages = 0, bands = 0;
    double ms_upload_host = 0, t_uploaded = 0; // host time spent in the band uploads; when the last band had left the caller's buffer
};

struct j2k_hip_encoder {
    int device = 0;
    Pending pend;
    // j2k_hip_encode_begin_borrowed: the upload and the launches of the pending frame run on a thread of their own
    std::future<int> begin_job;
    std::atomic<bool> begin_async{false};
    j2k_hip_params begin_params = {};
    j2k_hip_plane begin_planes[4] = {};
    bool last_fused = false;
    j2k_hip::FrontendArgs last_fa = {};   // of the last call's first frame (j2k_hip_debug_dwt_time replays its DWT launches)
    hipStream_t stream = nullptr;
    hipStream_t mqs[12] = {};      // MQ coder streams (run beside the context modeller); a band-pipelined call: one per stage
    hipEvent_t gev[12] = {};
    hipEvent_t mq_done[12] = {};
    hipEvent_t gates_zeroed = nullptr; // band-pipelined call: the gate counters are zero (the gated coder launch may be queued)
    hipEvent_t rc_fixed = nullptr, rc_tables = nullptr; // rate control on the device: pass tables final on the device / copied to the host (side stream)
    hipEvent_t k1_done = nullptr;
    bool dwt_word_ref = false;
    bool counted_inflight = false;
    std::string err;
    hipEvent_t ev[j2k_hip::EV_COUNT] = {};
    hipEvent_t lev[j2k_hip::kMaxLevels + 1] = {};
    int last_levels = 0;
    double level_ms[j2k_hip::kMaxLevels] = {};
    j2k_hip_stats stats = {};
    uint32_t last_guard = 0; // guard bits of the last file written (j2k_hip_encode_get_guard_bits); 0 before any

    j2k_hip::DevBuf in, P, Q, Z, blks, jobs, sym, out, meta, passes, cs, plan;
    std::vector<std::unique_ptr<j2k_hip::DevBuf>> seq_in; // j2k_hip_encode_sequence_budget: an input arena per host frame of the call
    std::unique_ptr<j2k_hip::Workers> t2_workers; // host threads of the Tier-2 planner (created with the first big frame)
    std::unique_ptr<j2k_hip::Workers> alloc_workers; // host threads of the layer allocation (rate control), kept from frame to frame
    j2k_hip::PinnedBuf h_meta, h_cs, h_plan, h_passes;
    // rate control on the device (rate.hip): the blocks' weights (per geometry), distortions, bounds; `rc_small` holds the passes
    // of earlier layers, the thresholds ahead with their sums, and a scan's results, mirrored in pinned host memory
    j2k_hip::DevBuf rc_weight, rc_disto, rc_reach, rc_bounds, rc_small;
    j2k_hip::PinnedBuf h_rc_bounds, h_rc_small;
    bool rc_weight_valid = false;
    // layers at given slopes (rate_layers_kernel): per block and layer a pass count and a byte count, [nb * L] bytes then [nb * L] words
    j2k_hip::DevBuf rc_layers;
    j2k_hip::PinnedBuf h_rc_layers;
    // the thresholds the layers of the last file's tiles were laid out at (j2k_hip_encode_get_layer_slopes): [tile][layer] of
    // tiles [last_slopes_first, ..); empty before any file under rate control
    std::vector<double> last_slopes;
    uint32_t last_slopes_first = 0, last_slopes_layers = 0;

    // cached geometry (host + device images)
    bool geo_valid = false;
    j2k_hip::Coding geo_cod;
    uint32_t geo_first = 0, geo_count = 0;
    j2k_hip::Geometry geo;
    std::vector<j2k_hip::CblkDev> h_blks;
    std::vector<j2k_hip::CblkDev> h_blks_seq;         // block table of a frame sequence (frames x blocks)
    j2k_hip::DevBuf blks_seq;
    size_t seq_frames = 0;
    bool seq_valid = false;
    std::vector<std::vector<j2k_hip::DwtJob>> h_jobs; // per level
    std::vector<j2k_hip::DwtJob> h_fused_jobs;        // level 1 fused with the front end: one job per tile
    size_t fused_jobs_pos = 0;
    std::vector<int> lvl_max_rw, lvl_max_rh;
    size_t sym_bytes = 0, out_bytes = 0;
    // working planes cover the bounding box of the requested tiles only (a tile-sharded rank pays for its
    // share of the image, not for the whole image): box origin in image coordinates, row stride and plane size in words
    int box_x0 = 0, box_y0 = 0;
    size_t stride = 0, plane_elems = 0;
    // component c's working plane starts comp_off[c] words into a frame's planes and has the rows of its own grid (sub-sampled
    // components: fewer); frame_elems words hold all of them.  Without sub-sampling: c * plane_elems, ncomp * plane_elems.
    size_t comp_off[4] = {0, 0, 0, 0}, frame_elems = 0;
    // band-pipelined encode (bands.h).  Streams: the row bands' H2D, the stages' D2H; events: band k has arrived, stage k's
    // coder + packing + results are through, stage k's codewords are in host memory
    static constexpr int kMaxBands = 8, kMaxStages = kMaxBands + 2; // (a coder stream per stage: mqs[]; the last band's blocks are up to three stages)
    hipStream_t up_stream = nullptr, dl_stream = nullptr; // the device's copy stream (encoder.cpp, DeviceShared): the bands' upload, then the stages' packing
    // gated coding (kernels.h, T1Args::gate_*): the coder workgroups of the frame (<= 64 blocks of one stage each), the group of
    // every block, and the per-call counters: blocks modelled per group, workgroups finished per stage, the abort word
    std::vector<j2k_hip::T1Args::GateGroup> h_gate_groups;
    std::vector<uint32_t> h_group_of, stage_group_first, stage_group_count;
    j2k_hip::DevBuf gate_groups, gate_group_of, gate_state; // gate_state: [groups] ready | [stages] done | abort
    hipEvent_t band_up[kMaxBands] = {}, stage_done[kMaxStages] = {}, stage_dl[kMaxStages] = {};
    bool band_valid = false;              // the schedule below belongs to `geo` and band_row_end
    std::vector<int> band_row_end;
    j2k_hip::BandSchedule band;
    std::vector<j2k_hip::CblkDev> h_blks_band; // the block table stage-major
    j2k_hip::DevBuf blks_band, pack_dst;  // its device image; per block: where its codeword goes in the packing arena (cs)
    j2k_hip::PinnedBuf h_stage_cs[kMaxStages]; // a stage's packed codewords on the host
    std::vector<std::vector<uint32_t>> job_row_first; // per level: first job of every tile row (+ one past the last)
    std::vector<uint32_t> fused_row_first;            // the same for the fused level-1 jobs (one per tile)
    std::vector<uint8_t> bounce;          // small pieces of the file are handed to the sink in larger writes
    // decode path (decoder.cpp): the file on the device, per-block codeword arena, bit-plane masks, block table, output staging
    j2k_hip::DevBuf d_file, d_cw, d_masks, d_dblk, d_segs, d_outimg;
    j2k_hip::PinnedBuf h_outimg, h_dtab;
    uint64_t dec_lane_blocks = 0, dec_wave_blocks = 0; // of the last decode call: blocks the lane kernel took / the wave kernel
    uint64_t dec_passes = 0, dec_cw_bytes = 0;         // ... and the coding passes and codeword bytes handed to Tier-1
    uint32_t dec_max_layers = 0; // j2k_hip_decode_set_max_layers: every decode call keeps the first so many quality layers (0: all)
    // compare (compare.cpp): the decoded components as dense 16-bit planes, the accumulators, and their host image
    j2k_hip::DevBuf cmp_dec, cmp_acc;
    j2k_hip::PinnedBuf h_cmp;
    // cinema colour (rgb_to_xyz; xyz_tables.h): the tables a frame needs, uploaded on first use and kept with the handle --
    // linear light by (source, sample depth), thresholds by destination depth (source = 0).  `host` stays alive while its
    // upload may still be in flight.
    struct XyzTable { uint32_t source, depth; std::vector<float> host; j2k_hip::DevBuf dev; };
    std::vector<std::unique_ptr<XyzTable>> xyz_tables;
    // ... and the way back in the decode's RGBA output stage (j2k_hip_decode_set_xyz_to_rgb): the setting, and its tables, kept
    // alike -- thresholds by (target, destination depth), code -> linear light by component depth (source = 0: it is the same
    // for every target).  Both are padded to max(2^depth, 4) words, the thresholds with +infinity.
    uint32_t dec_xyz_to_rgb = 0;
    std::vector<std::unique_ptr<XyzTable>> xyz_inverse_tables;
};

namespace j2k_hip {

// The front end's host side (encoder.cpp), shared with the compare calls (compare.cpp), which make the encode's source samples:
// the working planes of one frame over a box of the reference grid ...
struct PlaneLayout { size_t stride, comp_off[4], frame_elems; int cbx0[4], cby0[4], cw[4], ch[4]; };
PlaneLayout plane_layout(const Coding &cod, int bx0, int by0, int bx1, int by1);
// ... FrontendArgs from channel views whose `base` pointers are device pointers (checks the views) ...
FrontendArgs make_frontend_args(const Coding &cod, const j2k_hip_plane *planes, int x0, int y0, int x1, int y1);
// ... the stand-alone front end of one frame into planes of row stride S words, component c at dst + comp_off[c] ...
// (rgb_to_xyz: the handle's tables, uploaded on s ahead of the launch where they are new)
void run_frontend(j2k_hip_encoder *e, const Coding &cod, FrontendArgs fa, int32_t *dst, const size_t comp_off[4], size_t S, hipStream_t s);
// ... and a host frame's rows [y0, y1) into the handle's input arena, queued on s: dplanes[c].base = the device copy of planes[c]'s
void upload_planes(j2k_hip_encoder *e, const Coding &cod, const j2k_hip_plane *planes, int y0, int y1, j2k_hip_plane dplanes[4], hipStream_t s);

// What an encode and the stage hooks of its kernels (stage_hooks.cpp) share, defined in encoder.cpp:
// geometry, code-block table and DWT job lists of the handle, built or reused, with their device images ...
void prepare_geometry(j2k_hip_encoder *e, const Coding &cod, uint32_t tile_first, uint32_t tile_count);
// ... the decision-stream and codeword capacities of a code-block ...
struct CblkCaps { size_t sym, out; };
CblkCaps cblk_capacities(size_t area, uint32_t Mb, uint32_t style);
// ... whether level 1 of the DWT takes its samples straight from the frame, and the launch arguments of DWT level l of frame f ...
bool fuse_frontend(const Coding &cod, const FrontendArgs &fa, const Tuning &tn);
DwtLevelArgs dwt_level_args(j2k_hip_encoder *e, const Coding &cod, const FrontendArgs &fa, bool fused, size_t f, int l, int tile_row = -1);
#ifdef J2K_T1_COUNTERS
void t1_counters(T1Args &ta);
#endif
// T1Args has a member more in a J2K_T1_COUNTERS / J2K_MQ_TIMES build (kernels.h), so the files that fill one must be built
// alike.  Each refers to a tag named after its layout (through t1_arena_args) and encoder.cpp defines its own: a library
// whose encoder.cpp and stage_hooks.cpp disagree does not link.  (The kernels' side is the build recipe's: tools/README.md.)
#if defined(J2K_T1_COUNTERS) || defined(J2K_MQ_TIMES)
#define J2K_T1ARGS_LAYOUT_TAG t1args_layout_with_dbg
#else
#define J2K_T1ARGS_LAYOUT_TAG t1args_layout_plain
#endif
extern const char J2K_T1ARGS_LAYOUT_TAG __attribute__((visibility("hidden")));
// ... and where the Tier-1 kernels read and write in the handle's arenas: decisions, codewords, and the result tables of t.nb blocks
inline void t1_arena_args(const j2k_hip_encoder *e, const T1Tables &t, T1Args &ta)
{
    asm volatile("" : : "r"(&J2K_T1ARGS_LAYOUT_TAG)); // (the reference to the tag: an address in a register)
    ta.sym = e->sym.as<uint8_t>(); ta.out = e->out.as<uint8_t>();
    t.fill(ta, e->meta.as<uint32_t>(), e->passes.as<uint32_t>());
}
// The tables an encode keeps from call to call (geometry, sequence and band block tables, rate weights) are rebuilt by the next
// one: for every stage hook that overwrites an arena of the handle.
inline void invalidate_cached_tables(j2k_hip_encoder *e) { e->geo_valid = e->seq_valid = e->band_valid = e->rc_weight_valid = false; }

// After a failure nothing of a handle may stay in flight (the next call reuses every arena): waits for its streams.
void drain(j2k_hip_encoder *e);
// stream i of the handle's side streams (encode: the MQ coder groups; decode: the tail of the Tier-1 decode), created on first use
hipStream_t coder_stream(j2k_hip_encoder *e, int i);
// j2k_hip_encode_begin_borrowed: between it and its _end the handle belongs to the deferred half's thread.  Every other
// call is refused BEFORE it touches the handle (no drain, no error text written beside the worker): the refusal is
// remembered per calling thread and j2k_hip_last_error answers it.
bool begin_worker_thread();
const j2k_hip_encoder *&refused_handle();
// ... with a text of the refused call's own where it has one (null: the general text); a static string, per calling thread
const char *&refused_text();
// text of the last failure of a call without a handle (j2k_hip_create, header-only entry points), per thread
std::string &create_error();

// Runs f(), turning every exception into a status code + the handle's error text: nothing is thrown across the C ABI.
template <typename F> int guarded(j2k_hip_encoder *e, F &&f)
{
    if (e && e->begin_async.load() && !begin_worker_thread()) { refused_handle() = e; refused_text() = nullptr; return J2K_HIP_ERR_PARAM; }
    refused_handle() = nullptr;
    try {
        f();
        if (e) e->err.clear();
        return J2K_HIP_OK;
    } catch (const Error &x) {
        drain(e);
        if (e) e->err = x.what();
        return x.code;
    } catch (const std::bad_alloc &) {
        drain(e);
        if (e) e->err = "out of host memory";
        return J2K_HIP_ERR_MEMORY;
    } catch (const std::exception &x) {
        drain(e);
        if (e) e->err = x.what();
        return J2K_HIP_ERR_PARAM;
    } catch (...) {
        drain(e);
        if (e) e->err = "unknown error";
        return J2K_HIP_ERR_PARAM;
    }
}

} // namespace j2k_hip
