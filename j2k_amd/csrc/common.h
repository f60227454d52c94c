// common.h -- shared host-side definitions of libj2k_hip (no HIP types here).
//
// `Coding` is the normalised form of j2k_hip_params: the coding parameters that the reference's
// encode entry point fixes (reference: src/common/j2k_openjpeg_codec.cpp:627-719).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/j2k_hip.h"

namespace j2k_hip {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

constexpr int kFracBits = 6;     // T1 fractional bits below bit-plane 0 (T1_NMSEDEC_FRACBITS)
constexpr int kGuardBits = 2;    // QCD guard bits unless the parameters say otherwise (Coding::guard)
constexpr int kMaxGuardBits = 7; // ... and the most the three bits of Sqcd hold
constexpr int kMaxPasses = 96;   // 3*Mb-2 with Mb <= 32
constexpr int kMaxBitplanes = 30; // the most bit-planes the reader takes in a code-block (decode_plan.cpp; libopenjp2's limit)

// A code-block has more bit-planes than its sub-band signals: the J2K_HIP_ERR_OVERFLOW of a frame beyond its guard bits, thrown
// by host Tier-2 where it meets a negative zero-bit-plane count.  A type of its own so that a caller under J2K_HIP_GUARD_AUTO
// can tell it from every other overflow and plan the frame again with the guard bits it needs.
struct GuardExcess : Error {
    GuardExcess() : Error(J2K_HIP_ERR_OVERFLOW, "code-block has more bit-planes than its sub-band signals (guard bits exceeded)") {}
};

// struct_size of j2k_hip_params before guard_bits was appended: such a caller passes guard_bits 0
constexpr size_t kParamsSizeBeforeGuardBits = offsetof(j2k_hip_params, guard_bits);
// ... and before layer_slopes was: guard_bits and the padding behind it (the struct is pointer-aligned), layer_slopes NULL
constexpr size_t kParamsSizeBeforeLayerSlopes = offsetof(j2k_hip_params, layer_slopes);
inline bool params_size_ok(const j2k_hip_params *p)
{
    return p->struct_size == sizeof(j2k_hip_params) || p->struct_size == kParamsSizeBeforeLayerSlopes || p->struct_size == kParamsSizeBeforeGuardBits;
}
inline bool params_has_guard_bits(const j2k_hip_params *p) { return p->struct_size >= kParamsSizeBeforeLayerSlopes; }
inline const double *params_layer_slopes(const j2k_hip_params *p) { return p->struct_size == sizeof(j2k_hip_params) ? p->layer_slopes : nullptr; }
// the caller's struct widened to this library's layout (what lies beyond its struct_size is not read)
inline j2k_hip_params widened(const j2k_hip_params *p)
{
    j2k_hip_params q = {};
    std::memcpy(&q, p, p->struct_size); // (one of the three sizes params_size_ok takes)
    q.struct_size = sizeof q;
    return q;
}
constexpr int kPrecinctExp = 15; // maximal precincts (PPx = PPy = 15): the default, no SPcod precinct bytes

struct Coding {
    uint32_t width = 0, height = 0, ncomp = 0, prec = 0; // width / height: the image area's size (Xsiz - XOsiz, Ysiz - YOsiz)
    // origin of the image area and of the tile grid on the reference grid (SIZ XOsiz/YOsiz, XTOsiz/YTOsiz): 0 for everything the
    // encode path writes (reference: j2k_openjpeg_codec.cpp:667-670, :712-719), any value on the decode path
    uint32_t img_x0 = 0, img_y0 = 0, tile_x0 = 0, tile_y0 = 0;
    bool reversible = true, mct = false, promote = false;
    uint32_t layers = 1, numres = 6, cbw = 6, cbh = 6; // cbw/cbh = log2 of the code-block size
    uint32_t prog = 0;                                 // progression order (J2K_HIP_LRCP ..)
    // digital cinema profile (encode): Rsiz 3 / 4, tile-parts per component, TLM, the 4K progression order change; the cap per component
    uint32_t dci = 0, max_comp_size = 0;
    // code-block style (COD SPcod; cblk_style.h): encode 0 or bypass / reset / termall / pterm / segsym in any combination
    uint32_t cblk_style = 0;
    // encode: the planes are R, G, B[, A] of the full image and the front end makes Y, Cb, Cr[, A] at the components' own sizes
    bool rgb_to_sycc = false;
    // encode: channels 0..2 are R'G'B' and the front end makes cinema X'Y'Z' code values of them (0 = off; 1 sRGB, 2 Rec.709 under
    // a 2.4 power, 3 linear Rec.709; xyz_tables.h)
    uint32_t rgb_to_xyz = 0;
    // encode: QCD guard bits (every band signals expn + guard - 1 bit-planes).  guard_auto: `guard` is the floor, and a frame whose
    // blocks outgrow it is planned again with the smallest count that holds them (j2k_hip_params.guard_bits)
    uint32_t guard = kGuardBits;
    bool guard_auto = false;
    uint32_t dci_tileparts() const { return dci == 4 ? 6u : (dci == 3 ? 3u : 1u); }
    // per component: sub-sampling factors on the reference grid (decode: whatever SIZ holds; encode: comp_sub_x / _y, 1, 2 or 4, the
    // reference's own encode call never sub-samples), and -- decode only, the encode path writes one unsigned depth -- precision, signedness
    // (kMaxComps entries: a codestream read may hold more than the four components the plug-in's Buffer has channels for -- the
    //  reference then takes the first four, j2k_openjpeg_codec.cpp:278, :530 -- and Tier-2 has to walk the packets of all of them)
    static constexpr uint32_t kMaxComps = 16;
    uint8_t cdx[kMaxComps] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1}, cdy[kMaxComps] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
    uint8_t cprec[kMaxComps] = {}, csgnd[kMaxComps] = {};
    uint32_t ncomp_out() const { return ncomp < 4 ? ncomp : 4; } // components that are decoded / delivered
    bool subsampled() const { for (uint32_t c = 0; c < kMaxComps; ++c) if (cdx[c] != 1 || cdy[c] != 1) return true; return false; }
    // precinct exponents per resolution (index = resolution, 0 = lowest): 15 = maximal (no SPcod precinct bytes)
    bool user_precincts = false;
    uint8_t ppx[33] = {15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15};
    uint8_t ppy[33] = {15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15};
    uint32_t tile_w = 0, tile_h = 0;                   // always > 0 after normalisation
    uint32_t ntx = 1, nty = 1;
    std::string comment;
    bool has_comment = false;
    std::vector<float> rates;      // rate control: one compression ratio per layer (empty = no target)
    std::vector<float> psnr;       // fixed quality: one PSNR target (dB) per layer (empty = none); excludes rates
    std::vector<double> slopes;    // given slope thresholds: one per layer (empty = none; negative: everything left); excludes both
    bool rate_control() const
    {
        if (!slopes.empty()) return true;
        for (float r : rates) if (r > 1.0f) return true;
        for (float q : psnr) if (q > 0.0f) return true;
        return false;
    }
    // file wrapper (jp2.h): raw codestream unless jp2
    bool jp2 = false;
    uint32_t color_space = 0;      // OPJ_COLOR_SPACE numbering (0 unspecified, 1 sRGB, 2 grey, 3 sYCC, 4 e-YCC, 5 CMYK)
    int alpha_channel = -1;        // channel flagged as opacity in the cdef box
    bool alpha_premultiplied = false;
    std::vector<uint8_t> icc;      // restricted ICC profile for the colr box
    uint32_t aspect_num = 0, aspect_den = 0; // pixel aspect (width : height of a pixel); 0 = unknown / square
    float dpi = 0;                 // vertical resolution; 0 = unknown

    uint32_t levels() const { return numres - 1; }
    uint32_t ntiles() const { return ntx * nty; }
};

// Validates exactly what the reference path would reject (OpenJPEG setup/validation errors) plus
// the limits of this implementation; throws Error(J2K_HIP_ERR_PARAM, ...).
Coding normalise(const j2k_hip_params *p);
// Why `guard` guard bits cannot be written for these parameters (null: they can)
const char *guard_bits_refusal(const Coding &c, uint32_t guard);
// The tile-sharded entry points do not write sub-sampled components (a tile range whose origin is no multiple of the factors):
// throws Error(J2K_HIP_ERR_PARAM, ...) for such parameters.  Host code: called before any device work.
void refuse_subsampled_tiles(const Coding &cod);

// The sample type of a channel view (j2k_hip_plane, j2k_hip_outplane; include/j2k_hip.h): 8- and 16-bit unsigned integers
// holding `depth` significant bits, or 32-bit floats of nominal range 0..1 that stand for integers of `depth` (1..16) bits and
// lie at multiples of 4 bytes.  Throws Error(J2K_HIP_ERR_PARAM, ...).  Host code: called before any device work.
inline void check_sample_type(uint32_t sample_bits, uint32_t depth, const void *base, ptrdiff_t colbytes, ptrdiff_t rowbytes)
{
    if (sample_bits != 8 && sample_bits != 16 && sample_bits != 32) throw Error(J2K_HIP_ERR_PARAM, "sample_bits must be 8, 16 or 32");
    if (sample_bits == 32) {
        if (depth < 1 || depth > 16) throw Error(J2K_HIP_ERR_PARAM, "a float channel stands for an integer depth of 1..16");
        if (reinterpret_cast<uintptr_t>(base) % 4 || colbytes % 4 || rowbytes % 4)
            throw Error(J2K_HIP_ERR_PARAM, "a float channel's base, colbytes and rowbytes must be multiples of 4");
    } else if (depth < 1 || depth > sample_bits) throw Error(J2K_HIP_ERR_PARAM, "channel depth does not fit its sample type");
}

// A handful of worker threads that run the same function on slices 0..n-1 (host-side loops over all
// code-blocks of a large tile; starting threads per loop would cost more than the loops).
class Workers {
  public:
    explicit Workers(unsigned n);
    ~Workers();
    unsigned size() const { return n_; }
    // runs fn(i) for i in [0, count) (count <= size()), fn(0) on the calling thread; returns when all are done
    void run(unsigned count, const std::function<void(unsigned)> &fn);

  private:
    struct Impl;
    Impl *impl_;
    unsigned n_;
};

inline int ceildivpow2(int a, int b) { return (int)(((int64_t)a + ((int64_t)1 << b) - 1) >> b); }
inline int floordivpow2(int a, int b) { return a >> b; }
inline int floorlog2(uint32_t a) { int l = 0; while (a > 1) { a >>= 1; ++l; } return l; }

} // namespace j2k_hip
