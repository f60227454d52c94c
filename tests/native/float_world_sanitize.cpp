// The host binding's float worlds (j2k_amd/host: HipCodec and the test hook, FLOAT channels of depth 32) under
// AddressSanitizer + UndefinedBehaviorSanitizer on the CPU.  Built and run by tests/test_float_world_sanitize.py together with
// hip_codec.cpp and host_test_hook.cpp; no HIP, no device: the C ABI is the stand-in below, which checks the channel views it is
// handed (sample_bits 32, depth 16, 4-byte grid), reads or writes every sample through them -- so a wrong base, stride or
// extent is the sanitizer's to find -- and applies the float definition of include/j2k_hip.h.
#include "../../include/j2k_hip.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

struct j2k_hip_encoder { int device; };

static j2k_hip_params g_params;
static unsigned g_promote = 0, g_demote = 0, g_encodes = 0, g_decodes = 0;
static std::vector<unsigned> g_samples; // what the stand-in encode made of the floats, channel by channel

static unsigned promote16(unsigned v) { return (v > 16384u ? ((v - 1u) << 1) + 1u : v << 1) & 0xffffu; }
static unsigned demote16(unsigned v) { return v > 32768u ? ((v - 1) >> 1) + 1 : v >> 1; }
static unsigned quantise(float x, unsigned d, bool promote)
{
    const float t = x > 1.0f ? 1.0f : (x > 0.0f ? x : 0.0f);
    if (promote) return promote16((unsigned)(t * 32768.0f + 0.5f));
    return (unsigned)(t * (float)((1u << d) - 1) + 0.5f);
}
static void check_view(const void *base, ptrdiff_t colbytes, ptrdiff_t rowbytes, uint32_t bits, uint32_t depth)
{
    CHECK(bits == 32 && depth == 16);
    CHECK(base && reinterpret_cast<uintptr_t>(base) % 4 == 0 && colbytes % 4 == 0 && rowbytes % 4 == 0);
}

extern "C" {
int j2k_hip_device_count(void) { return 1; }
int j2k_hip_create(j2k_hip_encoder **enc, int device) { *enc = new j2k_hip_encoder{device}; return J2K_HIP_OK; }
void j2k_hip_destroy(j2k_hip_encoder *enc) { delete enc; }
const char *j2k_hip_last_error(const j2k_hip_encoder *) { return ""; }

int j2k_hip_encode(j2k_hip_encoder *, const j2k_hip_params *p, const j2k_hip_plane *planes, j2k_hip_write_fn write, void *user)
{
    g_params = *p;
    g_promote = p->promote_ae16;
    g_samples.clear();
    for (uint32_t c = 0; c < p->channels; ++c) {
        check_view(planes[c].base, planes[c].colbytes, planes[c].rowbytes, planes[c].sample_bits, planes[c].depth);
        for (uint32_t y = 0; y < p->height; ++y)
            for (uint32_t x = 0; x < p->width; ++x) {
                float f;
                std::memcpy(&f, static_cast<const unsigned char *>(planes[c].base) + (ptrdiff_t)y * planes[c].rowbytes + (ptrdiff_t)x * planes[c].colbytes, 4);
                g_samples.push_back(quantise(f, 16, p->promote_ae16 != 0));
            }
    }
    ++g_encodes;
    static const unsigned char soc[4] = {0xff, 0x4f, 0xff, 0xd9};
    return write(user, soc, 4) == 4 ? J2K_HIP_OK : J2K_HIP_ERR_SINK;
}

static void fill(const j2k_hip_outplane &p, unsigned value, bool demoted)
{
    check_view(p.base, p.colbytes, p.rowbytes, p.sample_bits, p.depth);
    for (uint32_t y = 0; y < p.height; ++y)
        for (uint32_t x = 0; x < p.width; ++x) {
            const unsigned v = (value + 257u * x + 4099u * y) & 0xffffu;
            const float f = demoted ? (float)demote16(v) / 32768.0f : (float)v / 65535.0f;
            std::memcpy(static_cast<unsigned char *>(p.base) + (ptrdiff_t)y * p.rowbytes + (ptrdiff_t)x * p.colbytes, &f, 4);
        }
}

int j2k_hip_rgba_mode(const void *, size_t, uint32_t *mode) { *mode = J2K_HIP_RGBA_RGB; return J2K_HIP_OK; }
int j2k_hip_decode_rgba(j2k_hip_encoder *, const void *, size_t, uint32_t, const j2k_hip_rect *, const j2k_hip_rgba_dst *dst)
{
    CHECK(dst->struct_size == sizeof(*dst));
    g_demote = dst->demote_ae16;
    fill(dst->r, 1000, g_demote != 0); fill(dst->g, 2000, g_demote != 0); fill(dst->b, 3000, g_demote != 0);
    if (dst->a.base) fill(dst->a, 65535, g_demote != 0);
    ++g_decodes;
    return J2K_HIP_OK;
}
int j2k_hip_decode(j2k_hip_encoder *, const void *, size_t, uint32_t, const j2k_hip_outplane *planes, uint32_t nplanes)
{
    for (uint32_t c = 0; c < nplanes; ++c) fill(planes[c], 1000 * (c + 1), false);
    ++g_decodes;
    return J2K_HIP_OK;
}
int j2k_hip_decode_sequence_check(const j2k_hip_file *, uint32_t, uint32_t *) { return J2K_HIP_OK; }
int j2k_hip_decode_sequence(j2k_hip_encoder *, const j2k_hip_file *, uint32_t nframes, uint32_t, const j2k_hip_rect *, const j2k_hip_outplane *planes, uint32_t nplanes)
{
    for (uint32_t k = 0; k < nframes * nplanes; ++k) fill(planes[k], 1000 * (k + 1), false);
    return J2K_HIP_OK;
}
int j2k_hip_read_info(const void *, size_t, j2k_hip_file_info *) { return J2K_HIP_OK; }

// the hook (host_test_hook.cpp)
long j2k_host_test_write(const unsigned char *frame, unsigned width, unsigned height, long rowbytes, int pixel_size, int channels, int depth,
                         int reversible, int ycc, int layers, int tile_size, int honour, long max_write, unsigned char *out, unsigned long out_cap,
                         char *err, unsigned long err_cap);
long j2k_host_test_read_rgba(const unsigned char *file, unsigned long file_len, unsigned subsample, unsigned char *frame, unsigned width,
                             unsigned height, long rowbytes, int pixel_size, int depth, int demote, int with_alpha, char *err, unsigned long err_cap);
long j2k_host_test_read(const unsigned char *file, unsigned long file_len, unsigned subsample, unsigned char *frame, unsigned width,
                        unsigned height, long rowbytes, int pixel_size, int channels, int depth, char *err, unsigned long err_cap);
}

static const unsigned char kFile[16] = {0xff, 0x4f, 0xff, 0x51, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

int main()
{
    char err[256];
    for (unsigned w : {1u, 5u, 33u})
        for (unsigned h : {1u, 4u})
            for (long pad : {0L, 16L, 4L}) {
                const long rowbytes = 16L * w + pad;
                // exactly the world's bytes on the heap: a view that leaves them is an ASan report
                std::vector<unsigned char> world((size_t)rowbytes * h);
                std::vector<float> want;
                for (int promote = 0; promote < 2; ++promote) {
                    for (unsigned y = 0; y < h; ++y)
                        for (unsigned x = 0; x < w; ++x)
                            for (unsigned k = 0; k < 4; ++k) {
                                const float specials[6] = {NAN, INFINITY, -INFINITY, -0.0f, 1.0000001f, 1e-45f};
                                const unsigned i = (y * w + x) * 4 + k;
                                const float f = i % 11 == 0 ? specials[(i / 11) % 6] : (float)((i * 2654435761u) >> 8) / 16777215.0f * 1.1f - 0.05f;
                                std::memcpy(&world[(size_t)y * rowbytes + 16 * x + 4 * k], &f, 4);
                            }
                    if (promote) setenv("J2K_HOST_TEST_PROMOTE", "1", 1); else unsetenv("J2K_HOST_TEST_PROMOTE");
                    for (int channels : {3, 4}) {
                        unsigned char out[16];
                        const long n = j2k_host_test_write(world.data(), w, h, rowbytes, 4, channels, 16, 1, 0, 1, 0, 1, -1, out, sizeof out, err, sizeof err);
                        CHECK(n == 4);
                        CHECK(g_promote == (unsigned)promote && g_params.width == w && g_params.height == h && g_params.channels == (uint32_t)channels);
                        CHECK(g_samples.size() == (size_t)channels * w * h);
                        // codec channel c = R, G, B, A = sample 1, 2, 3, 0 of the pixel
                        for (int c = 0; c < channels; ++c)
                            for (unsigned y = 0; y < h; ++y)
                                for (unsigned x = 0; x < w; ++x) {
                                    float f;
                                    std::memcpy(&f, &world[(size_t)y * rowbytes + 16 * x + 4 * ((c + 1) % 4)], 4);
                                    CHECK(g_samples[((size_t)c * h + y) * w + x] == quantise(f, 16, promote != 0));
                                }
                    }
                }
                unsetenv("J2K_HOST_TEST_PROMOTE");
                // the read side: every float of the world written (or every float but A), nothing else
                for (int demote = 0; demote < 2; ++demote)
                    for (int alpha = 0; alpha < 2; ++alpha) {
                        std::memset(world.data(), 0xa5, world.size());
                        CHECK(j2k_host_test_read_rgba(kFile, sizeof kFile, 1, world.data(), w, h, rowbytes, 4, 32, demote, alpha, err, sizeof err) == 1);
                        CHECK(g_demote == (unsigned)(demote && alpha)); // (the binding demotes a world handed over whole)
                        for (unsigned y = 0; y < h; ++y) {
                            for (unsigned x = 0; x < w; ++x)
                                for (unsigned k = 0; k < 4; ++k) {
                                    float f;
                                    std::memcpy(&f, &world[(size_t)y * rowbytes + 16 * x + 4 * k], 4);
                                    if (k == 0 && !alpha) { unsigned u; std::memcpy(&u, &f, 4); CHECK(u == 0xa5a5a5a5u); }
                                    else CHECK(f >= 0.0f && f <= 1.0f);
                                }
                            for (long b = 16L * w; b < rowbytes; ++b) CHECK(world[(size_t)y * rowbytes + b] == 0xa5);
                        }
                    }
                std::memset(world.data(), 0xa5, world.size());
                CHECK(j2k_host_test_read(kFile, sizeof kFile, 1, world.data(), w, h, rowbytes, 4, 3, 32, err, sizeof err) == 0);
                std::printf("ok %ux%u pad %ld\n", w, h, pad);
            }
    // a FLOAT channel that claims another depth is no 32-bpc world: refused by the binding, no call reaches the library
    {
        std::vector<unsigned char> world(16 * 4 * 2, 0);
        const unsigned before = g_decodes;
        CHECK(j2k_host_test_read_rgba(kFile, sizeof kFile, 1, world.data(), 4, 2, 64, 4, 16, 0, 1, err, sizeof err) == -1);
        CHECK(g_decodes == before);
        std::printf("ok refusal\n");
    }
    return 0;
}
