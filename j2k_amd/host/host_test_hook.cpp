// host_test_hook.cpp -- C entry points that let the Python tests drive the C++ codec interface the
// way the plug-in does: build the After Effects channel views like WorldToBuffer
// (reference: src/aftereffects/j2k.cpp:324-362), reorder them by FileInfo.channelMap like
// RGBAoutputFile::WriteFile (reference: src/common/j2k_rgba_file.cpp:763-813), call
// Codec::WriteFile through the base-class pointer, collect the bytes in an in-memory OutputFile.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hip_codec.h"

namespace {

class MemoryOutputFile : public j2k::OutputFile {
  public:
    std::vector<unsigned char> data;
    size_t pos = 0;
    size_t max_write = (size_t)-1; // fault injection: accept at most this many bytes per Write
    virtual WriteFlags Flags() const { return J2K_WRITE_SEEKABLE | J2K_WRITE_READABLE; }
    virtual size_t Read(void *buf, size_t n)
    {
        if (pos >= data.size()) return 0;
        n = n < data.size() - pos ? n : data.size() - pos;
        std::memcpy(buf, data.data() + pos, n);
        pos += n;
        return n;
    }
    virtual size_t Write(const void *buf, size_t n)
    {
        if (n > max_write) n = max_write;
        if (pos + n > data.size()) data.resize(pos + n);
        std::memcpy(data.data() + pos, buf, n);
        pos += n;
        return n;
    }
    virtual bool Seek(size_t p) { pos = p; return true; }
    virtual size_t Tell() { return pos; }
};

class MemoryInputFile : public j2k::InputFile {
  public:
    const unsigned char *data;
    size_t len, pos;
    MemoryInputFile(const unsigned char *d, size_t n) : data(d), len(n), pos(0) {}
    virtual ReadFlags Flags() const { return J2K_READ_SEEKABLE; }
    virtual size_t FileSize() { return len; }
    virtual size_t Read(void *buf, size_t n)
    {
        if (pos >= len) return 0;
        n = n < len - pos ? n : len - pos;
        std::memcpy(buf, data + pos, n);
        pos += n;
        return n;
    }
    virtual bool Seek(size_t p) { pos = p; return true; }
    virtual size_t Tell() { return pos; }
};

// Stands in for the plug-in's OpenJPEGCodec behind HipCodec::SetFallback: records that it was asked and fills what it
// is handed with a recognisable answer (the tests check that unsupported files get here, and only those).
class RecordingCodec : public j2k::Codec {
  public:
    int infos = 0, reads = 0;
    virtual const char *Name() const { return "Recording"; }
    virtual const char *FourCharCode() const { return "recd"; }
    virtual ReadFlags GetReadFlags() { return J2K_CAN_READ; }
    virtual WriteFlags GetWriteFlags() { return 0; }
    virtual bool Verify(j2k::InputFile &) { return true; }
    virtual void GetFileInfo(j2k::InputFile &, j2k::FileInfo &info) { ++infos; info.width = 4242; info.height = 2424; info.channels = 3; info.depth = 8; }
    virtual void ReadFile(j2k::InputFile &, const j2k::Buffer &buffer, unsigned int, j2k::Progress *)
    {
        ++reads;
        for (int c = 0; c < buffer.channels; c++) *buffer.channel[c].buf = (unsigned char)(0xC0 + c);
    }
    virtual void WriteFile(j2k::OutputFile &, const j2k::FileInfo &, const j2k::Buffer &, j2k::Progress *) { throw j2k::Exception("read only"); }
};

// test knobs of the read hooks: HipCodec::SetReadLayers, and HipCodec::SetReadCinemaColour (J2K_HOST_TEST_READ_CINEMA = the
// target; J2K_HOST_TEST_READ_CINEMA_ALL set to anything but 0: profileFilesOnly = false)
void read_knobs(j2k::HipCodec &hip)
{
    if (const char *l = std::getenv("J2K_HOST_TEST_READ_LAYERS")) hip.SetReadLayers((unsigned)std::atoi(l));
    if (const char *t = std::getenv("J2K_HOST_TEST_READ_CINEMA")) {
        const char *all = std::getenv("J2K_HOST_TEST_READ_CINEMA_ALL");
        hip.SetReadCinemaColour((unsigned)std::atoi(t), !(all && std::atoi(all) != 0));
    }
}

} // namespace

extern "C" {

// HipCodec with a fallback reader: returns 0 = decoded on the GPU, 1 = the fallback was asked (for GetFileInfo and
// ReadFile), -1 = j2k::Exception (what() in err).  with_fallback = 0: no fallback installed.
long j2k_host_test_read_fallback(const unsigned char *file, unsigned long file_len, int with_fallback, unsigned char *frame, unsigned width,
                                 unsigned height, int channels, long *info_out, char *err, unsigned long err_cap)
{
    using namespace j2k;
    Buffer buf;
    buf.channels = (unsigned char)channels;
    for (int c = 0; c < channels; c++) {
        Channel &ch = buf.channel[c];
        ch.width = width; ch.height = height; ch.sampleType = UCHAR; ch.depth = 8; ch.sgnd = false;
        ch.buf = frame + (size_t)c * width * height; ch.colbytes = 1; ch.rowbytes = width;
    }
    MemoryInputFile in(file, file_len);
    HipCodec hip(HipCodec::HonourSettings);
    read_knobs(hip);
    RecordingCodec other;
    if (with_fallback) hip.SetFallback(&other);
    Codec *codec = &hip;
    try {
        FileInfo info;
        codec->GetFileInfo(in, info);
        if (info_out) { info_out[0] = info.width; info_out[1] = info.height; info_out[2] = info.channels; }
        codec->ReadFile(in, buf, 1, NULL);
    } catch (const Exception &e) {
        if (err && err_cap) {
            std::string m = std::string(e.what()) + " | " + HipCodec::LastError();
            std::strncpy(err, m.c_str(), err_cap - 1);
            err[err_cap - 1] = 0;
        }
        return -1;
    }
    if (other.infos != other.reads) return -2;
    return other.reads ? 1 : 0;
}

// HipCodec::ReadFiles: n frames of file_len[f] bytes at files[f] into planar 8-bit channels, frame f at
// frames + f * channels * width * height.  Returns 1 = all frames written, 0 = ReadFiles returned false (the caller reads frame by
// frame), -1 = j2k::Exception (what() in err).
long j2k_host_test_read_files(const unsigned char *const *files, const unsigned long *file_len, unsigned n, unsigned subsample,
                              unsigned char *frames, unsigned width, unsigned height, int channels, char *err, unsigned long err_cap)
{
    using namespace j2k;
    std::vector<Buffer> bufs(n);
    std::vector<MemoryInputFile> ins;
    std::vector<InputFile *> ptrs;
    ins.reserve(n);
    for (unsigned f = 0; f < n; f++) {
        bufs[f].channels = (unsigned char)channels;
        for (int c = 0; c < channels; c++) {
            Channel &ch = bufs[f].channel[c];
            ch.width = width; ch.height = height; ch.sampleType = UCHAR; ch.depth = 8; ch.sgnd = false;
            ch.buf = frames + ((size_t)f * channels + c) * width * height; ch.colbytes = 1; ch.rowbytes = width;
        }
        ins.push_back(MemoryInputFile(files[f], file_len[f]));
    }
    for (unsigned f = 0; f < n; f++) ptrs.push_back(&ins[f]);
    HipCodec hip(HipCodec::HonourSettings);
    read_knobs(hip);
    try {
        return hip.ReadFiles(ptrs.data(), bufs.data(), n, subsample) ? 1 : 0;
    } catch (const Exception &e) {
        if (err && err_cap) {
            std::string m = std::string(e.what()) + " | " + HipCodec::LastError();
            std::strncpy(err, m.c_str(), err_cap - 1);
            err[err_cap - 1] = 0;
        }
        return -1;
    }
}

// The read side, driven like RGBAinputFile drives a Codec (reference: src/common/j2k_rgba_file.cpp:450-735 ->
// Codec::ReadFile, src/common/j2k_codec.h:311): `frame` is the host's interleaved A,R,G,B buffer (pixel_size = bytes
// per sample) of width x height pixels = the image size / subsample; codec channel c goes to the RGBA channel named
// channelMap[c] (R,G,B,A).  Only the channels' samples may change.  Returns 0, or -1 with what() in err.
long j2k_host_test_read(const unsigned char *file, unsigned long file_len, unsigned subsample, unsigned char *frame, unsigned width,
                        unsigned height, long rowbytes, int pixel_size, int channels, int depth, char *err, unsigned long err_cap)
{
    using namespace j2k;
    Channel argb[4];
    for (int i = 0; i < 4; i++) {
        Channel &c = argb[i];
        c.width = width; c.height = height;
        c.sampleType = pixel_size == 4 ? FLOAT : (pixel_size == 2 ? USHORT : UCHAR); // (4: an ARGB128 world of floats, depth 32)
        c.depth = (unsigned char)depth;
        c.sgnd = false;
        c.buf = frame + i * pixel_size;
        c.colbytes = 4 * pixel_size;
        c.rowbytes = rowbytes;
    }
    const Channel *by_name[4] = {&argb[1], &argb[2], &argb[3], &argb[0]}; // RED, GREEN, BLUE, ALPHA
    Buffer buf;
    buf.channels = (unsigned char)channels;
    for (int c = 0; c < channels; c++) buf.channel[c] = *by_name[c];
    MemoryInputFile in(file, file_len);
    HipCodec hip(HipCodec::HonourSettings);
    read_knobs(hip);
    Codec *codec = &hip;
    try {
        if (!codec->Verify(in)) throw Exception("Can't read this format");
        codec->ReadFile(in, buf, subsample, NULL);
    } catch (const Exception &e) {
        if (err && err_cap) {
            std::string m = std::string(e.what()) + " | " + HipCodec::LastError();
            std::strncpy(err, m.c_str(), err_cap - 1);
            err[err_cap - 1] = 0;
        }
        return -1;
    }
    return 0;
}

// HipCodec::ReadRGBA, driven like the three lines at the top of RGBAinputFile::ReadFile drive it: `frame` is
// the host's interleaved A,R,G,B world as WorldToBuffer lays it out (pixel_size = bytes per sample; depth = Channel.depth) of
// width x height pixels; demote != 0: the codec has the DemoteAE16 option; with_alpha = 0: no alpha channel is handed over.
// Returns 1 = the frame is written, 0 = not taken (nothing written), -1 with what() in err.
long j2k_host_test_read_rgba(const unsigned char *file, unsigned long file_len, unsigned subsample, unsigned char *frame, unsigned width,
                             unsigned height, long rowbytes, int pixel_size, int depth, int demote, int with_alpha, char *err,
                             unsigned long err_cap)
{
    using namespace j2k;
    Channel argb[4];
    for (int i = 0; i < 4; i++) {
        Channel &c = argb[i];
        c.width = width; c.height = height;
        c.sampleType = pixel_size == 4 ? FLOAT : (pixel_size == 2 ? USHORT : UCHAR); // (4: an ARGB128 world of floats, depth 32)
        c.depth = (unsigned char)depth;
        c.sgnd = false;
        c.buf = frame + i * pixel_size;
        c.colbytes = 4 * pixel_size;
        c.rowbytes = rowbytes;
    }
    if (!with_alpha) argb[0].buf = NULL;
    MemoryInputFile in(file, file_len);
    HipCodec hip(HipCodec::HonourSettings, -1, demote ? HipCodec::DemoteAE16 : HipCodec::NoOptions);
    read_knobs(hip);
    try {
        return hip.ReadRGBA(in, argb[1], argb[2], argb[3], argb[0], subsample, NULL) ? 1 : 0;
    } catch (const Exception &e) {
        if (err && err_cap) {
            std::string m = std::string(e.what()) + " | " + HipCodec::LastError();
            std::strncpy(err, m.c_str(), err_cap - 1);
            err[err_cap - 1] = 0;
        }
        return -1;
    }
}

// GetFileInfo through the interface: out[] = {width, height, channels, depth, format, colorSpace, alpha, profileLen,
// reversible, channelMap[0..3]}; the ICC profile (the codec's malloc'd copy) goes to icc_out and is freed.
long j2k_host_test_info(const unsigned char *file, unsigned long file_len, long *out, unsigned char *icc_out, unsigned long icc_cap,
                        char *err, unsigned long err_cap)
{
    using namespace j2k;
    MemoryInputFile in(file, file_len);
    HipCodec hip(HipCodec::HonourSettings);
    Codec *codec = &hip;
    FileInfo info;
    try {
        codec->GetFileInfo(in, info);
    } catch (const Exception &e) {
        if (err && err_cap) {
            std::string m = std::string(e.what()) + " | " + HipCodec::LastError();
            std::strncpy(err, m.c_str(), err_cap - 1);
            err[err_cap - 1] = 0;
        }
        return -1;
    }
    out[0] = info.width; out[1] = info.height; out[2] = info.channels; out[3] = info.depth; out[4] = info.format;
    out[5] = info.colorSpace; out[6] = info.alpha; out[7] = (long)info.profileLen; out[8] = info.settings.reversible;
    for (int i = 0; i < 4; i++) out[9 + i] = info.channelMap[i];
    if (info.iccProfile) {
        if (icc_out && info.profileLen <= icc_cap) std::memcpy(icc_out, info.iccProfile, info.profileLen);
        std::free(info.iccProfile);
    }
    return 0;
}

// The palette GetFileInfo reports (FileInfo.LUTsize / .LUT / .LUTmap, reference: j2k_openjpeg_codec.cpp:362-401): returns LUTsize
// (-1 after an exception); lut_out = LUTsize x 4 bytes (LUT[i].channel[0..3]), lutmap_out[0..3] = LUTmap.
long j2k_host_test_lut(const unsigned char *file, unsigned long file_len, unsigned char *lut_out, long *lutmap_out)
{
    using namespace j2k;
    MemoryInputFile in(file, file_len);
    HipCodec hip(HipCodec::HonourSettings);
    Codec *codec = &hip;
    FileInfo info;
    try {
        codec->GetFileInfo(in, info);
    } catch (const Exception &) {
        return -1;
    }
    for (unsigned i = 0; i < info.LUTsize; i++)
        for (int c = 0; c < 4; c++) lut_out[4 * i + c] = info.LUT[i].channel[c];
    for (int i = 0; i < 4; i++) lutmap_out[i] = info.LUTmap[i];
    if (info.iccProfile) std::free(info.iccProfile);
    return (long)info.LUTsize;
}

// frame: interleaved A,R,G,B samples (pixel_size = bytes per sample: 1, 2 or 4 = floats), rowbytes as in
// PF_EffectWorld.  channels = 1, 3 or 4 (FileInfo.channels); honour != 0 -> HipCodec::HonourSettings.
// Returns the codestream length (copied to out if it fits), or -1 after a j2k::Exception whose
// what() is copied to err.
long j2k_host_test_write_ex(const unsigned char *frame, unsigned width, unsigned height, long rowbytes, int pixel_size,
                            int channels, int depth, int reversible, int ycc, int layers, int tile_size, int honour,
                            long max_write, int format, int color_space, const void *icc, unsigned long icc_len,
                            int alpha_kind, unsigned char *out, unsigned long out_cap, char *err, unsigned long err_cap);

long j2k_host_test_write(const unsigned char *frame, unsigned width, unsigned height, long rowbytes, int pixel_size,
                         int channels, int depth, int reversible, int ycc, int layers, int tile_size, int honour,
                         long max_write, unsigned char *out, unsigned long out_cap, char *err, unsigned long err_cap)
{
    return j2k_host_test_write_ex(frame, width, height, rowbytes, pixel_size, channels, depth, reversible, ycc, layers,
                                  tile_size, honour, max_write, j2k::UNKNOWN_FORMAT, j2k::UNKNOWN_COLOR_SPACE, NULL, 0, -1,
                                  out, out_cap, err, err_cap);
}

} // extern "C"

namespace {
long write_frame(const unsigned char *frame, unsigned width, unsigned height, long rowbytes, int pixel_size,
                 int channels, int depth, int reversible, int ycc, int layers, int tile_size, int honour,
                 long max_write, int format, int color_space, const void *icc, unsigned long icc_len,
                 int alpha_kind, unsigned extra_options, unsigned char *out, unsigned long out_cap, char *err, unsigned long err_cap);
}

extern "C" {

// Same with the file-level fields of FileInfo: format (j2k::Format), color_space (j2k::ColorSpace), ICC
// profile, alpha_kind (j2k::Alpha, or -1 = STRAIGHT for 4 channels / NO_ALPHA otherwise).
long j2k_host_test_write_ex(const unsigned char *frame, unsigned width, unsigned height, long rowbytes, int pixel_size,
                            int channels, int depth, int reversible, int ycc, int layers, int tile_size, int honour,
                            long max_write, int format, int color_space, const void *icc, unsigned long icc_len,
                            int alpha_kind, unsigned char *out, unsigned long out_cap, char *err, unsigned long err_cap)
{
    return write_frame(frame, width, height, rowbytes, pixel_size, channels, depth, reversible, ycc, layers, tile_size, honour, max_write,
                       format, color_space, icc, icc_len, alpha_kind, 0u, out, out_cap, err, err_cap);
}

// j2k_host_test_write with HipCodec options given by the caller (HipCodec::Options bits, e.g. CinemaXYZ = 16) on top of the
// environment's knobs.
long j2k_host_test_write_options(const unsigned char *frame, unsigned width, unsigned height, long rowbytes, int pixel_size,
                                 int channels, int depth, int reversible, int ycc, int layers, int tile_size, int honour,
                                 unsigned options, unsigned char *out, unsigned long out_cap, char *err, unsigned long err_cap)
{
    return write_frame(frame, width, height, rowbytes, pixel_size, channels, depth, reversible, ycc, layers, tile_size, honour, -1,
                       j2k::UNKNOWN_FORMAT, j2k::UNKNOWN_COLOR_SPACE, NULL, 0, -1, options, out, out_cap, err, err_cap);
}

} // extern "C"

namespace {

long write_frame(const unsigned char *frame, unsigned width, unsigned height, long rowbytes, int pixel_size,
                 int channels, int depth, int reversible, int ycc, int layers, int tile_size, int honour,
                 long max_write, int format, int color_space, const void *icc, unsigned long icc_len,
                 int alpha_kind, unsigned extra_options, unsigned char *out, unsigned long out_cap, char *err, unsigned long err_cap)
{
    using namespace j2k;
    // WorldToBuffer: channel i of (A,R,G,B) starts at byte i*pixelSize
    Channel argb[4];
    for (int i = 0; i < 4; i++) {
        Channel &c = argb[i];
        c.width = width; c.height = height;
        c.sampleType = pixel_size == 4 ? FLOAT : (pixel_size == 2 ? USHORT : UCHAR); // (4: an ARGB128 world of floats, depth 32)
        c.depth = (unsigned char)(pixel_size * 8);
        c.sgnd = false;
        c.buf = const_cast<unsigned char *>(frame) + i * pixel_size;
        c.colbytes = 4 * pixel_size;
        c.rowbytes = rowbytes;
    }
    FileInfo info;
    info.width = width; info.height = height;
    info.channels = (unsigned char)channels; info.depth = (unsigned char)depth;
    info.alpha = alpha_kind >= 0 ? (Alpha)alpha_kind : (channels == 4 ? STRAIGHT : NO_ALPHA);
    info.settings.order = LRCP; // (the settings default is RPCL; the fixtures of the tests are LRCP)
    if (const char *ord = std::getenv("J2K_HOST_TEST_ORDER")) info.settings.order = (Order)std::atoi(ord);
    if (const char *kb = std::getenv("J2K_HOST_TEST_FILESIZE_KB")) { // test knob: settings.method = SIZE
        info.settings.method = SIZE;
        info.settings.fileSize = (size_t)std::atol(kb);
    }
    if (const char *m = std::getenv("J2K_HOST_TEST_CINEMA")) { // test knob: settings.method = CINEMA, value = DCI profile (2 | 4)
        info.settings.method = CINEMA;
        info.settings.dciProfile = std::atoi(m) == 4 ? DCI_4K : DCI_2K;
    }
    if (const char *a = std::getenv("J2K_HOST_TEST_ASPECT")) { // "num:den"
        int n = 0, d = 1;
        if (std::sscanf(a, "%d:%d", &n, &d) == 2) info.pixelAspect = Rational(n, d);
    }
    if (const char *d = std::getenv("J2K_HOST_TEST_DPI")) info.dpi = (float)std::atof(d);
    info.format = (Format)format;
    info.colorSpace = (ColorSpace)color_space;
    info.iccProfile = const_cast<void *>(icc); info.profileLen = icc_len;
    info.settings.reversible = reversible != 0; info.settings.ycc = ycc != 0;
    info.settings.layers = (unsigned char)layers; info.settings.tileSize = (unsigned short)tile_size;
    // RGBAoutputFile::WriteFile: codec channel c = the RGBA channel named channelMap[c]
    const Channel *by_name[4] = {&argb[1], &argb[2], &argb[3], &argb[0]}; // RED, GREEN, BLUE, ALPHA
    Buffer buf;
    buf.channels = info.channels;
    for (int c = 0; c < channels; c++) buf.channel[c] = *by_name[info.channelMap[c]];

    MemoryOutputFile file;
    if (max_write >= 0) file.max_write = (size_t)max_write;
    const bool promote = std::getenv("J2K_HOST_TEST_PROMOTE") != NULL; // test knob: the world holds 15+1-bit samples
    unsigned options = (promote ? HipCodec::PromoteAE16 : HipCodec::NoOptions) | extra_options;
    if (const char *ch = std::getenv("J2K_HOST_TEST_CHROMA")) // test knob: 422 | 420 -> HipCodec::Chroma422 / Chroma420
        options |= std::atoi(ch) == 420 ? HipCodec::Chroma420 : (std::atoi(ch) == 422 ? HipCodec::Chroma422 : 0u);
    HipCodec hip(honour ? HipCodec::HonourSettings : HipCodec::ReferenceLiteral, -1, options);
    if (const char *q = std::getenv("J2K_HOST_TEST_QUALITY")) { // test knob: settings.method = QUALITY; value = the slopes for
        info.settings.method = QUALITY;                          // SetQualitySlopes, comma-separated (hex floats keep every bit), or "" for none
        double slopes[J2K_CODEC_MAX_LAYERS + 1];
        unsigned n = 0;
        for (const char *s = q; *s && n <= J2K_CODEC_MAX_LAYERS;) {
            char *end = NULL;
            const double v = std::strtod(s, &end);
            if (end == s) break;
            slopes[n++] = v;
            s = *end == ',' ? end + 1 : end;
        }
        if (n) hip.SetQualitySlopes(slopes, n);
    }
    Codec *codec = &hip; // through the interface, as RGBAoutputFile does (j2k_rgba_file.cpp:812)
    try {
        codec->WriteFile(file, info, buf, NULL);
    } catch (const Exception &e) {
        if (err && err_cap) {
            std::string m = std::string(e.what()) + " | " + HipCodec::LastError();
            std::strncpy(err, m.c_str(), err_cap - 1);
            err[err_cap - 1] = 0;
        }
        return -1;
    }
    if (out && file.data.size() <= out_cap) std::memcpy(out, file.data.data(), file.data.size());
    return (long)file.data.size();
}

} // namespace

extern "C" {

// HipCodec::WriteFiles: n A,R,G,B worlds (frames[f], laid out as for j2k_host_test_write) to a byte budget, HonourSettings with
// settings.method = SIZE and a file size set (both must be ignored).  File f is copied to out + f * out_stride and its length to
// lens[f].  Returns 0, or -1 after a j2k::Exception (what() | LastError() in err): lens[f] then holds what file f had received.
long j2k_host_test_write_files(const unsigned char *const *frames, unsigned n, unsigned width, unsigned height, long rowbytes, int pixel_size,
                               int channels, int depth, int reversible, int ycc, int tile_size, unsigned options, unsigned long long total_bytes,
                               unsigned long long frame_max_bytes, unsigned char *out, unsigned long out_stride, unsigned long *lens, char *err,
                               unsigned long err_cap)
{
    using namespace j2k;
    FileInfo info;
    info.width = width; info.height = height;
    info.channels = (unsigned char)channels; info.depth = (unsigned char)depth;
    info.alpha = channels == 4 ? STRAIGHT : NO_ALPHA;
    info.settings.order = LRCP;
    info.settings.method = SIZE; info.settings.fileSize = 1; info.settings.layers = 3;
    info.settings.reversible = reversible != 0; info.settings.ycc = ycc != 0;
    info.settings.tileSize = (unsigned short)tile_size;
    std::vector<Buffer> bufs(n);
    for (unsigned f = 0; f < n; f++) {
        Channel argb[4];
        for (int i = 0; i < 4; i++) {
            Channel &c = argb[i];
            c.width = width; c.height = height;
            c.sampleType = pixel_size == 4 ? FLOAT : (pixel_size == 2 ? USHORT : UCHAR);
            c.depth = (unsigned char)(pixel_size * 8);
            c.sgnd = false;
            c.buf = const_cast<unsigned char *>(frames[f]) + i * pixel_size;
            c.colbytes = 4 * pixel_size;
            c.rowbytes = rowbytes;
        }
        const Channel *by_name[4] = {&argb[1], &argb[2], &argb[3], &argb[0]}; // RED, GREEN, BLUE, ALPHA
        bufs[f].channels = info.channels;
        for (int c = 0; c < channels; c++) bufs[f].channel[c] = *by_name[info.channelMap[c]];
    }
    std::vector<MemoryOutputFile> files(n);
    std::vector<OutputFile *> ptrs;
    for (unsigned f = 0; f < n; f++) ptrs.push_back(&files[f]);
    HipCodec hip(HipCodec::HonourSettings, -1, options);
    long rc = 0;
    try {
        hip.WriteFiles(ptrs.data(), info, bufs.data(), n, total_bytes, frame_max_bytes);
    } catch (const Exception &e) {
        if (err && err_cap) {
            std::string m = std::string(e.what()) + " | " + HipCodec::LastError();
            std::strncpy(err, m.c_str(), err_cap - 1);
            err[err_cap - 1] = 0;
        }
        rc = -1;
    }
    for (unsigned f = 0; f < n; f++) {
        lens[f] = (unsigned long)files[f].data.size();
        if (out && files[f].data.size() <= out_stride) std::memcpy(out + (size_t)f * out_stride, files[f].data.data(), files[f].data.size());
    }
    return rc;
}

// HipCodec::Compare of `file` against the A,R,G,B world `frame` (as in j2k_host_test_write: HonourSettings, the PROMOTE and
// CHROMA knobs, FileInfo of width x height x channels at `depth` bits; the coding settings do not matter).  ints_out = 7 values
// per channel (samples, differing, sumAbs, sumSq, maxAbs, firstX, firstY), dbl_out = 2 (mse, psnr).  Returns 1 = compared,
// 0 = Compare returned false (nothing written), -1 = j2k::Exception (what() in err).
long j2k_host_test_compare(const unsigned char *file, unsigned long file_len, int with_fallback, const unsigned char *frame, unsigned width,
                           unsigned height, long rowbytes, int pixel_size, int channels, int depth, unsigned long long *ints_out,
                           double *dbl_out, char *err, unsigned long err_cap)
{
    using namespace j2k;
    Channel argb[4];
    for (int i = 0; i < 4; i++) {
        Channel &c = argb[i];
        c.width = width; c.height = height;
        c.sampleType = pixel_size == 4 ? FLOAT : (pixel_size == 2 ? USHORT : UCHAR);
        c.depth = (unsigned char)(pixel_size * 8);
        c.sgnd = false;
        c.buf = const_cast<unsigned char *>(frame) + i * pixel_size;
        c.colbytes = 4 * pixel_size;
        c.rowbytes = rowbytes;
    }
    FileInfo info;
    info.width = width; info.height = height;
    info.channels = (unsigned char)channels; info.depth = (unsigned char)depth;
    info.alpha = channels == 4 ? STRAIGHT : NO_ALPHA;
    const Channel *by_name[4] = {&argb[1], &argb[2], &argb[3], &argb[0]}; // RED, GREEN, BLUE, ALPHA
    Buffer buf;
    buf.channels = info.channels;
    for (int c = 0; c < channels; c++) buf.channel[c] = *by_name[info.channelMap[c]];
    unsigned options = std::getenv("J2K_HOST_TEST_PROMOTE") != NULL ? HipCodec::PromoteAE16 : HipCodec::NoOptions;
    if (const char *ch = std::getenv("J2K_HOST_TEST_CHROMA"))
        options |= std::atoi(ch) == 420 ? HipCodec::Chroma420 : (std::atoi(ch) == 422 ? HipCodec::Chroma422 : 0u);
    HipCodec hip(HipCodec::HonourSettings, -1, options);
    read_knobs(hip);
    RecordingCodec other;
    if (with_fallback) hip.SetFallback(&other);
    MemoryInputFile in(file, file_len);
    HipCodec::Difference d[J2K_CODEC_MAX_CHANNELS];
    std::memset(d, 0xA5, sizeof(d));
    try {
        if (!hip.Compare(in, info, buf, d)) {
            for (size_t i = 0; i < sizeof(d); i++) if (reinterpret_cast<const unsigned char *>(d)[i] != 0xA5) return -2; // (false: nothing written)
            return other.infos || other.reads ? -3 : 0; // (... and the fallback codec has no such call)
        }
    } catch (const Exception &e) {
        if (err && err_cap) {
            std::string m = std::string(e.what()) + " | " + HipCodec::LastError();
            std::strncpy(err, m.c_str(), err_cap - 1);
            err[err_cap - 1] = 0;
        }
        return -1;
    }
    for (int c = 0; c < channels; c++) {
        unsigned long long *o = ints_out + 7 * c;
        o[0] = d[c].samples; o[1] = d[c].differing; o[2] = d[c].sumAbs; o[3] = d[c].sumSq; o[4] = d[c].maxAbs; o[5] = d[c].firstX; o[6] = d[c].firstY;
        dbl_out[2 * c] = d[c].mse; dbl_out[2 * c + 1] = d[c].psnr;
    }
    return 1;
}

const char *j2k_host_codec_name(void)
{
    static j2k::HipCodec c;
    return c.Name();
}

} // extern "C"
