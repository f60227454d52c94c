// hip_codec.h -- `j2k::HipCodec`, the MI355X encode codec behind the plug-in's Codec interface.
//
// Drop-in for OpenJPEGCodec::WriteFile (reference: src/common/j2k_openjpeg_codec.cpp:589-758):
// same virtual signature (src/common/j2k_codec.h:315), same error convention (throws
// j2k::Exception("Error writing file")), same sink (OutputFile::Write).  Registered by one
// `push_back(new HipCodec)` in CodecContainer::CodecContainer (src/common/j2k_codec.cpp:508-519);
// its name "HIP" sorts before "OpenJPEG", so GetDefaultCodec() (j2k_codec.cpp:540-548) picks it.
#pragma once

#include "j2k_codec_api.h"

namespace j2k {

class HipCodec : public Codec {
  public:
    // ReferenceLiteral reproduces the reference adapter's parameterisation exactly (5/3 reversible,
    // no colour transform -- it never copies settings.reversible/.ycc, j2k_openjpeg_codec.cpp:703-709);
    // HonourSettings maps settings.reversible -> 5/3 vs 9/7 and settings.ycc -> RCT/ICT.
    enum Mode { ReferenceLiteral, HonourSettings };

    // Options (bit flags).
    //   PromoteAE16: 16-bit (USHORT) channels hold After Effects' "15+1-bit" samples (0..32768): the 15+1 -> 16 bit
    //   Promote() of the AE layer (reference: src/aftereffects/FrameSeq.cpp:311-355) is applied on the GPU while the
    //   samples are loaded, so the caller drops the PromoteWorld / DemoteWorld pair around WriteFile
    //   (src/aftereffects/j2k.cpp:843-855: two host passes over the frame) and hands over the world as it is.
    //   DemoteAE16: the mirror on the read side.  ReadRGBA into four 16-bit (USHORT) channels delivers 15+1-bit samples:
    //   Demote() (FrameSeq.cpp:265-268) is applied by the decode's output kernel, so the caller drops the DemoteWorld pass
    //   of j2k_DrawSparseFrame (src/aftereffects/j2k.cpp:482-492).
    //   Chroma422 / Chroma420 (HonourSettings, buffers of 3 or 4 channels; ignored in ReferenceLiteral mode, for 1- and
    //   2-channel buffers and under a cinema profile): WriteFile writes Y Cb Cr with the chroma sub-sampled 2 x 1 / 2 x 2 --
    //   what broadcast and proxy JPEG 2000 use -- made from the world's R, G, B on the GPU while the samples are loaded
    //   (j2k_hip_params.rgb_to_sycc; settings.ycc is not used, an alpha channel stays full size).  The colour space written
    //   is sYCC: with FileInfo.format JP2 the colr box says so and ReadRGBA returns R, G, B again.  Both bits: 4:2:0.
    //   CinemaXYZ (HonourSettings, settings.method CINEMA, buffers of 3 channels of 8-bit, 16-bit or float samples within
    //   4096 x 2160; ignored otherwise): the world's R, G, B are sRGB and WriteFile writes what a DCI frame holds -- 12-bit
    //   X'Y'Z' code values, made on the GPU while the samples are loaded (j2k_hip_params.rgb_to_xyz = 1, depth 12 whatever
    //   FileInfo.depth says: the transform is the depth conversion).  The real profile (dci_profile 3 / 4) is then reached
    //   for any world depth when the frame fits the container.  No ICC profile is written and the colour space is
    //   unspecified.  Compare takes the same mapping.  With Chroma422 / Chroma420 as well, CinemaXYZ wins on such a frame.
    //   AutoGuardBits (both modes; not under a cinema profile, which is pinned to libopenjp2's bytes): WriteFile writes a frame
    //   whose coefficients outgrow the bit-planes two guard bits signal -- a lossless frame that libopenjp2 writes wrongly
    //   and this codec otherwise refuses with "Error writing file" -- with the guard bits it needs
    //   (j2k_hip_params.guard_bits = J2K_HIP_GUARD_AUTO).  Every other frame is written byte for byte as without the option;
    //   ReadFile and Compare take the count from the file.
    enum Options { NoOptions = 0, PromoteAE16 = 1, DemoteAE16 = 2, Chroma422 = 4, Chroma420 = 8, CinemaXYZ = 16, AutoGuardBits = 32 };

    // device: HIP device ordinal, or -1 = the host threads that call this codec take the devices in turn
    explicit HipCodec(Mode mode = ReferenceLiteral, int device = -1, unsigned options = NoOptions);
    virtual ~HipCodec();

    // Read side.  "HIP" sorts before "OpenJPEG", so GetDefaultCodec() (src/common/j2k_codec.cpp:540-548) makes this codec
    // the default READER too (RGBAinputFile, src/common/j2k_rgba_file.cpp:41).  Files that use a JPEG 2000 feature the
    // GPU decoder does not implement (status J2K_HIP_ERR_UNSUPPORTED: a COC that differs from the COD, coding-style or
    // quantisation overrides in tile-part headers, code-blocks beyond 64 x 64, more than 4 components, more than 16 bits, a
    // region-of-interest shift beyond 30 bit-planes, a palette) are handed to `fallback` -- the plug-in passes its OpenJPEGCodec -- for
    // GetFileInfo and ReadFile alike, so nothing the reference can open is lost.  Borrowed, may be NULL (the default):
    // such files then fail with "Error reading file" like any other failure.  Malformed files never reach the fallback.
    void SetFallback(Codec *fallback) { _fallback = fallback; }
    Codec *Fallback() const { return _fallback; }

    virtual const char *Name() const { return "HIP"; }
    virtual const char *FourCharCode() const { return "hipJ"; }
    virtual ReadFlags GetReadFlags() { return J2K_CAN_READ | J2K_CAN_SUBSAMPLE; }
    virtual WriteFlags GetWriteFlags() { return J2K_CAN_WRITE; }

    virtual bool Verify(InputFile &file);
    virtual void GetFileInfo(InputFile &file, FileInfo &info);  // replaces OpenJPEGCodec::GetFileInfo (j2k_openjpeg_codec.cpp:222-448)
    // replaces OpenJPEGCodec::ReadFile (:451-586); subsample = 1, 2, 4 ...: the image of ceil(size / subsample)
    // goes to the top-left of the destination channels
    virtual void ReadFile(InputFile &file, const Buffer &buffer, unsigned int subsample = 1, Progress *progress = NULL);
    virtual void WriteFile(OutputFile &file, const FileInfo &info, const Buffer &buffer, Progress *progress = NULL);
    // Channels of sampleType FLOAT, depth 32 (a 32-bpc world, ARGB128) are taken by WriteFile, ReadFile, ReadRGBA and ReadFiles
    // as they are: they stand for 16-bit samples (planes of sample_bits 32, depth 16; include/j2k_hip.h), quantised by the
    // front-end kernel and written as floats by the output kernels.  PromoteAE16 / DemoteAE16 select the 15+1-bit forms.

    // The whole of RGBAinputFile::ReadFile (src/common/j2k_rgba_file.cpp:450-735) in one decode: the file's components go
    // straight to the R, G, B, A channels of the caller's world -- sYCC -> RGB, grey into three channels, the palette
    // look-up, the alpha fill (full scale at the channels' depth: 2^depth - 1, where the reference stores 255 into a 16-bit
    // world) and, with DemoteAE16 and four USHORT or FLOAT channels, Demote -- in the decode's output kernel (include/j2k_hip.h:
    // j2k_hip_decode_rgba).  a.buf == NULL: no alpha wanted.
    // true: the frame is written.  false: not a file the fused path takes (status J2K_HIP_ERR_UNSUPPORTED: CMYK, e-sYCC, an
    // opacity channel that is not the last one, a feature the GPU decoder lacks ... -- the reference's own code asserts on the
    // first three); nothing is written and the caller goes on as before (RGBAinputFile's own path, which reaches ReadFile and
    // the fallback codec).  Damaged files and device failures throw "Error reading file".
    bool ReadRGBA(InputFile &file, const Channel &r, const Channel &g, const Channel &b, const Channel &a,
                  unsigned int subsample = 1, Progress *progress = NULL);

    // The frames of an image sequence in one decode (include/j2k_hip.h: j2k_hip_decode_sequence): files[i] goes to buffers[i]
    // as ReadFile(*files[i], buffers[i], subsample) would put it, the code-blocks of all n frames sharing their kernel
    // launches -- one host thread and one stream keep the GPU as busy as a thread and a handle per frame did.
    // true: all n frames are written.  false: nothing is written, because the frames cannot share a call -- one of them is
    // for the fallback reader (J2K_HIP_ERR_UNSUPPORTED) or differs from the first in geometry or coding parameters; the
    // caller reads them frame by frame through ReadFile.  A damaged frame and device failures throw "Error reading file"
    // (frames before the damaged one may have been written); LastError() names the frame.
    bool ReadFiles(InputFile *const *files, const Buffer *buffers, unsigned n, unsigned subsample);

    // The frames of a shot to a byte budget in one encode (include/j2k_hip.h: j2k_hip_encode_sequence_budget), the mirror of
    // ReadFiles: buffers[i] goes to *files[i] under the FileInfo / Buffer mapping of WriteFile, all n files together in at most
    // total_bytes and none above frame_max_bytes (0: no limit), every frame cut at one rate-distortion slope threshold unless
    // its own limit asks for a coarser one -- quality as even as the two limits allow.  settings.method and settings.layers
    // are not looked at (the budget sets the cut, in one layer), and AutoGuardBits does not apply.  Throws "Error writing file"
    // on failure -- a budget that cannot be met among them, LastError() naming the limit -- with nothing written to any file.
    void WriteFiles(OutputFile *const *files, const FileInfo &info, const Buffer *buffers, unsigned n, unsigned long long total_bytes,
                    unsigned long long frame_max_bytes);

    // What did a file lose against the frame it was written from?  `info` and `buffer` are what WriteFile was given (the same
    // FileInfo / Buffer -> parameters / planes mapping: PromoteAE16, FLOAT channels and Chroma422 / Chroma420 included); the
    // file is decoded and compared on the GPU (include/j2k_hip.h: j2k_hip_compare), nothing but a few sums comes back.
    // out[c], c < buffer.channels: component c on its own grid -- error = decoded - source sample, at FileInfo.depth bits,
    // before any colour transform; firstX / firstY: the first differing sample in raster order (0, 0 when none differs);
    // psnr is +infinity when nothing differs.  SetReadLayers applies: a draft read's loss is the draft's.
    // true: out is filled.  false: a file for the fallback reader (status J2K_HIP_ERR_UNSUPPORTED); nothing is written -- the
    // fallback codec has no such call.  A file that is not this frame's (size, channels, depth, sub-sampling), a damaged
    // file and device failures throw "Error reading file"; LastError() names the field.
    struct Difference {
        unsigned long long samples, differing, sumAbs, sumSq;
        unsigned maxAbs, firstX, firstY;
        double mse, psnr;
    };
    bool Compare(InputFile &file, const FileInfo &info, const Buffer &buffer, Difference out[J2K_CODEC_MAX_CHANNELS]);

    // Draft reads: ReadFile, ReadRGBA and ReadFiles decode only the first `layers` quality layers of their files (0, the
    // initial value: all of them; a file with fewer layers is read in full) -- sample for sample what they deliver for the
    // file cut down to those layers, what libopenjp2 does for opj_dparameters_t::cp_layer (include/j2k_hip.h:
    // j2k_hip_decode_set_max_layers).  Tier-1, the longest stage of a read, shrinks with the coding passes that remain.  A file
    // handed to the fallback codec is read in full: the Codec interface has no such parameter.
    // Quality by rate-distortion slope (settings.method == QUALITY under HonourSettings): WriteFile writes n quality layers, layer
    // l holding of every code-block the coding passes whose distortion decrease per byte reaches slopes[l] (OpenJPEG's units;
    // a negative entry: everything that is left) -- include/j2k_hip.h: j2k_hip_params.layer_slopes.  One threshold held over a
    // shot gives constant quality: the bytes follow the content.  What number stands for which `quality` is the host's choice
    // (pick a slope on one frame with Compare, or take the ones a SIZE encode ended at: j2k_hip_encode_get_layer_slopes); this
    // codec does not invent a formula.  n = 0 (the initial state): QUALITY stays unmapped, the frame is written as without the
    // method.  At most J2K_CODEC_MAX_LAYERS entries are taken; the other methods ignore them.  The values are copied.
    void SetQualitySlopes(const double *slopes, unsigned n)
    {
        _quality_layers = slopes == NULL ? 0u : (n > J2K_CODEC_MAX_LAYERS ? (unsigned)J2K_CODEC_MAX_LAYERS : n);
        for (unsigned l = 0; l < _quality_layers; l++) _quality_slopes[l] = slopes[l];
    }
    unsigned QualityLayers() const { return _quality_layers; }

    void SetReadLayers(unsigned layers) { _read_layers = layers; }
    unsigned ReadLayers() const { return _read_layers; }

    // Cinema frames to R'G'B' (the read side of the CinemaXYZ options): a digital-cinema codestream holds X'Y'Z' code values and
    // names no colour space, so ReadRGBA hands them over as R, G, B.  target 1..3 (sRGB / Rec.709 under a 2.4 power / Rec.709
    // linear, as CinemaXYZ's sources; 0, the initial value: today's behaviour) makes ReadRGBA convert them in its output
    // kernel (include/j2k_hip.h: j2k_hip_decode_set_xyz_to_rgb).  profileFilesOnly: only files that carry the one mark a DCI
    // frame has -- Rsiz 3 or 4 in SIZ (j2k_hip_read_profile) -- are converted, every other file is read as without the setting;
    // false: every file ReadRGBA takes as RGB is converted, and one it takes as grey, palette or sYCC throws.  A target above 3
    // throws at the read.  ReadFile, ReadFiles and Compare are planar reads and do not convert.
    void SetReadCinemaColour(unsigned target, bool profileFilesOnly = true) { _read_xyz = target; _read_xyz_profile_only = profileFilesOnly; }
    unsigned ReadCinemaColour() const { return _read_xyz; }

    // text of the last failure on the calling thread (the exception itself carries the reference's
    // fixed message)
    static const char *LastError();

  private:
    Mode _mode;
    int _device;
    unsigned _options;
    Codec *_fallback;
    unsigned _read_layers;
    unsigned _read_xyz;
    bool _read_xyz_profile_only;
    double _quality_slopes[J2K_CODEC_MAX_LAYERS];
    unsigned _quality_layers;
};

} // namespace j2k
