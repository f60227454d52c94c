"""ctypes binding of the C ABI in include/j2k_hip.h (libj2k_hip.so).

This is harness plumbing for tests and bench.py; the product boundary is the C ABI itself and the
C++ `HipCodec` in j2k_amd/host/.  The binding fails loudly when the HIP library is missing -- there
is no CPU fallback.

torch is imported first (when present) so that this library binds to the same HIP runtime that
torch already loaded into the process.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

try:  # plumbing only: makes both libraries share one HIP runtime in-process
    import torch  # noqa: F401
except Exception:  # pragma: no cover
    torch = None

PKG = os.path.dirname(os.path.abspath(__file__))
LIBPATH = os.environ.get("J2K_HIP_LIB") or os.path.join(PKG, "libj2k_hip.so")  # (J2K_HIP_LIB: A/B runs of two builds on one box)


class J2kHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"j2k_hip error {code}: {msg}")
        self.code = code


class Params(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("channels", C.c_uint32), ("depth", C.c_uint32), ("reversible", C.c_uint32),
                ("ycc", C.c_uint32), ("layers", C.c_uint32), ("tile_size", C.c_uint32),
                ("num_resolutions", C.c_uint32), ("cblk_w", C.c_uint32), ("cblk_h", C.c_uint32),
                ("progression", C.c_uint32), ("promote_ae16", C.c_uint32), ("comment", C.c_char_p),
                ("file_format", C.c_uint32), ("color_space", C.c_uint32), ("alpha", C.c_uint32),
                ("alpha_premultiplied", C.c_uint32), ("icc_profile", C.c_void_p), ("icc_profile_len", C.c_size_t),
                ("layer_rates", C.POINTER(C.c_float)), ("layer_psnr", C.POINTER(C.c_float)),
                ("pixel_aspect_num", C.c_uint32), ("pixel_aspect_den", C.c_uint32), ("dpi", C.c_float),
                ("num_precincts", C.c_uint32), ("precinct_w", C.c_uint32 * 33), ("precinct_h", C.c_uint32 * 33),
                ("dci_profile", C.c_uint32), ("max_cs_size", C.c_uint32), ("max_comp_size", C.c_uint32),
                ("cblk_style", C.c_uint32),
                ("comp_sub_x", C.c_uint32 * 4), ("comp_sub_y", C.c_uint32 * 4), ("rgb_to_sycc", C.c_uint32),
                ("rgb_to_xyz", C.c_uint32), ("guard_bits", C.c_uint32),
                ("layer_slopes", C.POINTER(C.c_double))]


GUARD_AUTO = 0x100  # J2K_HIP_GUARD_AUTO: OR-ed with a floor of 0..7 (0 = 2)


class Plane(C.Structure):
    _fields_ = [("base", C.c_void_p), ("colbytes", C.c_ssize_t), ("rowbytes", C.c_ssize_t),
                ("sample_bits", C.c_uint32), ("depth", C.c_uint32)]


class FileInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("struct_size", "width", "height", "channels", "depth", "reversible", "ycc", "layers",
                                          "num_resolutions", "tile_width", "tile_height", "progression", "file_format",
                                          "color_space", "alpha", "alpha_premultiplied")] + \
               [("icc_profile_offset", C.c_size_t), ("icc_profile_len", C.c_size_t)] + \
               [(n, C.c_uint32 * 4) for n in ("sub_x", "sub_y", "comp_depth", "comp_signed")] + \
               [("lut_size", C.c_uint32), ("lut_channels", C.c_uint32), ("lut", (C.c_uint8 * 4) * 256), ("lut_column", C.c_uint8 * 4)]

    def as_dict(self):
        d = {n: (list(getattr(self, n)) if n in ("sub_x", "sub_y", "comp_depth", "comp_signed", "lut_column") else getattr(self, n))
             for n, _ in self._fields_ if n != "lut"}
        d["lut"] = [list(self.lut[i])[:self.lut_channels] for i in range(self.lut_size)]  # palette entries (JP2 pclr), [] without one
        return d


class OutPlane(C.Structure):
    _fields_ = [("base", C.c_void_p), ("colbytes", C.c_ssize_t), ("rowbytes", C.c_ssize_t), ("sample_bits", C.c_uint32),
                ("depth", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("ms_upload", "ms_frontend", "ms_dwt", "ms_t1", "ms_t2_host",
                                          "ms_assemble", "ms_download", "ms_total")] + \
               [("codestream_bytes", C.c_uint64), ("num_codeblocks", C.c_uint64), ("num_symbols", C.c_uint64),
                ("dwt_bytes", C.c_double), ("bands", C.c_uint32), ("reserved_", C.c_uint32), ("ms_after_upload", C.c_double),
                ("early_download_bytes", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


WRITE_FN = C.CFUNCTYPE(C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t)

EXPORTS = ["j2k_hip_abi_version", "j2k_hip_create", "j2k_hip_destroy", "j2k_hip_last_error", "j2k_hip_encode",
           "j2k_hip_encode_begin", "j2k_hip_encode_begin_borrowed", "j2k_hip_encode_end", "j2k_hip_debug_tune", "j2k_hip_debug_get_tune", "j2k_hip_debug_fused_occupancy", "j2k_hip_debug_membw", "j2k_hip_debug_dwt_time", "j2k_hip_read_info", "j2k_hip_decode",
           "j2k_hip_decode_device", "j2k_hip_decode_region", "j2k_hip_decode_region_device", "j2k_hip_region_footprint",
           "j2k_hip_rgba_mode", "j2k_hip_decode_rgba", "j2k_hip_decode_rgba_device", "j2k_hip_stage_rgba_output",
           "j2k_hip_decode_sequence_check", "j2k_hip_decode_sequence", "j2k_hip_decode_sequence_device",
           "j2k_hip_decode_rgba_sequence", "j2k_hip_decode_rgba_sequence_device", "j2k_hip_debug_decode_kernels",
           "j2k_hip_decode_set_max_layers", "j2k_hip_decode_get_max_layers", "j2k_hip_debug_decode_work",
           "j2k_hip_decode_set_xyz_to_rgb", "j2k_hip_decode_get_xyz_to_rgb", "j2k_hip_xyz_inverse_tables", "j2k_hip_read_profile",
           "j2k_hip_stage_rgba_output_xyz",
           "j2k_hip_compare_check", "j2k_hip_compare", "j2k_hip_compare_device", "j2k_hip_stage_compare",
           "j2k_hip_encode_tiles", "j2k_hip_device_count", "j2k_hip_encode_batch",
           "j2k_hip_encode_tiles_distributed", "j2k_hip_multi_last_error",
           "j2k_hip_encode_to_buffer", "j2k_hip_encode_device", "j2k_hip_encode_sequence_device", "j2k_hip_encode_tiles_device",
           "j2k_hip_main_header", "j2k_hip_file_header", "j2k_hip_xyz_tables", "j2k_hip_stage_frontend", "j2k_hip_stage_dwt", "j2k_hip_stage_dwt_regions", "j2k_hip_stage_t1", "j2k_hip_stage_t1_passes",
           "j2k_hip_stage_t1_styled", "j2k_hip_stage_t1_slots", "j2k_hip_stage_transform",
           "j2k_hip_stage_rate", "j2k_hip_stage_gather", "j2k_hip_stage_pack_offsets",
           "j2k_hip_stage_idwt", "j2k_hip_stage_idwt_window", "j2k_hip_stage_t1_decode", "j2k_hip_stage_t1_decode_styled", "j2k_hip_stage_decode_output",
           "j2k_hip_get_stats", "j2k_hip_get_dwt_level_ms", "j2k_hip_malloc", "j2k_hip_free",
           "j2k_hip_memcpy_h2d", "j2k_hip_memcpy_d2h", "j2k_hip_synchronize", "j2k_hip_debug_copy_sink", "j2k_hip_debug_count_sink",
           "j2k_hip_debug_cblk_capacities", "j2k_hip_debug_blocks", "j2k_hip_debug_tier2",
           "j2k_hip_encode_get_guard_bits", "j2k_hip_guard_bits_needed", "j2k_hip_debug_tier2_guard", "j2k_hip_debug_tier2_plan",
           "j2k_hip_encode_get_layer_slopes", "j2k_hip_stage_rate_layers",
           "j2k_hip_slope_grid", "j2k_hip_encode_sequence_budget_check", "j2k_hip_encode_sequence_budget_device",
           "j2k_hip_encode_sequence_budget",
           "j2k_hip_stage_rate_curve"]

SLOPE_K_MIN, SLOPE_K_MAX, SLOPE_ALL = -2048, 2047, -2049  # include/j2k_hip.h: the public grid of slope thresholds


class Budget(C.Structure):
    """include/j2k_hip.h: j2k_hip_budget."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("total_bytes", C.c_uint64), ("frame_max_bytes", C.c_uint64)]


class BudgetResult(C.Structure):
    """include/j2k_hip.h: j2k_hip_budget_result."""
    _fields_ = [("struct_size", C.c_uint32), ("shared_index", C.c_int32), ("total_bytes", C.c_uint64), ("capped_frames", C.c_uint32),
                ("curve_launches", C.c_uint32), ("exact_plans", C.c_uint32), ("reserved", C.c_uint32)]


def make_budget(total_bytes: int = 0, frame_max_bytes: int = 0) -> Budget:
    return Budget(C.sizeof(Budget), 0, total_bytes, frame_max_bytes)

class Tier2Plan(C.Structure):
    """include/j2k_hip.h: j2k_hip_tier2_plan."""
    _fields_ = [("total_len", C.c_uint64), ("guard_bits", C.c_uint32),
                ("blob_bytes", C.c_size_t), ("nheaders", C.c_size_t), ("ncblk_dst", C.c_size_t), ("nbodies", C.c_size_t),
                ("blob", C.c_void_p), ("blob_cap", C.c_size_t),
                ("hdr_dst", C.c_void_p), ("hdr_src", C.c_void_p), ("hdr_len", C.c_void_p), ("hdr_cap", C.c_size_t),
                ("cblk_dst", C.c_void_p), ("cblk_cap", C.c_size_t),
                ("body_dst", C.c_void_p), ("body_cblk", C.c_void_p), ("body_off", C.c_void_p), ("body_len", C.c_void_p), ("body_cap", C.c_size_t)]


class IdwtRegion(C.Structure):
    """include/j2k_hip.h: j2k_hip_idwt_region."""
    _fields_ = [(n, C.c_uint32) for n in ("x", "y", "w", "h", "x0", "y0")]


class Rect(C.Structure):
    """include/j2k_hip.h: j2k_hip_rect."""
    _fields_ = [(n, C.c_uint32) for n in ("x", "y", "w", "h")]


class DecBlock(C.Structure):
    """include/j2k_hip.h: j2k_hip_dec_block."""
    _fields_ = [(n, C.c_uint32) for n in ("x", "y", "w", "h", "orient", "numbps", "npasses", "roishift")] + \
               [("half_step", C.c_float), ("cw_len", C.c_uint32), ("cw_off", C.c_uint64)]


class OutComp(C.Structure):
    """include/j2k_hip.h: j2k_hip_outcomp."""
    _fields_ = [("offset", C.c_uint64), ("prec", C.c_uint32), ("sub_x", C.c_uint32), ("sub_y", C.c_uint32)]


class RgbaDst(C.Structure):
    """include/j2k_hip.h: j2k_hip_rgba_dst."""
    _fields_ = [("struct_size", C.c_uint32), ("r", OutPlane), ("g", OutPlane), ("b", OutPlane), ("a", OutPlane), ("demote_ae16", C.c_uint32)]


class RgbaStage(C.Structure):
    """include/j2k_hip.h: j2k_hip_rgba_stage."""
    _fields_ = [(n, C.c_uint32) for n in ("struct_size", "mode", "org_x", "org_y", "lut_size", "lut_columns")] + \
               [("lut", (C.c_uint8 * 4) * 256), ("lut_rgb", C.c_uint8 * 4)]


class RateScan(C.Structure):
    """include/j2k_hip.h: j2k_hip_rate_scan."""
    _fields_ = [("thresh", C.c_double), ("mode", C.c_uint32), ("slot", C.c_uint32)]


RATE_SCAN, RATE_SUMS_FETCH, RATE_SUMS_FETCH_LAST = 0, 1, 2  # J2K_HIP_RATE_*
# j2k_hip_rate_taken / j2k_hip_gather_piece as numpy records (the hooks take and fill arrays of them)
RATE_TAKEN = np.dtype([("lo", "<u8"), ("hi", "<u4"), ("n", "<u4")])
GATHER_PIECE = np.dtype([("dst", "<u8"), ("src", "<u8"), ("len", "<u4"), ("reserved", "<u4")])


class Diff(C.Structure):
    """include/j2k_hip.h: j2k_hip_diff -- one component of a compare."""
    _fields_ = [("struct_size", C.c_uint32), ("max_abs", C.c_uint32)] + \
               [(n, C.c_uint64) for n in ("samples", "differing", "sum_abs", "sum_sq")] + \
               [("first_x", C.c_uint32), ("first_y", C.c_uint32), ("mse", C.c_double), ("psnr", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "struct_size"}


class SeqFile(C.Structure):
    """include/j2k_hip.h: j2k_hip_file."""
    _fields_ = [("data", C.c_void_p), ("len", C.c_size_t)]


RGBA_RGB, RGBA_GREY, RGBA_PALETTE, RGBA_SYCC = 1, 2, 3, 4  # J2K_HIP_RGBA_*


class CopySink(C.Structure):
    """include/j2k_hip.h: j2k_hip_copy_sink -- the `user` of j2k_hip_debug_copy_sink."""
    _fields_ = [("dst", C.c_void_p), ("capacity", C.c_size_t), ("pos", C.c_size_t)]


def native_sink(L, copying: bool = True):
    """The write function (a WRITE_FN) of a sink that lives in the library -- no Python in the write path.  Its `user`
    argument is the caller's: a CopySink (copying) or a c_size_t that receives the byte count (counting)."""
    fn = C.cast(L.j2k_hip_debug_copy_sink if copying else L.j2k_hip_debug_count_sink, WRITE_FN)
    return fn


_lib = None


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIBPATH):
        raise OSError(f"{LIBPATH} is missing: build it with `python __graft_entry__.py` "
                      "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = C.CDLL(LIBPATH)
    L.j2k_hip_last_error.restype = C.c_char_p
    L.j2k_hip_last_error.argtypes = [C.c_void_p]
    L.j2k_hip_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    L.j2k_hip_destroy.argtypes = [C.c_void_p]
    L.j2k_hip_debug_fused_occupancy.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.j2k_hip_destroy.restype = None
    L.j2k_hip_encode.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Plane), WRITE_FN, C.c_void_p]
    L.j2k_hip_encode_begin.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Plane)]
    L.j2k_hip_encode_end.argtypes = [C.c_void_p, WRITE_FN, C.c_void_p]
    L.j2k_hip_encode_begin_borrowed.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Plane)]
    L.j2k_hip_debug_tune.argtypes = [C.c_char_p, C.c_int]
    L.j2k_hip_debug_get_tune.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
    L.j2k_hip_debug_membw.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.POINTER(C.c_double)]
    L.j2k_hip_encode_tiles.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Plane), C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t,
                                       C.POINTER(C.c_size_t)]
    L.j2k_hip_encode_batch.argtypes = [C.POINTER(C.c_int), C.c_uint32, C.c_uint32, C.POINTER(Params), C.POINTER(Plane), C.c_uint32,
                                       WRITE_FN, C.POINTER(C.c_void_p)]
    L.j2k_hip_encode_tiles_distributed.argtypes = [C.POINTER(C.c_int), C.c_uint32, C.POINTER(Params), C.POINTER(Plane), WRITE_FN, C.c_void_p]
    L.j2k_hip_multi_last_error.restype = C.c_char_p
    L.j2k_hip_read_info.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(FileInfo)]
    L.j2k_hip_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(OutPlane), C.c_uint32]
    L.j2k_hip_decode_device.argtypes = L.j2k_hip_decode.argtypes
    L.j2k_hip_decode_region.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(Rect), C.POINTER(OutPlane), C.c_uint32]
    L.j2k_hip_decode_region_device.argtypes = L.j2k_hip_decode_region.argtypes
    L.j2k_hip_region_footprint.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(Rect),
                                           C.POINTER(Rect), C.c_uint32]
    L.j2k_hip_stage_idwt_window.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                            C.POINTER(Rect), C.c_void_p, C.c_void_p]
    L.j2k_hip_debug_dwt_time.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)]
    L.j2k_hip_encode_to_buffer.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Plane), C.c_void_p, C.c_size_t,
                                           C.POINTER(C.c_size_t)]
    L.j2k_hip_encode_device.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Plane), C.POINTER(C.c_void_p),
                                        C.POINTER(C.c_size_t), C.c_void_p, C.c_size_t]
    L.j2k_hip_encode_sequence_device.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Plane), C.c_uint32,
                                                 C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.j2k_hip_encode_tiles_device.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Plane), C.c_uint32, C.c_uint32,
                                              C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p, C.c_size_t]
    L.j2k_hip_main_header.argtypes = [C.POINTER(Params), C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                      C.POINTER(C.c_uint32)]
    L.j2k_hip_file_header.argtypes = [C.POINTER(Params), C.c_uint64, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    if hasattr(L, "j2k_hip_xyz_tables"):  # (an earlier build loaded through J2K_HIP_LIB for an A/B run has none)
        L.j2k_hip_xyz_tables.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.j2k_hip_stage_frontend.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Plane), C.c_void_p]
    L.j2k_hip_stage_dwt.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                    C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_double)]
    if hasattr(L, "j2k_hip_stage_dwt_regions"):  # (an earlier build loaded through J2K_HIP_LIB for an A/B run has none)
        L.j2k_hip_stage_dwt_regions.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                C.POINTER(IdwtRegion), C.c_uint32, C.c_void_p, C.c_void_p]
    U32P = C.POINTER(C.c_uint32)
    L.j2k_hip_stage_transform.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Plane), U32P, U32P, C.c_uint32, C.c_int, C.c_void_p]
    L.j2k_hip_stage_t1.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, U32P, U32P, U32P, U32P, U32P,
                                   C.POINTER(C.c_float), U32P, U32P, U32P, C.POINTER(C.c_uint64), C.c_void_p, C.c_size_t]
    L.j2k_hip_stage_t1_passes.argtypes = L.j2k_hip_stage_t1.argtypes + [U32P, C.POINTER(C.c_int32)]
    L.j2k_hip_stage_t1_styled.argtypes = L.j2k_hip_stage_t1.argtypes + [U32P, C.c_uint32]
    L.j2k_hip_stage_t1_slots.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, U32P, U32P, U32P, U32P, U32P,
                                         C.POINTER(C.c_float), C.c_uint32, U32P, U32P, C.c_uint32, U32P, U32P, U32P, U32P, U32P, U32P,
                                         C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    L.j2k_hip_stage_rate.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 9 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                     C.c_void_p, C.POINTER(RateScan), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.j2k_hip_stage_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                       C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    L.j2k_hip_stage_pack_offsets.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]
    L.j2k_hip_stage_idwt.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                     C.POINTER(IdwtRegion), C.c_uint32, C.c_void_p, C.c_void_p]
    L.j2k_hip_stage_t1_decode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(DecBlock),
                                          C.c_void_p, C.c_size_t]
    L.j2k_hip_stage_t1_decode_styled.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(DecBlock), C.c_void_p,
                                                 C.c_size_t, C.c_uint32, U32P, U32P, U32P, C.c_uint32]
    L.j2k_hip_stage_decode_output.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32,
                                              C.POINTER(OutComp), C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(OutPlane), C.c_uint32]
    L.j2k_hip_rgba_mode.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]
    L.j2k_hip_decode_rgba.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(Rect), C.POINTER(RgbaDst)]
    L.j2k_hip_decode_rgba_device.argtypes = L.j2k_hip_decode_rgba.argtypes
    L.j2k_hip_stage_rgba_output.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32,
                                            C.POINTER(OutComp), C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(RgbaDst), C.POINTER(RgbaStage)]
    L.j2k_hip_decode_sequence_check.argtypes = [C.POINTER(SeqFile), C.c_uint32, C.POINTER(C.c_uint32)]
    L.j2k_hip_decode_sequence.argtypes = [C.c_void_p, C.POINTER(SeqFile), C.c_uint32, C.c_uint32, C.POINTER(Rect), C.POINTER(OutPlane), C.c_uint32]
    L.j2k_hip_decode_sequence_device.argtypes = L.j2k_hip_decode_sequence.argtypes
    L.j2k_hip_decode_rgba_sequence.argtypes = [C.c_void_p, C.POINTER(SeqFile), C.c_uint32, C.c_uint32, C.POINTER(Rect), C.POINTER(RgbaDst)]
    L.j2k_hip_decode_rgba_sequence_device.argtypes = L.j2k_hip_decode_rgba_sequence.argtypes
    L.j2k_hip_debug_decode_kernels.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.j2k_hip_debug_decode_work.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.j2k_hip_decode_set_max_layers.argtypes = [C.c_void_p, C.c_uint32]
    L.j2k_hip_decode_get_max_layers.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    if hasattr(L, "j2k_hip_decode_set_xyz_to_rgb"):  # (an earlier build loaded through J2K_HIP_LIB for an A/B run has none)
        L.j2k_hip_decode_set_xyz_to_rgb.argtypes = [C.c_void_p, C.c_uint32]
        L.j2k_hip_decode_get_xyz_to_rgb.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.j2k_hip_xyz_inverse_tables.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.j2k_hip_read_profile.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]
        L.j2k_hip_stage_rgba_output_xyz.argtypes = L.j2k_hip_stage_rgba_output.argtypes + [C.c_uint32]
    L.j2k_hip_compare_check.argtypes = [C.POINTER(Params), C.c_void_p, C.c_size_t]
    L.j2k_hip_compare.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Plane), C.c_void_p, C.c_size_t, C.POINTER(Diff), C.c_uint32]
    L.j2k_hip_compare_device.argtypes = L.j2k_hip_compare.argtypes
    L.j2k_hip_stage_compare.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Plane), C.c_void_p, C.POINTER(Diff), C.c_uint32]
    L.j2k_hip_get_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
    L.j2k_hip_get_dwt_level_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int]
    L.j2k_hip_malloc.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t]
    L.j2k_hip_free.argtypes = [C.c_void_p, C.c_void_p]
    L.j2k_hip_memcpy_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.j2k_hip_memcpy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.j2k_hip_synchronize.argtypes = [C.c_void_p]
    if hasattr(L, "j2k_hip_debug_tier2"):  # (an earlier build loaded through J2K_HIP_LIB for an A/B run has none)
        L.j2k_hip_debug_cblk_capacities.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.j2k_hip_debug_blocks.argtypes = [C.POINTER(Params), C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.j2k_hip_debug_tier2.argtypes = [C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_uint64)]
    if hasattr(L, "j2k_hip_guard_bits_needed"):
        L.j2k_hip_encode_get_guard_bits.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.j2k_hip_guard_bits_needed.argtypes = [C.POINTER(Params), C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]
        L.j2k_hip_debug_tier2_guard.argtypes = L.j2k_hip_debug_tier2.argtypes + [C.POINTER(C.c_uint32)]
    if hasattr(L, "j2k_hip_debug_tier2_plan"):
        L.j2k_hip_debug_tier2_plan.argtypes = [C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(Tier2Plan)]
    if hasattr(L, "j2k_hip_encode_get_layer_slopes"):
        L.j2k_hip_encode_get_layer_slopes.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        L.j2k_hip_stage_rate_layers.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32] + [C.c_void_p] * 5 + [C.c_uint32] + [C.c_void_p] * 4
    if hasattr(L, "j2k_hip_slope_grid"):
        L.j2k_hip_slope_grid.argtypes = [C.c_int32, C.POINTER(C.c_double)]
        L.j2k_hip_encode_sequence_budget_check.argtypes = [C.POINTER(Params), C.c_uint32, C.POINTER(Budget)]
        L.j2k_hip_encode_sequence_budget_device.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_uint32, C.POINTER(Budget), C.c_void_p, C.c_void_p,
                                                            C.c_void_p, C.POINTER(BudgetResult)]
        L.j2k_hip_encode_sequence_budget.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_uint32, C.POINTER(Budget), WRITE_FN, C.POINTER(C.c_void_p),
                                                     C.c_void_p, C.POINTER(BudgetResult)]
        L.j2k_hip_stage_rate_curve.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p, C.c_int32,
                                               C.c_uint32, C.c_uint32] + [C.c_void_p] * 3
    _lib = L
    return L


def tune(key: str, value: int):
    """Process-wide tuning knob of the library (j2k_hip_debug_tune); never changes an output byte."""
    L = load_library()
    if L.j2k_hip_debug_tune(key.encode(), int(value)) != 0:
        raise KeyError(key)


def get_tune(key: str) -> int:
    L = load_library()
    v = C.c_int()
    if L.j2k_hip_debug_get_tune(key.encode(), C.byref(v)) != 0:
        raise KeyError(key)
    return v.value


def read_info(data: bytes) -> dict:
    """Header of a raw codestream or JP2 file (j2k_hip_read_info; no device needed)."""
    L = load_library()
    fi = FileInfo()
    fi.struct_size = C.sizeof(FileInfo)
    buf = np.frombuffer(data, dtype=np.uint8)
    rc = L.j2k_hip_read_info(buf.ctypes.data, len(data), C.byref(fi))
    if rc != 0:
        raise J2kHipError(rc, L.j2k_hip_last_error(None).decode())
    return fi.as_dict()


def rgba_mode(data: bytes) -> int:
    """How the file's components become R, G, B, A (j2k_hip_rgba_mode: RGBA_RGB / _GREY / _PALETTE / _SYCC; no device needed)."""
    L = load_library()
    m = C.c_uint32()
    buf = np.frombuffer(data, dtype=np.uint8)
    rc = L.j2k_hip_rgba_mode(buf.ctypes.data, len(data), C.byref(m))
    if rc != 0:
        raise J2kHipError(rc, L.j2k_hip_last_error(None).decode())
    return m.value


def _seq_files(files):
    """The j2k_hip_file array of a list of bytes objects (and the arrays that keep the bytes alive)."""
    bufs = [np.frombuffer(d, dtype=np.uint8) if len(d) else np.zeros(0, np.uint8) for d in files]
    arr = (SeqFile * max(len(files), 1))()
    for f, b in enumerate(bufs):
        arr[f].data, arr[f].len = (b.ctypes.data if b.size else None), b.size
    return arr, bufs


def sequence_check(files) -> None:
    """May these files share one sequence decode call (j2k_hip_decode_sequence_check; headers only, no device needed)?
    Raises J2kHipError -- its text begins with "frame k: ", .frame is k -- when they may not."""
    L = load_library()
    arr, _keep = _seq_files(files)
    bad = C.c_uint32(0xffffffff)
    rc = L.j2k_hip_decode_sequence_check(arr, len(files), C.byref(bad))
    if rc != 0:
        err = J2kHipError(rc, L.j2k_hip_last_error(None).decode())
        err.frame = bad.value
        raise err


def _set_outplane(p, base, colbytes, rowbytes, sample_bits, depth, width, height):
    p.base, p.colbytes, p.rowbytes = base, colbytes, rowbytes
    p.sample_bits, p.depth, p.width, p.height = sample_bits, depth, width, height


def region_footprint(width: int, height: int, levels: int, reversible: bool, window, x0: int = 0, y0: int = 0, nrects: int | None = None):
    """Which coefficients of a Mallat plane a window (x, y, w, h) needs (j2k_hip_region_footprint; no device needed):
    [(x, y, w, h)] in plane coordinates for LL, then HL, LH, HH per level from the lowest resolution up."""
    L = load_library()
    n = 3 * levels + 1 if nrects is None else nrects
    rects = (Rect * max(n, 1))()
    rc = L.j2k_hip_region_footprint(int(reversible), width, height, levels, x0, y0, C.byref(Rect(*window)), rects, n)
    if rc != 0:
        raise J2kHipError(rc, L.j2k_hip_last_error(None).decode())
    return [(r.x, r.y, r.w, r.h) for r in rects[:n]]


def make_params(width, height, channels, depth, reversible=True, ycc=False, layers=1, tile_size=0,
                num_resolutions=6, cblk=(64, 64), promote=False, comment="", jp2=False, color_space=0,
                alpha_channel=-1, alpha_premultiplied=False, icc=None, rates=None, psnr=None, progression=0,
                pixel_aspect=None, dpi=0.0, precincts=None, dci_profile=0, max_cs_size=0, max_comp_size=0, cblk_style=0,
                sub=None, rgb_to_sycc=False, rgb_to_xyz=0, guard_bits=0, slopes=None):
    """comment: None -> library default COM, "" -> no COM segment.  jp2/color_space/alpha_channel/icc describe
    the JP2 file wrapper (color_space in OPJ_COLOR_SPACE numbering: 1 sRGB, 2 grey, 3 sYCC).
    sub = [(dx, dy), ...]: the sub-sampling factors of the components (SIZ XRsiz / YRsiz), one pair per channel; rgb_to_sycc:
    the planes are R, G, B[, A] of the full image and the library makes Y, Cb, Cr[, A] at those factors.  rgb_to_xyz: channels
    0..2 are R'G'B' (1 sRGB, 2 Rec.709 under a 2.4 power, 3 linear Rec.709) and the library makes cinema X'Y'Z' codes of them.
    guard_bits: 0 = two, strictly; 1..7 = that many, strictly; GUARD_AUTO | floor = as many as the frame needs, the floor at least.
    slopes: one rate-distortion slope threshold per layer (layer_slopes; negative = everything that is left); sets the layer count."""
    p = Params()
    p.struct_size = C.sizeof(Params)
    p.width, p.height, p.channels, p.depth = width, height, channels, depth
    p.reversible, p.ycc, p.layers, p.tile_size = int(reversible), int(ycc), layers, tile_size
    p.num_resolutions, p.cblk_w, p.cblk_h = num_resolutions, cblk[0], cblk[1]
    p.progression, p.promote_ae16 = progression, int(promote)
    p.comment = comment.encode() if comment is not None else None
    p.file_format, p.color_space = int(jp2), color_space
    p.alpha, p.alpha_premultiplied = alpha_channel + 1, int(alpha_premultiplied)
    if pixel_aspect:
        p.pixel_aspect_num, p.pixel_aspect_den = pixel_aspect
    p.dpi = dpi
    p.dci_profile, p.max_cs_size, p.max_comp_size = dci_profile, max_cs_size, max_comp_size  # 3 / 4: OpenJPEG's cinema 2K / 4K profile
    if sub is not None:
        for c, (dx, dy) in enumerate(sub):
            p.comp_sub_x[c], p.comp_sub_y[c] = dx, dy
    p.rgb_to_sycc = int(rgb_to_sycc)
    p.rgb_to_xyz = int(rgb_to_xyz)
    p.guard_bits = int(guard_bits)
    p.cblk_style = cblk_style  # COD SPcod code-block style: 1 bypass, 2 reset, 4 termall, 16 pterm, 32 segsym, in any combination
    if precincts:  # [(w, h), ...] highest resolution first (OpenJPEG's -c / res_spec semantics)
        p.num_precincts = len(precincts)
        for i, (pw, ph) in enumerate(precincts):
            p.precinct_w[i], p.precinct_h[i] = pw, ph
    if rates is not None:  # one compression ratio per layer (OpenJPEG tcp_rates); sets the layer count
        p.layers = len(rates)
        p._rates_keepalive = (C.c_float * len(rates))(*rates)
        p.layer_rates = C.cast(p._rates_keepalive, C.POINTER(C.c_float))
    if psnr is not None:  # one PSNR target (dB) per layer (OpenJPEG tcp_distoratio / cp_fixed_quality)
        p.layers = len(psnr)
        p._psnr_keepalive = (C.c_float * len(psnr))(*psnr)
        p.layer_psnr = C.cast(p._psnr_keepalive, C.POINTER(C.c_float))
    if slopes is not None:  # one slope threshold per layer, exact doubles (what Encoder.layer_slopes reports of a search)
        p.layers = len(slopes)
        p._slopes_keepalive = (C.c_double * len(slopes))(*slopes)
        p.layer_slopes = C.cast(p._slopes_keepalive, C.POINTER(C.c_double))
    if icc:
        p._icc_keepalive = C.create_string_buffer(bytes(icc), len(icc))  # borrowed by the C side for each call
        p.icc_profile, p.icc_profile_len = C.cast(p._icc_keepalive, C.c_void_p), len(icc)
    return p


def slope_grid(k: int) -> float:
    """j2k_hip_slope_grid: threshold k of the public grid, -1.0 for SLOPE_ALL; refused outside SLOPE_ALL..SLOPE_K_MAX."""
    L = load_library()
    t = C.c_double()
    if not -(1 << 31) <= k < (1 << 31):
        raise J2kHipError(1, "slope grid index outside the range")
    rc = L.j2k_hip_slope_grid(k, C.byref(t))
    if rc != 0:
        raise J2kHipError(rc, "slope grid index outside the range")
    return t.value


def sequence_budget_check(params: Params, nframes: int, budget: Budget) -> None:
    """j2k_hip_encode_sequence_budget_check: raises what Encoder.encode_sequence_budget_device would refuse before any device work."""
    L = load_library()
    rc = L.j2k_hip_encode_sequence_budget_check(C.byref(params), nframes, C.byref(budget))
    if rc != 0:
        raise J2kHipError(rc, L.j2k_hip_last_error(None).decode())


def main_header(params: Params) -> bytes:
    """SOC..QCD[,COM] of the codestream (what rank 0 of a tile-sharded job prepends)."""
    L = load_library()
    n, nt = C.c_size_t(), C.c_uint32()
    buf = C.create_string_buffer(70000)
    rc = L.j2k_hip_main_header(C.byref(params), buf, len(buf), C.byref(n), C.byref(nt))
    if rc != 0:
        raise J2kHipError(rc, L.j2k_hip_last_error(None).decode())
    return buf.raw[:n.value]


def xyz_tables(source: int, src_depth: int, dst_depth: int):
    """The tables of rgb_to_xyz as the kernel gets them (j2k_hip_xyz_tables; no device needed): (lin, thr, matrix) -- lin[v]
    the linear light of a src_depth-bit sample, thr[c - 1] the threshold of code c of dst_depth bits, matrix 3 x 3, all float32."""
    L = load_library()
    if not (1 <= src_depth <= 16 and 1 <= dst_depth <= 16):  # (the sizes of the arrays below)
        raise J2kHipError(1, "rgb_to_xyz tables: the depths must be 1..16")
    lin, thr = np.zeros(1 << src_depth, np.float32), np.zeros((1 << dst_depth) - 1, np.float32)
    m = np.zeros(9, np.float32)
    rc = L.j2k_hip_xyz_tables(source, src_depth, dst_depth, lin.ctypes.data, thr.ctypes.data if thr.size else None, m.ctypes.data)
    if rc != 0:
        raise J2kHipError(rc, L.j2k_hip_last_error(None).decode())
    return lin, thr, m.reshape(3, 3)


def xyz_inverse_tables(target: int, comp_depth: int, dst_depth: int):
    """The tables of xyz_to_rgb as the kernel gets them (j2k_hip_xyz_inverse_tables; no device needed): (dl, othr, matrix) --
    dl[c] of 2^comp_depth values, othr[k - 1] = the threshold of code k, the 3 x 3 matrix, all float32."""
    L = load_library()
    if not (1 <= comp_depth <= 16 and 1 <= dst_depth <= 16):
        raise J2kHipError(1, "xyz_to_rgb tables: the depths must be 1..16")
    dl, othr = np.zeros(1 << comp_depth, np.float32), np.zeros((1 << dst_depth) - 1, np.float32)
    m = np.zeros(9, np.float32)
    rc = L.j2k_hip_xyz_inverse_tables(target, comp_depth, dst_depth, dl.ctypes.data, othr.ctypes.data if othr.size else None, m.ctypes.data)
    if rc != 0:
        raise J2kHipError(rc, L.j2k_hip_last_error(None).decode())
    return dl, othr, m.reshape(3, 3)


def read_profile(data: bytes) -> int:
    """Rsiz of the codestream's SIZ segment (j2k_hip_read_profile; header only): 3 / 4 = the 2K / 4K digital cinema profiles."""
    L = load_library()
    v = C.c_uint32()
    buf = np.frombuffer(data, dtype=np.uint8)
    rc = L.j2k_hip_read_profile(buf.ctypes.data, len(data), C.byref(v))
    if rc != 0:
        raise J2kHipError(rc, L.j2k_hip_last_error(None).decode())
    return v.value


def cblk_capacities(area: int, Mb: int, cblk_style: int = 0):
    """(decision bytes, codeword bytes) of the slot a frame gives a code-block (j2k_hip_debug_cblk_capacities; no device needed)."""
    L = load_library()
    sym, out = C.c_uint64(), C.c_uint64()
    rc = L.j2k_hip_debug_cblk_capacities(area, Mb, cblk_style, C.byref(sym), C.byref(out))
    if rc != 0:
        raise J2kHipError(rc, L.j2k_hip_last_error(None).decode())
    return sym.value, out.value


BLOCK_COLUMNS = ("tile", "comp", "res", "band", "orient", "x", "y", "w", "h", "Mb")


def frame_blocks(params: Params) -> np.ndarray:
    """The code-blocks of a frame in the order of the encoder's tables, (n, 10) uint32 with the columns BLOCK_COLUMNS
    (j2k_hip_debug_blocks; no device needed)."""
    L = load_library()
    n = C.c_size_t()
    rc = L.j2k_hip_debug_blocks(C.byref(params), None, 0, C.byref(n))
    rows = np.zeros((n.value, len(BLOCK_COLUMNS)), np.uint32)
    if rc == 0:
        rc = L.j2k_hip_debug_blocks(C.byref(params), rows.ctypes.data, n.value, C.byref(n))
    if rc != 0:
        raise J2kHipError(rc, L.j2k_hip_last_error(None).decode())
    return rows


def host_tier2(params: Params, numbps, npasses, length, pricer: bool = False, with_guard: bool = False):
    """Host Tier-2 alone on per-block results in frame_blocks order (j2k_hip_debug_tier2; no device needed): the planned
    codestream's length, or with pricer the rate control's TilePricer of every tile (0).  Raises what an encode would.
    with_guard: (that, the guard bits the plan was made with) -- params.guard_bits is honoured, GUARD_AUTO included."""
    L = load_library()
    a = [np.ascontiguousarray(v, dtype=np.uint32) for v in (numbps, npasses, length)]
    assert a[0].shape == a[1].shape == a[2].shape and a[0].ndim == 1
    total, guard = C.c_uint64(), C.c_uint32()
    if with_guard:
        rc = L.j2k_hip_debug_tier2_guard(C.byref(params), a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[0].size, int(pricer),
                                         C.byref(total), C.byref(guard))
    else:
        rc = L.j2k_hip_debug_tier2(C.byref(params), a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[0].size, int(pricer), C.byref(total))
    if rc != 0:
        raise J2kHipError(rc, L.j2k_hip_last_error(None).decode())
    return (total.value, guard.value) if with_guard else total.value


MAX_PASSES = 96  # J2K_HIP_MAX_PASSES: the row length of the per-pass tables


def host_tier2_plan(params: Params, numbps, npasses, length, rates=None, alloc=None, workers: int = 0) -> dict:
    """Host Tier-2's plan of per-block results in frame_blocks order (j2k_hip_debug_tier2_plan; no device needed).  rates:
    (n, MAX_PASSES) bytes at the end of every pass, required under a code-block style and refused without one; alloc: (np, len,
    off), each (n, layers), a layer allocation; workers: 0 plans serially, n with n threads.  params.guard_bits is honoured as by
    host_tier2.  Returns dict(total_len, guard_bits, blob, headers = (dst, src, len) arrays, cblk_dst (no allocation) or None,
    bodies = (dst, cblk, off, len) arrays (with one) or None, length = the blocks' lengths as given, which assemble() needs
    beside cblk_dst); assemble() lays it out."""
    L = load_library()
    a = [np.ascontiguousarray(v, dtype=np.uint32) for v in (numbps, npasses, length)]
    assert a[0].shape == a[1].shape == a[2].shape and a[0].ndim == 1
    n = a[0].size
    ptr = lambda v: v.ctypes.data if v is not None and v.size else None
    r = None
    if rates is not None:
        r = np.ascontiguousarray(rates, dtype=np.uint32)
        assert r.shape == (n, MAX_PASSES)
    al, layers = [None, None, None], 0
    if alloc is not None:
        al = [np.ascontiguousarray(v, dtype=np.uint32) for v in alloc]
        assert al[0].ndim == 2 and al[0].shape[0] == n and al[0].shape == al[1].shape == al[2].shape
        layers = al[0].shape[1]
    out = Tier2Plan()

    def call():
        rc = L.j2k_hip_debug_tier2_plan(C.byref(params), a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, n, ptr(r), ptr(al[0]), ptr(al[1]),
                                        ptr(al[2]), layers, workers, C.byref(out))
        if rc != 0:
            raise J2kHipError(rc, L.j2k_hip_last_error(None).decode())

    call()  # sizes
    blob = np.zeros(max(1, out.blob_bytes), np.uint8)
    hd, hs, hl = np.zeros(max(1, out.nheaders), np.uint64), np.zeros(max(1, out.nheaders), np.uint32), np.zeros(max(1, out.nheaders), np.uint32)
    cd = np.zeros(max(1, out.ncblk_dst), np.uint64)
    bd = np.zeros(max(1, out.nbodies), np.uint64)
    bc, bo, bl = (np.zeros(max(1, out.nbodies), np.uint32) for _ in range(3))
    out.blob, out.blob_cap = blob.ctypes.data, blob.size
    out.hdr_dst, out.hdr_src, out.hdr_len, out.hdr_cap = hd.ctypes.data, hs.ctypes.data, hl.ctypes.data, hd.size
    out.cblk_dst, out.cblk_cap = cd.ctypes.data, cd.size
    out.body_dst, out.body_cblk, out.body_off, out.body_len, out.body_cap = bd.ctypes.data, bc.ctypes.data, bo.ctypes.data, bl.ctypes.data, bd.size
    call()
    nh, nbd = out.nheaders, out.nbodies
    return dict(total_len=int(out.total_len), guard_bits=int(out.guard_bits), blob=blob[:out.blob_bytes],
                headers=(hd[:nh], hs[:nh], hl[:nh]),
                cblk_dst=cd[:out.ncblk_dst] if alloc is None else None,
                bodies=(bd[:nbd], bc[:nbd], bo[:nbd], bl[:nbd]) if alloc is not None else None,
                length=a[2])


def assemble(plan: dict, block_bytes) -> bytes:
    """The codestream of a host_tier2_plan: the blob's pieces and the blocks' bytes (block_bytes[i]: bytes or uint8 array of
    block i, frame_blocks order) laid where the plan puts them.  Every byte of the stream must be written exactly once."""
    total = plan["total_len"]
    out = np.zeros(total, np.uint8)
    seen = np.zeros(total, np.uint8)

    def put(dst, src):
        out[dst:dst + len(src)] = src
        seen[dst:dst + len(src)] += 1

    blob = plan["blob"]
    for d, s, ln in zip(*plan["headers"]):
        assert int(d) + int(ln) <= total and int(s) + int(ln) <= blob.size
        put(int(d), blob[int(s):int(s) + int(ln)])
    blocks = [np.frombuffer(bytes(b), np.uint8) for b in block_bytes]
    if plan["bodies"] is None:
        for i, d in enumerate(plan["cblk_dst"]):
            ln = int(plan["length"][i])
            assert blocks[i].size == ln and int(d) + ln <= total
            put(int(d), blocks[i])
    else:
        for d, c, o, ln in zip(*plan["bodies"]):
            assert int(o) + int(ln) <= blocks[int(c)].size and int(d) + int(ln) <= total
            put(int(d), blocks[int(c)][int(o):int(o) + int(ln)])
    if not np.all(seen == 1):
        raise AssertionError("Tier-2 plan: its pieces do not tile the codestream")
    return out.tobytes()


def guard_bits_needed(params: Params, numbps) -> int:
    """The smallest guard-bit count at or above the one `params` ask for that holds blocks of `numbps` bit-planes, frame_blocks
    order (j2k_hip_guard_bits_needed; no device needed): the rule an encode under GUARD_AUTO uses."""
    L = load_library()
    a = np.ascontiguousarray(numbps, dtype=np.uint32)
    g = C.c_uint32()
    rc = L.j2k_hip_guard_bits_needed(C.byref(params), a.ctypes.data, a.size, C.byref(g))
    if rc != 0:
        raise J2kHipError(rc, L.j2k_hip_last_error(None).decode())
    return g.value


def file_header(params: Params, codestream_len: int) -> bytes:
    """Bytes that precede the codestream in the output file (JP2 boxes; empty for raw J2K)."""
    L = load_library()
    n = C.c_size_t()
    buf = C.create_string_buffer(4096 + int(params.icc_profile_len))
    rc = L.j2k_hip_file_header(C.byref(params), codestream_len, buf, len(buf), C.byref(n))
    if rc != 0:
        raise J2kHipError(rc, L.j2k_hip_last_error(None).decode())
    return buf.raw[:n.value]


_SAMPLE_DTYPES = (np.uint8, np.uint16, np.float32)


def _sample_dtype(bits: int):
    """numpy type of a sample_bits value: 8 / 16-bit unsigned integers, 32 = IEEE binary32 of nominal range 0..1."""
    return {8: np.uint8, 16: np.uint16, 32: np.float32}[bits]


def _layout_depth(layout: dict) -> int:
    """Channel.depth of an AE frame's samples: the sample type's bits; a float frame (sample_bytes 4, synth.ae_frame_float)
    stands for integers of layout["depth"] bits (default 16)."""
    sb = layout["sample_bytes"]
    return layout.get("depth", 16) if sb == 4 else 8 * sb


def _array_depth(a: np.ndarray) -> int:
    return 16 if a.dtype == np.float32 else 8 * a.itemsize


def planes_from_layout(base_addr: int, layout: dict, channels: int, depth_bits: int | None = None):
    """Channel views (R,G,B[,A] = codec channels 0..) over an AE ARGB frame (see synth.ae_frame; sample_bytes 4: an ARGB128
    frame of floats, synth.ae_frame_float)."""
    sb = layout["sample_bytes"]
    offs = layout["channel_offsets"]  # A,R,G,B
    order = [offs[1], offs[2], offs[3], offs[0]]
    arr = (Plane * channels)()
    for c in range(channels):
        arr[c].base = base_addr + order[c]
        arr[c].colbytes = layout["colbytes"]
        arr[c].rowbytes = layout["rowbytes"]
        arr[c].sample_bits = 8 * sb
        arr[c].depth = depth_bits if depth_bits is not None else _layout_depth(layout)
    return arr


def comp_shapes(params: Params):
    """(rows, columns) of every component of `params` on its own grid: ceil(height / sub_y) x ceil(width / sub_x)."""
    return [(-(-params.height // max(params.comp_sub_y[c], 1)), -(-params.width // max(params.comp_sub_x[c], 1)))
            for c in range(params.channels)]


def planes_from_arrays(arrays, depth_bits: int, base_of=None):
    """Channel views over a list of 2-D uint8 / uint16 / float32 arrays of any sizes and strides (the components of a sub-sampled image,
    one array each; padded rows, samples of interleaved pixels).  depth_bits: the significant bits of the samples.
    base_of: array index -> address of its first sample (default: the array's own host address; a device copy otherwise)."""
    arr = (Plane * len(arrays))()
    for c, a in enumerate(arrays):
        assert a.ndim == 2 and a.dtype in _SAMPLE_DTYPES
        arr[c].base = base_of(c) if base_of else a.ctypes.data
        arr[c].colbytes, arr[c].rowbytes = a.strides[1], a.strides[0]
        arr[c].sample_bits, arr[c].depth = 8 * a.itemsize, depth_bits
    return arr


def _split_comps(raw: np.ndarray, params: Params):
    """The dense 32-bit words of a stage hook -> (channels, H, W) for components of one size, a list of 2-D arrays otherwise."""
    dt = np.int32 if params.reversible else np.float32
    shapes = comp_shapes(params)
    words = raw.view(dt)
    if all(s == shapes[0] for s in shapes):
        return words.reshape(params.channels, params.height, params.width)
    out, pos = [], 0
    for (h, w) in shapes:
        out.append(words[pos:pos + h * w].reshape(h, w))
        pos += h * w
    return out


def compare_check(params: Params, data: bytes) -> None:
    """Does the file describe the image of `params` (j2k_hip_compare_check: width, height, channels, depth, sub-sampling,
    unsigned components; headers only, no device needed)?  Raises J2kHipError when it does not."""
    L = load_library()
    buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(0, np.uint8)
    rc = L.j2k_hip_compare_check(C.byref(params), buf.ctypes.data if buf.size else None, buf.size)
    if rc != 0:
        raise J2kHipError(rc, L.j2k_hip_last_error(None).decode())


def _source_views(params: Params, frame=None, layout=None, planar=None, comps=None, views=None):
    """A source frame, given the way the encode_* methods take it, as (buffer, address of the buffer -> Plane array):
    frame + layout (an AE frame, encode_host), planar = (channels, h, w) samples (encode_planar_host), comps = one 2-D array
    per component (encode_components_host), or views = (buffer, callable) for any other channel views."""
    if views is not None:
        return views
    if frame is not None:
        return frame, lambda a: planes_from_layout(a, layout, params.channels)
    dt = np.uint16 if params.depth > 8 else np.uint8
    arrs = [np.ascontiguousarray(np.asarray(c).astype(dt)) for c in (planar if planar is not None else comps)]
    offs, pos = [], 0
    for a in arrs:  # (every plane at a multiple of 16 bytes of one buffer)
        offs.append(pos)
        pos += -(-a.nbytes // 16) * 16
    buf = np.zeros(max(pos, 16), np.uint8)
    for a, o in zip(arrs, offs):
        buf[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
    return buf, lambda addr: planes_from_arrays(arrs, params.depth, base_of=lambda c: addr + offs[c])


class Encoder:
    """Thin RAII wrapper over a j2k_hip_encoder handle."""

    def __init__(self, device: int = 0):
        self.L = load_library()
        self.h = C.c_void_p()
        rc = self.L.j2k_hip_create(C.byref(self.h), device)
        if rc != 0:
            raise J2kHipError(rc, self.L.j2k_hip_last_error(None).decode())

    def close(self):
        if getattr(self, "h", None) and self.h:
            self.L.j2k_hip_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise J2kHipError(rc, self.L.j2k_hip_last_error(self.h).decode())

    # -- memory -----------------------------------------------------------------------------------
    def malloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self._check(self.L.j2k_hip_malloc(self.h, C.byref(p), nbytes))
        return p.value

    def free(self, dptr: int):
        self._check(self.L.j2k_hip_free(self.h, dptr))

    def h2d(self, dptr: int, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        self._check(self.L.j2k_hip_memcpy_h2d(self.h, dptr, arr.ctypes.data, arr.nbytes))

    def d2h(self, dptr: int, nbytes: int) -> np.ndarray:
        out = np.empty(nbytes, dtype=np.uint8)
        self._check(self.L.j2k_hip_memcpy_d2h(self.h, out.ctypes.data, dptr, nbytes))
        return out

    def upload(self, arr: np.ndarray) -> int:
        arr = np.ascontiguousarray(arr)
        d = self.malloc(max(arr.nbytes, 16))
        self.h2d(d, arr)
        return d

    def synchronize(self):
        self._check(self.L.j2k_hip_synchronize(self.h))

    # -- encode -----------------------------------------------------------------------------------
    def encode_host(self, frame: np.ndarray, layout: dict, params: Params, via_sink: bool = False) -> bytes:
        planes = planes_from_layout(frame.ctypes.data, layout, params.channels)
        return self._encode_planes_host(planes, frame.nbytes, params, via_sink)

    def encode_planar_host(self, planes_arr: np.ndarray, params: Params, via_sink: bool = False) -> bytes:
        """planes_arr: (channels, h, w) unsigned samples -> planar host buffers of 8- or 16-bit samples."""
        dt = np.uint16 if params.depth > 8 else np.uint8
        buf = np.ascontiguousarray(planes_arr.astype(dt))
        nc, h, w = buf.shape
        arr = (Plane * nc)()
        for c in range(nc):
            arr[c].base = buf.ctypes.data + c * h * w * buf.itemsize
            arr[c].colbytes, arr[c].rowbytes = buf.itemsize, w * buf.itemsize
            arr[c].sample_bits, arr[c].depth = 8 * buf.itemsize, params.depth  # samples already hold `depth` bits
        return self._encode_planes_host(arr, buf.nbytes, params, via_sink)

    def encode_components_host(self, comps, params: Params, via_sink: bool = False) -> bytes:
        """comps: one 2-D array of unsigned samples per component, each of its own size (sub-sampled components) -> planar host
        buffers of 8- or 16-bit samples, encoded through j2k_hip_encode_to_buffer (via_sink: j2k_hip_encode)."""
        dt = np.uint16 if params.depth > 8 else np.uint8
        bufs = [np.ascontiguousarray(np.asarray(c).astype(dt)) for c in comps]
        return self._encode_planes_host(planes_from_arrays(bufs, params.depth), sum(b.nbytes for b in bufs), params, via_sink)

    def _encode_planes_host(self, planes, in_bytes: int, params: Params, via_sink: bool) -> bytes:
        if via_sink:
            chunks = []

            @WRITE_FN
            def sink(user, buf, n):
                chunks.append(C.string_at(buf, n))
                return n
            self._check(self.L.j2k_hip_encode(self.h, C.byref(params), planes, sink, None))
            return b"".join(chunks)
        cap = in_bytes * 2 + (1 << 20) + int(params.icc_profile_len)
        out = np.empty(cap, dtype=np.uint8)
        n = C.c_size_t()
        self._check(self.L.j2k_hip_encode_to_buffer(self.h, C.byref(params), planes, out.ctypes.data, cap, C.byref(n)))
        return out[:n.value].tobytes()

    def encode_begin_host(self, frame: np.ndarray, layout: dict, params: Params):
        """First half of j2k_hip_encode (j2k_hip_encode_begin): returns once the frame has left `frame`."""
        planes = planes_from_layout(frame.ctypes.data, layout, params.channels)
        self._check(self.L.j2k_hip_encode_begin(self.h, C.byref(params), planes))

    def encode_begin_borrowed(self, frame: np.ndarray, layout: dict, params: Params):
        """j2k_hip_encode_begin_borrowed: returns at once; `frame` and `params` must stay as they are until encode_end()."""
        planes = planes_from_layout(frame.ctypes.data, layout, params.channels)
        self._borrowed = (frame, params, planes)  # (kept alive on the caller's behalf)
        self._check(self.L.j2k_hip_encode_begin_borrowed(self.h, C.byref(params), planes))

    def encode_end(self) -> bytes:
        """Second half (j2k_hip_encode_end): the finished file through the sink callback."""
        chunks = []

        @WRITE_FN
        def sink(user, buf, n):
            chunks.append(C.string_at(buf, n))
            return n
        self._check(self.L.j2k_hip_encode_end(self.h, sink, None))
        return b"".join(chunks)

    def encode_device(self, d_frame: int, layout: dict, params: Params, download: bool = True):
        """Returns (device_ptr, length, bytes or None)."""
        planes = planes_from_layout(d_frame, layout, params.channels)
        dptr, n = C.c_void_p(), C.c_size_t()
        self._check(self.L.j2k_hip_encode_device(self.h, C.byref(params), planes, C.byref(dptr), C.byref(n), None, 0))
        data = self.d2h(dptr.value, n.value).tobytes() if download else None
        return dptr.value, n.value, data

    def encode_sequence_device(self, d_frames: list, layout: dict, params: Params, download: bool = True):
        """Frames of one sequence (device pointers, same layout) in one call -> [(device_ptr, length, bytes or None)]."""
        nf, nc = len(d_frames), params.channels
        arr = (Plane * (nf * nc))()
        for f, d in enumerate(d_frames):
            one = planes_from_layout(d, layout, nc)
            for c in range(nc):
                arr[f * nc + c] = one[c]
        ptrs, lens = (C.c_void_p * nf)(), (C.c_size_t * nf)()
        self._check(self.L.j2k_hip_encode_sequence_device(self.h, C.byref(params), arr, nf, ptrs, lens))
        return [(ptrs[f], lens[f], self.d2h(ptrs[f], lens[f]).tobytes() if download else None) for f in range(nf)]

    def encode_sequence_budget_device(self, d_frames: list, layout: dict, params: Params, total_bytes: int = 0, frame_max_bytes: int = 0,
                                      budget: Budget | None = None, outputs=None, download: bool = True):
        """j2k_hip_encode_sequence_budget_device: the frames of one shot (device pointers, same layout) to a byte budget ->
        (files [bytes], frame_index [int], result dict).  outputs = (ptrs, lens, index) ctypes arrays to pass instead of fresh ones."""
        nf, nc = len(d_frames), params.channels
        arr = (Plane * (nf * nc))()
        for f, d in enumerate(d_frames):
            one = planes_from_layout(d, layout, nc)
            for c in range(nc):
                arr[f * nc + c] = one[c]
        ptrs, lens, index = outputs if outputs else ((C.c_void_p * nf)(), (C.c_size_t * nf)(), (C.c_int32 * nf)())
        b = budget if budget is not None else make_budget(total_bytes, frame_max_bytes)
        res = BudgetResult(struct_size=C.sizeof(BudgetResult))
        self._check(self.L.j2k_hip_encode_sequence_budget_device(self.h, C.byref(params), arr, nf, C.byref(b), ptrs, lens, index, C.byref(res)))
        files = [self.d2h(ptrs[f], lens[f]).tobytes() if download else int(lens[f]) for f in range(nf)]  # (not downloaded: the lengths)
        return files, [int(v) for v in index], {k: int(getattr(res, k)) for k, _ in BudgetResult._fields_ if k not in ("struct_size", "reserved")}

    def encode_sequence_budget(self, frames: list, layout: dict, params: Params, total_bytes: int = 0, frame_max_bytes: int = 0,
                               budget: Budget | None = None, capacity: int | None = None, fill: int = 0):
        """j2k_hip_encode_sequence_budget: the same from host frames (AE-layout buffers), every file into a copy sink of its own ->
        (files [bytes], frame_index [int], result dict, sinks [(buffer, bytes written)]).  The sinks' buffers (capacity bytes
        each, filled with `fill` first) come back too, so that a failed call can be shown to have written nothing: on failure the
        J2kHipError carries them as .sinks."""
        nf, nc = len(frames), params.channels
        arr = (Plane * (nf * nc))()
        for f, fr in enumerate(frames):
            one = planes_from_layout(fr.ctypes.data, layout, nc)
            for c in range(nc):
                arr[f * nc + c] = one[c]
        cap = capacity if capacity is not None else max(int(fr.nbytes) for fr in frames) * 2 + (1 << 20)
        bufs = [np.full(cap, fill, np.uint8) for _ in range(nf)]
        sinks = [CopySink(b.ctypes.data, cap, 0) for b in bufs]
        users = (C.c_void_p * nf)(*[C.cast(C.pointer(sk), C.c_void_p) for sk in sinks])
        index = (C.c_int32 * nf)(*([fill] * nf))
        b = budget if budget is not None else make_budget(total_bytes, frame_max_bytes)
        res = BudgetResult(struct_size=C.sizeof(BudgetResult))
        try:
            self._check(self.L.j2k_hip_encode_sequence_budget(self.h, C.byref(params), arr, nf, C.byref(b), native_sink(self.L), users, index, C.byref(res)))
        except J2kHipError as x:
            x.sinks = [(bufs[f], int(sinks[f].pos)) for f in range(nf)]
            x.index = [int(v) for v in index]
            raise
        files = [bufs[f][:sinks[f].pos].tobytes() for f in range(nf)]
        return files, [int(v) for v in index], {k: int(getattr(res, k)) for k, _ in BudgetResult._fields_ if k not in ("struct_size", "reserved")}

    def encode_tiles_device(self, d_frame: int, layout: dict, params: Params, tile_first: int, tile_count: int):
        planes = planes_from_layout(d_frame, layout, params.channels)
        dptr, n = C.c_void_p(), C.c_size_t()
        self._check(self.L.j2k_hip_encode_tiles_device(self.h, C.byref(params), planes, tile_first, tile_count,
                                                       C.byref(dptr), C.byref(n), None, 0))
        return self.d2h(dptr.value, n.value).tobytes()

    def encode_tiles_host(self, planes, params: Params, tile_first: int, tile_count: int) -> bytes:
        """j2k_hip_encode_tiles: the tile-parts of a tile range from host memory.  planes: a Plane array of any channel views
        (planes_from_layout, planes_from_arrays, bottom-up rows); only the rows of the range's tiles are read."""
        cap = 4 * params.width * params.height * params.channels + (1 << 20)
        out = np.empty(cap, dtype=np.uint8)
        n = C.c_size_t()
        self._check(self.L.j2k_hip_encode_tiles(self.h, C.byref(params), planes, tile_first, tile_count, out.ctypes.data, cap, C.byref(n)))
        return out[:n.value].tobytes()

    # -- decode -----------------------------------------------------------------------------------
    def decode_planar(self, data: bytes, subsample: int = 1, sample_bits: int | None = None, depth: int | None = None,
                      channels: int | None = None, out: np.ndarray | None = None) -> np.ndarray:
        """Decode into planar host buffers: (channels, ceil(h / subsample), ceil(w / subsample)) of uint8 / uint16.
        depth = Channel.depth of the destination (default: the file's precision in the smallest fitting sample type).
        out: a buffer of that shape to decode into (a host that decodes frame after frame keeps its buffers)."""
        i = read_info(data)
        nc = channels or i["channels"]
        red = max(subsample, 1).bit_length() - 1
        w, h = -(-i["width"] >> red), -(-i["height"] >> red)
        bits = sample_bits or (8 if i["depth"] <= 8 else 16)
        if out is None:
            out = np.zeros((nc, h, w), dtype=_sample_dtype(bits))
        assert out.shape == (nc, h, w) and out.itemsize * 8 == bits and out.flags.c_contiguous
        arr = (OutPlane * nc)()
        for c in range(nc):
            arr[c].base = out.ctypes.data + c * h * w * out.itemsize
            arr[c].colbytes, arr[c].rowbytes = out.itemsize, w * out.itemsize
            arr[c].sample_bits, arr[c].depth = bits, depth or min(i["depth"], 16, bits)
            arr[c].width, arr[c].height = w, h
        buf = np.frombuffer(data, dtype=np.uint8)
        self._check(self.L.j2k_hip_decode(self.h, buf.ctypes.data, len(data), subsample, arr, nc))
        return out

    def decode_region_planar(self, data: bytes, rect, subsample: int = 1, sample_bits: int | None = None, depth: int | None = None,
                             channels: int | None = None, out: np.ndarray | None = None, device: bool = False) -> np.ndarray:
        """Decode the window rect = (x, y, w, h) of the image decode_planar delivers at this subsample into planar buffers
        (channels, h, w); out: a buffer to decode into, (channels, rows, cols) of any size -- it receives the window's
        top-left part.  device=True: through a device copy of the buffer (j2k_hip_decode_region_device)."""
        i = read_info(data)
        nc = channels or i["channels"]
        bits = sample_bits or (8 if i["depth"] <= 8 else 16)
        if out is None:
            out = np.zeros((nc, rect[3], rect[2]), dtype=_sample_dtype(bits))
        assert out.ndim == 3 and out.shape[0] == nc and out.itemsize * 8 == bits and out.flags.c_contiguous
        _, h, w = out.shape
        d = self.upload(out) if device else None
        base = d if device else out.ctypes.data
        arr = (OutPlane * nc)()
        for c in range(nc):
            arr[c].base = base + c * h * w * out.itemsize
            arr[c].colbytes, arr[c].rowbytes = out.itemsize, w * out.itemsize
            arr[c].sample_bits, arr[c].depth = bits, depth or min(i["depth"], 16, bits)
            arr[c].width, arr[c].height = w, h
        buf = np.frombuffer(data, dtype=np.uint8)
        try:
            fn = self.L.j2k_hip_decode_region_device if device else self.L.j2k_hip_decode_region
            self._check(fn(self.h, buf.ctypes.data, len(data), subsample, C.byref(Rect(*rect)), arr, nc))
            if device:
                out[...] = self.d2h(d, out.nbytes).view(out.dtype).reshape(out.shape)
        finally:
            if d:
                self.free(d)
        return out

    def decode_channels(self, data: bytes, chans: list, depth: int | None = None, subsample: int = 1):
        """Decode into one 2-D numpy view per codec channel, wherever each lies and whatever its strides (padded rows,
        samples of interleaved pixels, bottom-up rows): the general form of the C ABI's destination."""
        arr = (OutPlane * len(chans))()
        for c, a in enumerate(chans):
            assert a.ndim == 2 and a.dtype in _SAMPLE_DTYPES
            arr[c].base = a.ctypes.data
            arr[c].colbytes, arr[c].rowbytes = a.strides[1], a.strides[0]
            arr[c].sample_bits, arr[c].depth = 8 * a.itemsize, depth or _array_depth(a)
            arr[c].width, arr[c].height = a.shape[1], a.shape[0]
        buf = np.frombuffer(data, dtype=np.uint8)
        self._check(self.L.j2k_hip_decode(self.h, buf.ctypes.data, len(data), subsample, arr, len(chans)))

    def decode_ae(self, data: bytes, frame: np.ndarray, layout: dict, width: int, height: int, channels: int, depth: int | None = None,
                  subsample: int = 1, device: bool = False, region=None):
        """Decode into an After Effects ARGB frame (see synth.ae_frame): codec channels R,G,B[,A] go to their samples,
        every other byte of `frame` must stay as it is.  device=True: through a device copy of the frame.
        region = (x, y, w, h): that window of the image goes to the frame's top-left (j2k_hip_decode_region)."""
        sb = layout["sample_bytes"]
        offs = layout["channel_offsets"]
        order = [offs[1], offs[2], offs[3], offs[0]]
        base = frame.ctypes.data
        d = None
        if device:
            d = self.upload(frame)
            base = d
        arr = (OutPlane * channels)()
        for c in range(channels):
            arr[c].base = base + order[c]
            arr[c].colbytes, arr[c].rowbytes = layout["colbytes"], layout["rowbytes"]
            arr[c].sample_bits, arr[c].depth = 8 * sb, depth or _layout_depth(layout)
            arr[c].width, arr[c].height = width, height
        buf = np.frombuffer(data, dtype=np.uint8)
        try:
            if region is not None:
                fn = self.L.j2k_hip_decode_region_device if device else self.L.j2k_hip_decode_region
                self._check(fn(self.h, buf.ctypes.data, len(data), subsample, C.byref(Rect(*region)), arr, channels))
            elif device:
                self._check(self.L.j2k_hip_decode_device(self.h, buf.ctypes.data, len(data), subsample, arr, channels))
            else:
                self._check(self.L.j2k_hip_decode(self.h, buf.ctypes.data, len(data), subsample, arr, channels))
            if device:
                frame[:] = self.d2h(d, frame.nbytes)
        finally:
            if d:
                self.free(d)
        return frame

    def decode_rgba(self, data: bytes, frame: np.ndarray, layout: dict, width: int, height: int, depth: int | None = None,
                    subsample: int = 1, region=None, demote: bool = False, device: bool = False, alpha: bool = True):
        """Decode straight into the R, G, B, A samples of an After Effects ARGB frame (see synth.ae_frame; j2k_hip_decode_rgba):
        colour conversion, palette, alpha fill and (demote) the 16 -> 15+1 bit Demote happen in the output kernel.  alpha=False:
        no alpha destination, the frame's A samples stay.  device=True: through a device copy of the frame.  region = (x, y, w, h)."""
        sb = layout["sample_bytes"]
        offs = layout["channel_offsets"]  # A,R,G,B
        d = self.upload(frame) if device else None
        base = d if device else frame.ctypes.data
        dst = RgbaDst()
        dst.struct_size, dst.demote_ae16 = C.sizeof(RgbaDst), int(demote)
        for p, off in ((dst.r, offs[1]), (dst.g, offs[2]), (dst.b, offs[3])) + (((dst.a, offs[0]),) if alpha else ()):
            _set_outplane(p, base + off, layout["colbytes"], layout["rowbytes"], 8 * sb, depth or _layout_depth(layout), width, height)
        buf = np.frombuffer(data, dtype=np.uint8)
        try:
            fn = self.L.j2k_hip_decode_rgba_device if device else self.L.j2k_hip_decode_rgba
            self._check(fn(self.h, buf.ctypes.data, len(data), subsample, C.byref(Rect(*region)) if region is not None else None, C.byref(dst)))
            if device:
                frame[:] = self.d2h(d, frame.nbytes)
        finally:
            if d:
                self.free(d)
        return frame

    def decode_rgba_channels(self, data: bytes, r, g, b, a=None, depth: int | None = None, subsample: int = 1, region=None, demote: bool = False):
        """j2k_hip_decode_rgba into one 2-D numpy view per channel, wherever each lies and whatever its strides (planar buffers,
        padded or bottom-up rows, samples of interleaved pixels); a=None: no alpha destination."""
        dst = RgbaDst()
        dst.struct_size, dst.demote_ae16 = C.sizeof(RgbaDst), int(demote)
        for p, v in ((dst.r, r), (dst.g, g), (dst.b, b), (dst.a, a)):
            if v is None:
                continue
            assert v.ndim == 2 and v.dtype in _SAMPLE_DTYPES
            _set_outplane(p, v.ctypes.data, v.strides[1], v.strides[0], 8 * v.itemsize, depth or _array_depth(v), v.shape[1], v.shape[0])
        buf = np.frombuffer(data, dtype=np.uint8)
        self._check(self.L.j2k_hip_decode_rgba(self.h, buf.ctypes.data, len(data), subsample,
                                               C.byref(Rect(*region)) if region is not None else None, C.byref(dst)))

    # -- decode: the frames of a sequence in one call ---------------------------------------------
    def decode_sequence_planar(self, files, subsample: int = 1, region=None, device: bool = False, sample_bits: int | None = None,
                               depth: int | None = None, channels: int | None = None, out: np.ndarray | None = None) -> np.ndarray:
        """Decode frames of one geometry in one call (j2k_hip_decode_sequence[_device]) into planar buffers:
        (frames, channels, h, w) of uint8 / uint16, frame f what decode_planar / decode_region_planar gives for files[f].
        region = (x, y, w, h); out: a buffer (frames, channels, rows, cols) to decode into (its top-left part is written);
        device=True: through a device copy of the buffer."""
        i = read_info(files[0])
        nf, nc = len(files), channels or i["channels"]
        red = max(subsample, 1).bit_length() - 1
        w, h = (region[2], region[3]) if region is not None else (-(-i["width"] >> red), -(-i["height"] >> red))
        bits = sample_bits or (8 if i["depth"] <= 8 else 16)
        if out is None:
            out = np.zeros((nf, nc, h, w), dtype=_sample_dtype(bits))
        assert out.ndim == 4 and out.shape[:2] == (nf, nc) and out.itemsize * 8 == bits and out.flags.c_contiguous
        _, _, rows, cols = out.shape
        d = self.upload(out) if device else None
        base = d if device else out.ctypes.data
        arr = (OutPlane * (nf * nc))()
        for k in range(nf * nc):
            _set_outplane(arr[k], base + k * rows * cols * out.itemsize, out.itemsize, cols * out.itemsize, bits,
                          depth or min(i["depth"], 16, bits), cols, rows)
        fa, _keep = _seq_files(files)
        try:
            fn = self.L.j2k_hip_decode_sequence_device if device else self.L.j2k_hip_decode_sequence
            self._check(fn(self.h, fa, nf, subsample, C.byref(Rect(*region)) if region is not None else None, arr, nc))
            if device:
                out[...] = self.d2h(d, out.nbytes).view(out.dtype).reshape(out.shape)
        finally:
            if d:
                self.free(d)
        return out

    def decode_sequence_channels(self, files, chans: list, depth: int | None = None, subsample: int = 1, region=None):
        """j2k_hip_decode_sequence into one 2-D numpy view per frame and codec channel (chans[f][c]), wherever each lies and
        whatever its strides: the general form of the C ABI's destination."""
        nf, nc = len(files), len(chans[0])
        arr = (OutPlane * (nf * nc))()
        for f in range(nf):
            assert len(chans[f]) == nc
            for c, a in enumerate(chans[f]):
                assert a.ndim == 2 and a.dtype in _SAMPLE_DTYPES
                _set_outplane(arr[f * nc + c], a.ctypes.data, a.strides[1], a.strides[0], 8 * a.itemsize, depth or _array_depth(a), a.shape[1], a.shape[0])
        fa, _keep = _seq_files(files)
        self._check(self.L.j2k_hip_decode_sequence(self.h, fa, nf, subsample, C.byref(Rect(*region)) if region is not None else None, arr, nc))

    def decode_rgba_sequence(self, files, frames: np.ndarray, layout: dict, width: int, height: int, depth: int | None = None,
                             subsample: int = 1, region=None, demote: bool = False, device: bool = False, alpha: bool = True):
        """Decode frames of one geometry straight into the R, G, B, A samples of After Effects ARGB frames (decode_rgba's
        arguments; j2k_hip_decode_rgba_sequence[_device]): frames = one contiguous array whose slice f is frame f's buffer."""
        nf = len(files)
        assert frames.shape[0] == nf and frames.flags.c_contiguous
        sb, offs = layout["sample_bytes"], layout["channel_offsets"]  # A,R,G,B
        d = self.upload(frames) if device else None
        base = d if device else frames.ctypes.data
        per = frames.nbytes // nf
        dsts = (RgbaDst * nf)()
        for f in range(nf):
            dst = dsts[f]
            dst.struct_size, dst.demote_ae16 = C.sizeof(RgbaDst), int(demote)
            for p, off in ((dst.r, offs[1]), (dst.g, offs[2]), (dst.b, offs[3])) + (((dst.a, offs[0]),) if alpha else ()):
                _set_outplane(p, base + f * per + off, layout["colbytes"], layout["rowbytes"], 8 * sb, depth or _layout_depth(layout), width, height)
        fa, _keep = _seq_files(files)
        try:
            fn = self.L.j2k_hip_decode_rgba_sequence_device if device else self.L.j2k_hip_decode_rgba_sequence
            self._check(fn(self.h, fa, nf, subsample, C.byref(Rect(*region)) if region is not None else None, dsts))
            if device:
                frames[...] = self.d2h(d, frames.nbytes).view(frames.dtype).reshape(frames.shape)
        finally:
            if d:
                self.free(d)
        return frames

    def decode_rgba_sequence_channels(self, files, chans: list, depth: int | None = None, subsample: int = 1, region=None, demote: bool = False):
        """j2k_hip_decode_rgba_sequence into 2-D numpy views: chans[f] = (r, g, b, a) of frame f, a may be None in all frames."""
        nf = len(files)
        dsts = (RgbaDst * nf)()
        for f in range(nf):
            dst = dsts[f]
            dst.struct_size, dst.demote_ae16 = C.sizeof(RgbaDst), int(demote)
            for p, v in zip((dst.r, dst.g, dst.b, dst.a), chans[f]):
                if v is None:
                    continue
                assert v.ndim == 2 and v.dtype in _SAMPLE_DTYPES
                _set_outplane(p, v.ctypes.data, v.strides[1], v.strides[0], 8 * v.itemsize, depth or _array_depth(v), v.shape[1], v.shape[0])
        fa, _keep = _seq_files(files)
        self._check(self.L.j2k_hip_decode_rgba_sequence(self.h, fa, nf, subsample, C.byref(Rect(*region)) if region is not None else None, dsts))

    def set_max_layers(self, layers: int):
        """j2k_hip_decode_set_max_layers: every decode call on this handle keeps the first `layers` quality layers of its file
        (0 = all); sticky until set again."""
        self._check(self.L.j2k_hip_decode_set_max_layers(self.h, layers))

    def max_layers(self) -> int:
        v = C.c_uint32()
        self._check(self.L.j2k_hip_decode_get_max_layers(self.h, C.byref(v)))
        return v.value

    def set_xyz_to_rgb(self, target: int):
        """j2k_hip_decode_set_xyz_to_rgb: the RGBA decode calls on this handle convert X'Y'Z' code values to R'G'B' of `target`
        (0 = off, 1 sRGB, 2 Rec.709 under a 2.4 power, 3 Rec.709 linear); sticky until set again."""
        self._check(self.L.j2k_hip_decode_set_xyz_to_rgb(self.h, target))

    def xyz_to_rgb(self) -> int:
        v = C.c_uint32()
        self._check(self.L.j2k_hip_decode_get_xyz_to_rgb(self.h, C.byref(v)))
        return v.value

    def decode_work(self) -> tuple:
        """(coding passes, codeword bytes) handed to Tier-1 by the last decode call, summed over the frames of a sequence call."""
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self.L.j2k_hip_debug_decode_work(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def decode_kernels(self) -> tuple:
        """(blocks the lane-per-block kernel took, blocks the wave-per-block kernel took) in the last decode call."""
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self.L.j2k_hip_debug_decode_kernels(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def stats(self) -> dict:
        s = Stats()
        self._check(self.L.j2k_hip_get_stats(self.h, C.byref(s)))
        return s.as_dict()

    def guard_bits(self) -> int:
        """Guard bits in the QCD of the last file this handle wrote (j2k_hip_encode_get_guard_bits); 0 before any."""
        g = C.c_uint32()
        self._check(self.L.j2k_hip_encode_get_guard_bits(self.h, C.byref(g)))
        return g.value

    def layer_slopes(self, tile: int = 0) -> list:
        """The slope thresholds the layers of tile `tile` of the last file this handle wrote were laid out at
        (j2k_hip_encode_get_layer_slopes): what a rates / psnr search ended at (-1: everything left), or the slopes given."""
        n = C.c_uint32()
        self._check(self.L.j2k_hip_encode_get_layer_slopes(self.h, tile, None, 0, C.byref(n)))
        out = (C.c_double * max(n.value, 1))()
        self._check(self.L.j2k_hip_encode_get_layer_slopes(self.h, tile, out, n.value, C.byref(n)))
        return [out[i] for i in range(n.value)]

    def dwt_time(self, first: int, count: int, repeat: int = 20) -> float:
        """Mean device time (ms) of the DWT launches of levels [first, first+count) of the last encode, replayed back to back."""
        ms = C.c_double()
        self._check(self.L.j2k_hip_debug_dwt_time(self.h, first, count, repeat, C.byref(ms)))
        return ms.value

    def dwt_level_ms(self):
        buf = (C.c_double * 40)()
        n = self.L.j2k_hip_get_dwt_level_ms(self.h, buf, 40)
        return list(buf[:n])

    # -- compare ----------------------------------------------------------------------------------
    def _diffs(self, n: int):
        arr = (Diff * n)()
        for d in arr:
            d.struct_size = C.sizeof(Diff)
        return arr

    def compare(self, data: bytes, params: Params, frame=None, layout=None, planar=None, comps=None, views=None) -> list:
        """j2k_hip_compare: the file `data` against the source frame it was written from (host memory; given as frame + layout,
        planar, comps or views: _source_views) -> one dict per component (samples, differing, sum_abs, sum_sq, max_abs,
        first_x, first_y, mse, psnr)."""
        buf, planes = _source_views(params, frame, layout, planar, comps, views)
        diffs = self._diffs(params.channels)
        file = np.frombuffer(data, dtype=np.uint8)
        self._check(self.L.j2k_hip_compare(self.h, C.byref(params), planes(buf.ctypes.data), file.ctypes.data, file.size, diffs, len(diffs)))
        return [d.as_dict() for d in diffs]

    def compare_device(self, data: bytes, params: Params, frame=None, layout=None, planar=None, comps=None, views=None, d_buf=None) -> list:
        """j2k_hip_compare_device: the same with the source frame in device memory (d_buf: it is there already)."""
        buf, planes = _source_views(params, frame, layout, planar, comps, views)
        diffs = self._diffs(params.channels)
        file = np.frombuffer(data, dtype=np.uint8)
        d_in = d_buf if d_buf is not None else self.upload(buf)
        try:
            self._check(self.L.j2k_hip_compare_device(self.h, C.byref(params), planes(d_in), file.ctypes.data, file.size, diffs, len(diffs)))
        finally:
            if d_buf is None:
                self.free(d_in)
        return [d.as_dict() for d in diffs]

    def stage_compare(self, decoded, params: Params, frame=None, layout=None, planar=None, comps=None, views=None) -> list:
        """j2k_hip_stage_compare: the source frame against decoded component planes supplied by the caller -- `decoded`: one 2-D
        array of unsigned samples per component, each at the component's own size."""
        buf, planes = _source_views(params, frame, layout, planar, comps, views)
        dec = np.concatenate([np.ascontiguousarray(np.asarray(d).astype(np.uint16)).reshape(-1) for d in decoded])
        diffs = self._diffs(params.channels)
        d_in, d_dec = self.upload(buf), self.upload(dec)
        try:
            self._check(self.L.j2k_hip_stage_compare(self.h, C.byref(params), planes(d_in), d_dec, diffs, len(diffs)))
        finally:
            self.free(d_in)
            self.free(d_dec)
        return [d.as_dict() for d in diffs]

    # -- stages -----------------------------------------------------------------------------------
    def stage_frontend(self, frame: np.ndarray, layout: dict, params: Params, depth_bits: int | None = None) -> np.ndarray:
        """j2k_hip_stage_frontend of an AE frame; depth_bits: Channel.depth of its samples (default: what the layout says)."""
        d_in = self.upload(frame)
        n = params.channels * params.width * params.height
        d_out = self.malloc(4 * n)
        try:
            planes = planes_from_layout(d_in, layout, params.channels, depth_bits)
            self._check(self.L.j2k_hip_stage_frontend(self.h, C.byref(params), planes, d_out))
            raw = self.d2h(d_out, 4 * n)
        finally:
            self.free(d_in)
            self.free(d_out)
        return _split_comps(raw[:4 * sum(h * w for h, w in comp_shapes(params))], params)

    def stage_frontend_planes(self, buf: np.ndarray, planes, params: Params):
        """j2k_hip_stage_frontend of any channel views: `planes` is a callable, device address of `buf` -> Plane array.
        Components of one size: (channels, H, W); sub-sampled ones: a list of 2-D arrays."""
        d_in = self.upload(buf)
        n = sum(h * w for h, w in comp_shapes(params))
        d_out = self.malloc(4 * n)
        try:
            self._check(self.L.j2k_hip_stage_frontend(self.h, C.byref(params), planes(d_in), d_out))
            raw = self.d2h(d_out, 4 * n)
        finally:
            self.free(d_in)
            self.free(d_out)
        return _split_comps(raw, params)

    def stage_transform(self, buf: np.ndarray, planes, params: Params, cuts=None, descending: bool = False) -> np.ndarray:
        """j2k_hip_stage_transform: the front end and the DWT launches of an encode of the channel views `planes`
        (a callable: device address of `buf` -> Plane array, e.g. planes_from_layout) -> (channels, H, W) coefficients
        (sub-sampled components: a list of 2-D arrays, each at its own size).
        cuts: per level (0 = full resolution) a list of cut points in row pairs; each level is launched once per interval."""
        d_in = self.upload(buf)
        n = params.channels * params.width * params.height
        d_out = self.malloc(4 * n)
        cuts = [list(c) for c in (cuts or [])]
        flat = [v for c in cuts for v in c]
        try:
            self._check(self.L.j2k_hip_stage_transform(self.h, C.byref(params), planes(d_in), (C.c_uint32 * max(len(flat), 1))(*flat),
                                                       (C.c_uint32 * max(len(cuts), 1))(*[len(c) for c in cuts]), len(cuts), int(descending), d_out))
            raw = self.d2h(d_out, 4 * n)
        finally:
            self.free(d_in)
            self.free(d_out)
        return _split_comps(raw[:4 * sum(h * w for h, w in comp_shapes(params))], params)

    def stage_dwt(self, planes: np.ndarray, levels: int, reversible: bool, x0=0, y0=0, repeat=1):
        """planes: (n, h, w) int32 / float32. Returns (result, ms per run)."""
        dt = np.int32 if reversible else np.float32
        planes = np.ascontiguousarray(planes, dtype=dt)
        n, h, w = planes.shape
        d_in = self.upload(planes)
        d_out = self.malloc(planes.nbytes)
        ms = C.c_double()
        try:
            self._check(self.L.j2k_hip_stage_dwt(self.h, int(reversible), w, h, n, levels, x0, y0, d_in, d_out, repeat,
                                                 C.byref(ms)))
            raw = self.d2h(d_out, planes.nbytes)
        finally:
            self.free(d_in)
            self.free(d_out)
        return raw.view(dt).reshape(n, h, w), ms.value

    def stage_dwt_regions(self, planes: np.ndarray, levels: int, reversible: bool, regions):
        """The region form of stage_dwt (j2k_hip_stage_dwt_regions): planes (n, h, w) int32 / float32, regions
        [(x, y, w, h, x0, y0)] sub-rectangles of every plane, each transformed on its own with its own origin, every
        (plane, region) a job of the same launch per level.  Returns the planes; words outside every region stay."""
        dt = np.int32 if reversible else np.float32
        planes = np.ascontiguousarray(planes, dtype=dt)
        n, h, w = planes.shape
        nr = len(regions)
        rg = (IdwtRegion * max(nr, 1))()
        for i in range(nr):
            rg[i].x, rg[i].y, rg[i].w, rg[i].h, rg[i].x0, rg[i].y0 = regions[i]
        d_in = self.upload(planes)
        d_out = self.malloc(max(planes.nbytes, 16))
        try:
            self._check(self.L.j2k_hip_stage_dwt_regions(self.h, int(reversible), w, h, n, levels, rg, nr, d_in, d_out))
            raw = self.d2h(d_out, planes.nbytes)
        finally:
            self.free(d_in)
            self.free(d_out)
        return raw.view(dt).reshape(n, h, w)

    def stage_t1(self, coef: np.ndarray, rects, orients, stepsizes, reversible: bool, want_passes: bool = False, style=None):
        """coef: (H, W) int32/float32 plane; rects: list of (x, y, w, h). Returns list of dicts.  style (a code-block style,
        0 included): through j2k_hip_stage_t1_styled, with `rates` per pass and no `nmsedec`."""
        dt = np.int32 if reversible else np.float32
        coef = np.ascontiguousarray(coef, dtype=dt)
        H, W = coef.shape
        nb = len(rects)
        U = lambda v: (C.c_uint32 * nb)(*v)
        bx, by, bw, bh = (U([r[i] for r in rects]) for i in range(4))
        ori = U(orients)
        ss = (C.c_float * nb)(*stepsizes)
        numbps, npasses, length = U([0] * nb), U([0] * nb), U([0] * nb)
        offs = (C.c_uint64 * nb)()
        cap = sum(r[2] * r[3] for r in rects) * 8 + 4096
        data = np.empty(cap, dtype=np.uint8)
        d = self.upload(coef)
        MP = 96
        rates = (C.c_uint32 * (nb * MP))()
        dist = (C.c_int32 * (nb * MP))()
        try:
            if style is not None:
                self._check(self.L.j2k_hip_stage_t1_styled(self.h, int(reversible), d, W, nb, bx, by, bw, bh, ori, ss, numbps,
                                                           npasses, length, offs, data.ctypes.data, cap, rates, C.c_uint32(style)))
            elif want_passes:
                self._check(self.L.j2k_hip_stage_t1_passes(self.h, int(reversible), d, W, nb, bx, by, bw, bh, ori, ss, numbps,
                                                           npasses, length, offs, data.ctypes.data, cap, rates, dist))
            else:
                self._check(self.L.j2k_hip_stage_t1(self.h, int(reversible), d, W, nb, bx, by, bw, bh, ori, ss, numbps, npasses,
                                                    length, offs, data.ctypes.data, cap))
        finally:
            self.free(d)
        out = [dict(numbps=numbps[i], npasses=npasses[i], length=length[i],
                    data=data[offs[i]:offs[i] + length[i]].tobytes()) for i in range(nb)]
        if style is not None:
            for i, o in enumerate(out):
                o["rates"] = list(rates[i * MP:i * MP + o["npasses"]])
        elif want_passes:
            for i, o in enumerate(out):
                o["rates"] = list(rates[i * MP:i * MP + o["npasses"]])
                o["nmsedec"] = list(dist[i * MP:i * MP + o["npasses"]])
        return out

    def stage_t1_slots(self, coef: np.ndarray, rects, orients, stepsizes, reversible: bool, style: int, sym_cap, out_cap,
                       guard_bytes: int, want_passes: bool = False):
        """j2k_hip_stage_t1_slots: stage_t1 with the caller's capacities per block (bytes of decisions, bytes of codeword) and
        guard stripes of guard_bytes around every slot; a block that does not fit does not raise.  Returns a dict: err (the
        kernels' error word), numbps / npasses / nsym / length (uint32 arrays), rates ((n, 96) uint32, with want_passes), sym
        and out (the arenas whole, uint8), sym_off / out_off (where each block's slot begins: computed here, from the layout
        the header states) and fill (the byte both arenas are filled with before the launches)."""
        dt = np.int32 if reversible else np.float32
        coef = np.ascontiguousarray(coef, dtype=dt)
        H, W = coef.shape
        nb = len(rects)
        U = lambda v: (C.c_uint32 * max(nb, 1))(*v)
        bx, by, bw, bh = (U([r[i] for r in rects]) for i in range(4))
        ori = U(orients)
        ss = (C.c_float * max(nb, 1))(*stepsizes)
        sc, oc = U([int(v) for v in sym_cap]), U([int(v) for v in out_cap])
        sym_off = guard_bytes + np.concatenate([[0], np.cumsum([int(v) + guard_bytes for v in sym_cap])]).astype(np.int64)
        out_off = guard_bytes + np.concatenate([[0], np.cumsum([int(v) + guard_bytes for v in out_cap])]).astype(np.int64)
        sym = np.zeros(int(sym_off[-1]), dtype=np.uint8)
        out = np.zeros(int(out_off[-1]), dtype=np.uint8)
        numbps, npasses, nsym, length = (np.zeros(max(nb, 1), dtype=np.uint32) for _ in range(4))
        P = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
        MP = 96
        rates = np.zeros((max(nb, 1), MP), dtype=np.uint32) if want_passes else None
        err = C.c_uint32(0xffffffff)
        d = self.upload(coef)
        try:
            self._check(self.L.j2k_hip_stage_t1_slots(self.h, int(reversible), d, W, nb, bx, by, bw, bh, ori, ss, C.c_uint32(style),
                                                      sc, oc, guard_bytes, C.byref(err), P(numbps), P(npasses), P(nsym), P(length),
                                                      P(rates) if want_passes else None, sym.ctypes.data, sym.size,
                                                      out.ctypes.data, out.size))
        finally:
            self.free(d)
        res = dict(err=err.value, numbps=numbps[:nb], npasses=npasses[:nb], nsym=nsym[:nb], length=length[:nb], sym=sym, out=out,
                   sym_off=sym_off[:nb], out_off=out_off[:nb], fill=0xA5)
        if want_passes:
            res["rates"] = rates[:nb]
        return res

    def stage_rate(self, weight, comp, numbps, npasses, pass_rate, pass_dist, first=0, count=0, done=None, ahead=None, scans=()):
        """j2k_hip_stage_rate.  Tables per block (pass_rate / pass_dist: (n, 96)); scans: (thresh, mode, slot) with mode one
        of RATE_SCAN / RATE_SUMS_FETCH / RATE_SUMS_FETCH_LAST.  Returns a dict: disto (n, 96) float64, reach (n, 96) float32,
        bounds (3, n); with queries also body (4, K) uint64, taken (nscans, count) RATE_TAKEN records, bytes (nscans, count)
        uint32 and sums (nscans, 8) uint64."""
        MP = 96
        n = len(npasses)
        weight = np.ascontiguousarray(weight, dtype=np.float64)
        comp = np.ascontiguousarray(comp, dtype=np.uint8)
        numbps = np.ascontiguousarray(numbps, dtype=np.uint32)
        npasses = np.ascontiguousarray(npasses, dtype=np.uint32)
        pass_rate = np.ascontiguousarray(pass_rate, dtype=np.uint32).reshape(n, MP)
        pass_dist = np.ascontiguousarray(pass_dist, dtype=np.int32).reshape(n, MP)
        assert weight.size == comp.size == numbps.size == n
        disto, reach, bounds = np.zeros((n, MP), np.float64), np.zeros((n, MP), np.float32), np.zeros((3, max(n, 1)), np.float64)
        K = 0 if ahead is None else len(ahead)
        ah = np.ascontiguousarray(ahead if K else [0.0], dtype=np.float64)
        body = np.zeros((4, max(K, 1)), np.uint64)
        dn = None if done is None else np.ascontiguousarray(done, dtype=np.uint8)
        assert dn is None or dn.size == count
        ns = len(scans)
        sc = (RateScan * max(ns, 1))()
        for i, (t, mode, slot) in enumerate(scans):
            sc[i].thresh, sc[i].mode, sc[i].slot = t, mode, slot
        taken = np.zeros((max(ns, 1), max(count, 1)), RATE_TAKEN)
        nbytes = np.zeros((max(ns, 1), max(count, 1)), np.uint32)
        sums = np.zeros((max(ns, 1), 8), np.uint64)
        ptr = lambda a: a.ctypes.data
        self._check(self.L.j2k_hip_stage_rate(self.h, n, ptr(weight), ptr(comp), ptr(numbps), ptr(npasses), ptr(pass_rate), ptr(pass_dist),
                                              ptr(disto), ptr(reach), ptr(bounds), first, count, None if dn is None else ptr(dn),
                                              ptr(ah) if K else None, K, ptr(body) if K else None, sc if ns else None, ns,
                                              ptr(taken) if ns else None, ptr(nbytes) if ns else None, ptr(sums) if ns else None))
        out = dict(disto=disto, reach=reach, bounds=bounds[:, :n])
        if K:
            out["body"] = body
        if ns:
            out.update(taken=taken[:ns, :count], bytes=nbytes[:ns, :count], sums=sums)
        return out

    def stage_rate_layers(self, weight, numbps, npasses, pass_rate, pass_dist, slopes):
        """j2k_hip_stage_rate_layers: rate_layers_kernel on tables per block (pass_rate / pass_dist: (n, 96); weight: one per
        block, or fewer -- block i takes weight[i % len(weight)]).  Returns a dict: passes (n, L) uint8 and bytes (n, L) uint32,
        cumulative over the layers; spare_passes / spare_bytes: the entries behind the last block's as they came back (the
        device arrays were filled with 0xA5); rate_back / dist_back: the pass tables as they lie on the device afterwards."""
        MP, SPARE = 96, 64
        n, nl = len(npasses), len(slopes)
        weight = np.ascontiguousarray(weight, dtype=np.float64)
        numbps = np.ascontiguousarray(numbps, dtype=np.uint32)
        npasses = np.ascontiguousarray(npasses, dtype=np.uint32)
        pass_rate = np.ascontiguousarray(pass_rate, dtype=np.uint32).reshape(n, MP)
        pass_dist = np.ascontiguousarray(pass_dist, dtype=np.int32).reshape(n, MP)
        sl = np.ascontiguousarray(slopes, dtype=np.float64)
        assert numbps.size == n
        passes, nbytes = np.zeros((n + SPARE, max(nl, 1)), np.uint8), np.zeros((n + SPARE, max(nl, 1)), np.uint32)
        rate_back, dist_back = np.zeros((n, MP), np.uint32), np.zeros((n, MP), np.int32)
        ptr = lambda a: a.ctypes.data if a.size else None
        self._check(self.L.j2k_hip_stage_rate_layers(self.h, n, ptr(weight), weight.size, ptr(numbps), ptr(npasses), ptr(pass_rate), ptr(pass_dist),
                                                     ptr(sl), nl, ptr(passes), ptr(nbytes), ptr(rate_back), ptr(dist_back)))
        return dict(passes=passes[:n], bytes=nbytes[:n], spare_passes=passes[n:], spare_bytes=nbytes[n:], rate_back=rate_back, dist_back=dist_back)

    def stage_rate_curve(self, weight, numbps, npasses, pass_rate, pass_dist, nframes, cap, base, step, K):
        """j2k_hip_stage_rate_curve: rate_curve_kernel on tables per block, read as nframes frames.  Returns a dict: sums
        (nframes, K, 2) uint64 = body bytes and header bits per frame and candidate; spare: the entries behind them as they came
        back (filled with 0xA5 first); rate_back / dist_back: the pass tables as they lie on the device afterwards."""
        MP, SPARE = 96, 64
        n = len(npasses)
        weight = np.ascontiguousarray(weight, dtype=np.float64)
        numbps = np.ascontiguousarray(numbps, dtype=np.uint32)
        npasses = np.ascontiguousarray(npasses, dtype=np.uint32)
        pass_rate = np.ascontiguousarray(pass_rate, dtype=np.uint32).reshape(n, MP)
        pass_dist = np.ascontiguousarray(pass_dist, dtype=np.int32).reshape(n, MP)
        cap = np.ascontiguousarray(cap, dtype=np.int32)
        assert numbps.size == n and cap.size == nframes
        nf, k = max(int(nframes), 0), max(int(K), 0)
        sums = np.zeros(nf * min(k, 64) * 2 + SPARE, np.uint64)
        rate_back, dist_back = np.zeros((n, MP), np.uint32), np.zeros((n, MP), np.int32)
        ptr = lambda a: a.ctypes.data if a.size else None
        self._check(self.L.j2k_hip_stage_rate_curve(self.h, n, ptr(weight), weight.size, ptr(numbps), ptr(npasses), ptr(pass_rate), ptr(pass_dist),
                                                    nframes, ptr(cap), base, step, K, ptr(sums), ptr(rate_back), ptr(dist_back)))
        return dict(sums=sums[:nf * k * 2].reshape(nf, k, 2), spare=sums[nf * k * 2:], rate_back=rate_back, dist_back=dist_back)

    def stage_gather(self, src, dst, blocks=(), headers=(), segments=(), blob=None) -> np.ndarray:
        """j2k_hip_stage_gather: src / dst (/ blob, default: src) uint8 arrays, the piece lists [(dst, src, len)].  Returns
        the destination after the launch; `dst` itself is not changed."""
        src = np.ascontiguousarray(src, dtype=np.uint8)
        blob = src if blob is None else np.ascontiguousarray(blob, dtype=np.uint8)
        out = np.array(dst, dtype=np.uint8, copy=True)
        tables = [np.array([(d, s, ln, 0) for d, s, ln in pieces], dtype=GATHER_PIECE) for pieces in (blocks, headers, segments)]
        ptr = lambda a: a.ctypes.data if a.size else None
        self._check(self.L.j2k_hip_stage_gather(self.h, ptr(src), src.size, ptr(blob), blob.size, ptr(out), out.size,
                                                ptr(tables[0]), tables[0].size, ptr(tables[1]), tables[1].size,
                                                ptr(tables[2]), tables[2].size))
        return out

    def stage_pack_offsets(self, lens, base: int = 0, dst=None) -> np.ndarray:
        """j2k_hip_stage_pack_offsets: dst[i] = base + lens[0] + .. + lens[i - 1] (uint64); dst: what the array holds before."""
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        out = np.zeros(lens.size, np.uint64) if dst is None else np.array(dst, dtype=np.uint64, copy=True)
        assert out.size == lens.size
        self._check(self.L.j2k_hip_stage_pack_offsets(self.h, lens.ctypes.data if lens.size else None, lens.size, C.c_uint64(base),
                                                      out.ctypes.data if out.size else None))
        return out

    def stage_idwt(self, planes: np.ndarray, levels: int, reversible: bool, x0=0, y0=0, regions=None):
        """planes: (n, h, w) int32 / float32 in Mallat layout -> the synthesised samples.  regions: [(x, y, w, h, x0, y0)]
        sub-rectangles of every plane, each a Mallat layout of its own (x0, y0 are then ignored); words outside stay."""
        dt = np.int32 if reversible else np.float32
        planes = np.ascontiguousarray(planes, dtype=dt)
        n, h, w = planes.shape
        nr = len(regions) if regions else 0
        rg = (IdwtRegion * max(nr, 1))()
        for i in range(nr):
            rg[i].x, rg[i].y, rg[i].w, rg[i].h, rg[i].x0, rg[i].y0 = regions[i]
        d_in = self.upload(planes)
        d_out = self.malloc(max(planes.nbytes, 16))
        try:
            self._check(self.L.j2k_hip_stage_idwt(self.h, int(reversible), w, h, n, levels, x0, y0, rg if nr else None, nr,
                                                  d_in, d_out))
            raw = self.d2h(d_out, planes.nbytes)
        finally:
            self.free(d_in)
            self.free(d_out)
        return raw.view(dt).reshape(n, h, w)

    def stage_idwt_window(self, planes: np.ndarray, levels: int, reversible: bool, window, x0=0, y0=0, guard=None):
        """The windowed inverse DWT (j2k_hip_stage_idwt_window): planes (n, h, w) in Mallat layout, window = (x, y, w, h) in
        plane coordinates.  Only the window of the result is specified.  guard = a 32-bit fill: one row of it lies before and
        behind the planes in the same device allocation, and (result, rows before, rows behind) is returned."""
        dt = np.int32 if reversible else np.float32
        planes = np.ascontiguousarray(planes).view(dt) if planes.dtype in (np.uint32, np.int32, np.float32) else np.ascontiguousarray(planes, dtype=dt)
        n, h, w = planes.shape
        pad = w * 4 if guard is not None else 0
        d_in = self.upload(planes)
        d_out = self.malloc(max(planes.nbytes, 16) + 2 * pad)
        try:
            if pad:
                self.h2d(d_out, np.full(n * h * w + 2 * w, guard, dtype=np.uint32))
            self._check(self.L.j2k_hip_stage_idwt_window(self.h, int(reversible), w, h, n, levels, x0, y0, C.byref(Rect(*window)),
                                                         d_in, d_out + pad))
            raw = self.d2h(d_out, planes.nbytes + 2 * pad)
        finally:
            self.free(d_in)
            self.free(d_out)
        body = raw[pad:pad + planes.nbytes].view(dt).reshape(n, h, w)
        if guard is None:
            return body
        return body, raw[:pad].view(np.uint32), raw[pad + planes.nbytes:].view(np.uint32)

    def stage_t1_decode(self, plane: np.ndarray, blocks, reversible: bool, kernel: str = "wave") -> np.ndarray:
        """plane: (H, W) int32 / float32 the blocks are decoded into (what it holds elsewhere stays).  blocks: dicts with
        rect (x, y, w, h), orient, numbps, npasses, data (codeword bytes) and optionally half_step, roishift.
        kernel: "wave" (a wavefront per block) or "lanes" (a lane per block, groups of 64 in the order given)."""
        dt = np.int32 if reversible else np.float32
        plane = np.ascontiguousarray(plane, dtype=dt)
        H, W = plane.shape
        nb = len(blocks)
        arr = (DecBlock * max(nb, 1))()
        pos = 0
        for i, b in enumerate(blocks):
            arr[i].x, arr[i].y, arr[i].w, arr[i].h = b["rect"]
            arr[i].orient, arr[i].numbps, arr[i].npasses = b["orient"], b["numbps"], b["npasses"]
            arr[i].roishift, arr[i].half_step = b.get("roishift", 0), b.get("half_step", 1.0)
            arr[i].cw_off, arr[i].cw_len = pos, len(b["data"])
            pos += len(b["data"])
        cw = np.frombuffer(b"".join(b["data"] for b in blocks) + b"\0", dtype=np.uint8)
        d = self.upload(plane)
        try:
            self._check(self.L.j2k_hip_stage_t1_decode(self.h, {"wave": 0, "lanes": 1}[kernel], int(reversible), d, W, nb, arr,
                                                       cw.ctypes.data, pos))
            raw = self.d2h(d, plane.nbytes)
        finally:
            self.free(d)
        return raw.view(dt).reshape(H, W)

    def stage_t1_decode_styled(self, plane: np.ndarray, blocks, reversible: bool, style: int, raw_table=None) -> np.ndarray:
        """stage_t1_decode through the lane kernel under the code-block style `style`; under bypass or termall every block also
        has segs = [(bytes, passes), ...], its codeword segments in order.  raw_table = (seg_first, seg_count, segs pairs,
        nsegs_total) replaces the table built from the blocks (for the refusals)."""
        dt = np.int32 if reversible else np.float32
        plane = np.ascontiguousarray(plane, dtype=dt)
        H, W = plane.shape
        nb = len(blocks)
        arr = (DecBlock * max(nb, 1))()
        pos = 0
        first, count, pairs = [], [], []
        for i, b in enumerate(blocks):
            arr[i].x, arr[i].y, arr[i].w, arr[i].h = b["rect"]
            arr[i].orient, arr[i].numbps, arr[i].npasses = b["orient"], b["numbps"], b["npasses"]
            arr[i].roishift, arr[i].half_step = b.get("roishift", 0), b.get("half_step", 1.0)
            arr[i].cw_off, arr[i].cw_len = pos, len(b["data"])
            pos += len(b["data"])
            sg = b.get("segs") or ()
            first.append(len(pairs))
            count.append(len(sg))
            pairs += [tuple(s) for s in sg]
        total = len(pairs)
        if raw_table is not None:
            first, count, pairs, total = raw_table
        mk = lambda v: (C.c_uint32 * max(len(v), 1))(*v)
        a_first, a_count, a_segs = mk(first), mk(count), mk([v for s in pairs for v in s])
        cw = np.frombuffer(b"".join(b["data"] for b in blocks) + b"\0", dtype=np.uint8)
        d = self.upload(plane)
        try:
            self._check(self.L.j2k_hip_stage_t1_decode_styled(self.h, int(reversible), d, W, nb, arr, cw.ctypes.data, pos, style,
                                                              a_first, a_count, a_segs, total))
            raw = self.d2h(d, plane.nbytes)
        finally:
            self.free(d)
        return raw.view(dt).reshape(H, W)

    def stage_decode_output(self, comps, precs, subs, width: int, height: int, reversible: bool, mct: bool, chans, buf: np.ndarray,
                            stride: int | None = None, gap: int = 0x7fc0dead) -> np.ndarray:
        """The decode's output stage alone.  comps: one 2-D plane per component, int32 / float32 (irreversible planes may
        also come as uint32 bit patterns), of ceil(height / sub_y) x ceil(width / sub_x) samples; precs, subs = [(sub_x,
        sub_y)]: per component.  They go into one device buffer at row stride `stride` words (default: the widest plane's
        width); the words between a row's end and the stride hold `gap`.  chans: dicts with base (a byte offset into buf),
        colbytes, rowbytes, sample_bits, depth, width, height.  buf: the uint8 buffer the channels lie in, uploaded as it
        is.  Returns the whole buffer as the kernel left it."""
        dt = np.int32 if reversible else np.float32
        planes = [np.ascontiguousarray(c).view(np.uint32) if np.asarray(c).dtype == np.uint32 else
                  np.ascontiguousarray(c, dtype=dt).view(np.uint32) for c in comps]
        stride = stride if stride is not None else max(p.shape[1] for p in planes)
        rows = [p.shape[0] for p in planes]
        words = np.full((sum(rows), max(stride, 1)), gap, dtype=np.uint32)
        oc = (OutComp * len(planes))()
        y0 = 0
        for c, p in enumerate(planes):
            words[y0:y0 + p.shape[0], :min(p.shape[1], stride)] = p[:, :stride]
            oc[c].offset, oc[c].prec = y0 * stride, precs[c]
            oc[c].sub_x, oc[c].sub_y = subs[c]
            y0 += p.shape[0]
        arr = (OutPlane * len(chans))()
        for c, ch in enumerate(chans):
            arr[c].base = ch["base"]
            arr[c].colbytes, arr[c].rowbytes = ch["colbytes"], ch["rowbytes"]
            arr[c].sample_bits, arr[c].depth = ch["sample_bits"], ch["depth"]
            arr[c].width, arr[c].height = ch["width"], ch["height"]
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        d_comp = self.upload(words)
        d_buf = self.upload(buf)
        try:
            self._check(self.L.j2k_hip_stage_decode_output(self.h, int(reversible), int(mct), width, height, d_comp, words.size, stride,
                                                           oc, len(planes), d_buf, buf.nbytes, arr, len(chans)))
            return self.d2h(d_buf, buf.nbytes)
        finally:
            self.free(d_comp)
            self.free(d_buf)

    def stage_rgba_output(self, comps, precs, subs, width: int, height: int, reversible: bool, mct: bool, mode: int, chans, buf: np.ndarray,
                          demote: bool = False, lut=None, lut_rgb=(0, 1, 2), org=(0, 0), stride: int | None = None,
                          gap: int = 0x7fc0dead, xyz_to_rgb: int | None = None) -> np.ndarray:
        """The RGBA output stage alone (j2k_hip_stage_rgba_output).  comps, precs, subs, stride, gap as in stage_decode_output,
        each plane of ceil((org_y + height) / sub_y) x ceil((org_x + width) / sub_x) samples.  chans: the dicts of
        stage_decode_output for R, G, B and A in this order; A may be None (no alpha destination).  lut: (entries, columns)
        uint8 palette, lut_rgb the columns R, G, B take.  xyz_to_rgb (0..3): through j2k_hip_stage_rgba_output_xyz, with the
        X'Y'Z' -> R'G'B' conversion of that target.  Returns the whole buffer as the kernel left it."""
        dt = np.int32 if reversible else np.float32
        planes = [np.ascontiguousarray(c).view(np.uint32) if np.asarray(c).dtype == np.uint32 else
                  np.ascontiguousarray(c, dtype=dt).view(np.uint32) for c in comps]
        stride = stride if stride is not None else max(p.shape[1] for p in planes)
        words = np.full((sum(p.shape[0] for p in planes), max(stride, 1)), gap, dtype=np.uint32)
        oc = (OutComp * len(planes))()
        y0 = 0
        for c, p in enumerate(planes):
            words[y0:y0 + p.shape[0], :min(p.shape[1], stride)] = p[:, :stride]
            oc[c].offset, oc[c].prec = y0 * stride, precs[c]
            oc[c].sub_x, oc[c].sub_y = subs[c]
            y0 += p.shape[0]
        dst = RgbaDst()
        dst.struct_size, dst.demote_ae16 = C.sizeof(RgbaDst), int(demote)
        for p, ch in zip((dst.r, dst.g, dst.b, dst.a), chans):
            if ch is not None:
                _set_outplane(p, ch["base"], ch["colbytes"], ch["rowbytes"], ch["sample_bits"], ch["depth"], ch["width"], ch["height"])
        st = RgbaStage()
        st.struct_size, st.mode, st.org_x, st.org_y = C.sizeof(RgbaStage), mode, org[0], org[1]
        if lut is not None:
            lut = np.asarray(lut, dtype=np.uint8)
            st.lut_size, st.lut_columns = lut.shape
            for i in range(lut.shape[0]):
                for k in range(lut.shape[1]):
                    st.lut[i][k] = int(lut[i, k])
            for k in range(3):
                st.lut_rgb[k] = lut_rgb[k]
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        d_comp = self.upload(words)
        d_buf = self.upload(buf)
        try:
            if xyz_to_rgb is None:
                self._check(self.L.j2k_hip_stage_rgba_output(self.h, int(reversible), int(mct), width, height, d_comp, words.size, stride,
                                                             oc, len(planes), d_buf, buf.nbytes, C.byref(dst), C.byref(st)))
            else:
                self._check(self.L.j2k_hip_stage_rgba_output_xyz(self.h, int(reversible), int(mct), width, height, d_comp, words.size, stride,
                                                                 oc, len(planes), d_buf, buf.nbytes, C.byref(dst), C.byref(st), xyz_to_rgb))
            return self.d2h(d_buf, buf.nbytes)
        finally:
            self.free(d_comp)
            self.free(d_buf)
