"""GPU: HipCodec::Compare through the C++ interface: on a file that HipCodec::WriteFile just wrote from the same world it is
all zero for 5/3 and equal to the C call (j2k_hip_compare) for 9/7; a file for the fallback reader makes it return false."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import float_model as fm
from conftest import golden_case
from j2k_amd import api, synth
from test_read_fallback import _with_coc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    from j2k_amd import build
    path = os.path.join(os.path.dirname(api.LIBPATH), "libj2k_host.so")
    if not os.path.exists(path):
        build.build_host()
    api.load_library()
    H = C.CDLL(path)
    H.j2k_host_test_write.restype = C.c_long
    H.j2k_host_test_write.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_int, C.c_long, C.c_void_p, C.c_ulong, C.c_char_p, C.c_ulong]
    H.j2k_host_test_compare.restype = C.c_long
    H.j2k_host_test_compare.argtypes = [C.c_void_p, C.c_ulong, C.c_int, C.c_void_p, C.c_uint, C.c_uint, C.c_long, C.c_int, C.c_int, C.c_int,
                                        C.POINTER(C.c_ulonglong), C.POINTER(C.c_double), C.c_char_p, C.c_ulong]
    return H


@pytest.fixture(scope="module")
def enc():
    e = api.Encoder(0)
    yield e
    e.close()


def _write(host, frame, lay, w, h, channels, depth, reversible, ycc):
    out = np.empty(frame.nbytes + (1 << 20), dtype=np.uint8)
    err = C.create_string_buffer(512)
    n = host.j2k_host_test_write(frame.ctypes.data, w, h, lay["rowbytes"], lay["sample_bytes"], channels, depth, int(reversible), int(ycc), 1, 0, 1,
                                 -1, out.ctypes.data, out.nbytes, err, 512)
    assert n >= 0, err.value.decode()
    return out[:n].tobytes()


FIELDS = ("samples", "differing", "sum_abs", "sum_sq", "max_abs", "first_x", "first_y")


def _compare(host, data, frame, lay, w, h, channels, depth, fallback=False):
    ints = (C.c_ulonglong * 28)()
    dbl = (C.c_double * 8)()
    err = C.create_string_buffer(512)
    buf = np.frombuffer(data, dtype=np.uint8)
    status = host.j2k_host_test_compare(buf.ctypes.data, len(data), int(fallback), frame.ctypes.data, w, h, lay["rowbytes"], lay["sample_bytes"],
                                        channels, depth, ints, dbl, err, 512)
    if status != 1:
        return status, err.value.decode()
    out = []
    for c in range(channels):
        d = {k: int(ints[7 * c + i]) for i, k in enumerate(FIELDS)}
        d["mse"], d["psnr"] = dbl[2 * c], dbl[2 * c + 1]
        out.append(d)
    return 1, out


@pytest.mark.parametrize("name, channels", [("g3_300x200_rgb8_53_rct", 3), ("g7_300x200_rgb10_53", 3), ("g9_300x200_rgba8_53_rct", 4)])
def test_a_lossless_file_it_just_wrote_is_all_zero(host, golden, name, channels):
    g, pl, _, _ = golden_case(golden, name)
    frame, lay = synth.ae_frame(pl, g["prec"], row_pad_bytes=8)
    data = _write(host, frame, lay, g["width"], g["height"], channels, g["prec"], True, True)
    status, got = _compare(host, data, frame, lay, g["width"], g["height"], channels, g["prec"])
    assert status == 1, got
    for d in got:
        assert d == dict(samples=g["width"] * g["height"], differing=0, sum_abs=0, sum_sq=0, max_abs=0, first_x=0, first_y=0, mse=0.0, psnr=math.inf)


@pytest.mark.parametrize("name", ["g6_300x200_rgb8_97_ict", "g6_300x200_rgb16_97_ict"])
def test_a_lossy_file_it_just_wrote_equals_the_c_call(host, enc, golden, name):
    g, pl, _, _ = golden_case(golden, name)
    frame, lay = synth.ae_frame(pl, g["prec"], row_pad_bytes=8)
    data = _write(host, frame, lay, 300, 200, 3, g["prec"], False, True)
    status, got = _compare(host, data, frame, lay, 300, 200, 3, g["prec"])
    assert status == 1, got
    assert got == enc.compare(data, api.make_params(300, 200, 3, g["prec"]), frame=frame, layout=lay)
    assert all(d["differing"] > 0 and 0 < d["psnr"] < math.inf for d in got)


def test_float_world_and_chroma_options(host, enc, golden, monkeypatch):
    """A FLOAT world follows WriteFile's SampleType FLOAT path; Chroma420 compares Y Cb Cr on their own grids."""
    g, pl, _, _ = golden_case(golden, "g7_300x200_rgb10_53")
    frame, lay = synth.ae_frame_float(pl, 16, row_pad_bytes=32, prec=g["prec"])
    data = _write(host, frame, lay, 300, 200, 3, g["prec"], True, False)
    status, got = _compare(host, data, frame, lay, 300, 200, 3, g["prec"])
    assert status == 1 and all(d["differing"] == 0 and d["psnr"] == math.inf for d in got), got
    # promoted 15+1-bit floats
    pl16 = fm.promote16(fm.demote16(golden_case(golden, "g6_300x200_rgb16_97_ict")[1])).astype(np.int32)
    monkeypatch.setenv("J2K_HOST_TEST_PROMOTE", "1")
    frame, lay = synth.ae_frame_float(pl16, 16, promote=True)
    data = _write(host, frame, lay, 300, 200, 3, 16, True, True)
    status, got = _compare(host, data, frame, lay, 300, 200, 3, 16)
    assert status == 1 and all(d["differing"] == 0 for d in got), got
    monkeypatch.delenv("J2K_HOST_TEST_PROMOTE")
    # 4:2:0 out of the world's R, G, B
    monkeypatch.setenv("J2K_HOST_TEST_CHROMA", "420")
    g, pl, _, _ = golden_case(golden, "g3_300x200_rgb8_53_rct")
    frame, lay = synth.ae_frame(pl, 8)
    for rev in (True, False):
        data = _write(host, frame, lay, 300, 200, 3, 8, rev, False)
        status, got = _compare(host, data, frame, lay, 300, 200, 3, 8)
        assert status == 1, got
        assert [d["samples"] for d in got] == [300 * 200, 150 * 100, 150 * 100]
        p = api.make_params(300, 200, 3, 8, sub=[(1, 1), (2, 2), (2, 2)], rgb_to_sycc=True)
        assert got == enc.compare(data, p, frame=frame, layout=lay)
        assert all((d["differing"] == 0) == rev for d in got)


def test_a_file_for_the_fallback_reader_returns_false(host, golden):
    g, pl, _, cs = golden_case(golden, "g6_300x200_rgb16_97_ict")
    frame, lay = synth.ae_frame(pl, 16)
    bad = _with_coc(cs, (1,), -1)  # a COC that changes a component's levels: J2K_HIP_ERR_UNSUPPORTED
    for fallback in (True, False):
        status, msg = _compare(host, bad, frame, lay, 300, 200, 3, 16, fallback=fallback)
        assert status == 0, msg  # false, nothing written, the fallback codec not asked; never an exception
    # a file that is not this frame's, and a damaged one, throw
    status, msg = _compare(host, cs, frame, lay, 300, 200, 3, 12)
    assert status == -1 and "Error reading file" in msg and "depth" in msg
    status, msg = _compare(host, cs[:60], frame, lay, 300, 200, 3, 16)
    assert status == -1 and "Error reading file" in msg
    status, got = _compare(host, cs, frame, lay, 300, 200, 3, 16)
    assert status == 1 and all(d["differing"] > 0 for d in got)
