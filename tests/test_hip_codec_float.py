"""GPU: HipCodec through the C++ interface with a 32-bpc world (Channels of sampleType FLOAT, depth 32; ARGB128): WriteFile
writes the committed libopenjp2 file from the floats of its integers, ReadRGBA fills the floats the model makes of the 16-bit
world's samples -- no temporary world, no SmartCopyWorld."""
import ctypes as C
import os

import numpy as np
import pytest

import float_model as fm
import rgba_cases as rc
from conftest import golden_case
from j2k_amd import api, synth
from oracle.oracle import strip_com

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    from j2k_amd import build
    path = os.path.join(os.path.dirname(api.LIBPATH), "libj2k_host.so")
    if not os.path.exists(path):
        build.build_host()
    api.load_library()
    H = C.CDLL(path)
    H.j2k_host_test_read_rgba.restype = C.c_long
    H.j2k_host_test_read_rgba.argtypes = [C.c_void_p, C.c_ulong, C.c_uint, C.c_void_p, C.c_uint, C.c_uint, C.c_long, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.c_char_p, C.c_ulong]
    H.j2k_host_test_write.restype = C.c_long
    H.j2k_host_test_write.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_int, C.c_long, C.c_void_p, C.c_ulong, C.c_char_p, C.c_ulong]
    return H


def _write(host, frame, lay, w, h, channels, depth, reversible, ycc):
    out = np.empty(frame.nbytes + (1 << 20), dtype=np.uint8)
    err = C.create_string_buffer(512)
    n = host.j2k_host_test_write(frame.ctypes.data, w, h, lay["rowbytes"], lay["sample_bytes"], channels, depth, int(reversible), int(ycc), 1, 0, 1,
                                 -1, out.ctypes.data, out.nbytes, err, 512)
    assert n >= 0, err.value.decode()
    return out[:n].tobytes()


@pytest.mark.parametrize("name, rev", [("g6_300x200_rgb16_97_ict", False), ("g7_300x200_rgb10_53", True)])
def test_write_file_from_a_float_world_writes_the_golden(host, golden, name, rev):
    g, pl, _, cs = golden_case(golden, name)
    frame, lay = synth.ae_frame_float(pl, 16, row_pad_bytes=32, prec=g["prec"])  # the floats of the ARGB64 world's integers
    got = _write(host, frame, lay, g["width"], g["height"], 3, g["prec"], rev, g["params"].get("mct", False))
    assert strip_com(got) == cs


def test_promoted_float_world_writes_what_the_promoted_16_bit_world_writes(host, golden, monkeypatch):
    g, pl, _, _ = golden_case(golden, "g6_300x200_rgb16_97_ict")
    pl = fm.promote16(fm.demote16(pl)).astype(np.int32)
    monkeypatch.setenv("J2K_HOST_TEST_PROMOTE", "1")
    frame, lay = synth.ae_frame_float(pl, 16, promote=True)
    iframe, ilay = synth.ae_frame(fm.demote16(pl).astype(np.int32), 16)
    a = _write(host, frame, lay, 300, 200, 3, 16, False, True)
    b = _write(host, iframe, ilay, 300, 200, 3, 16, False, True)
    assert a == b


def _read(host, data, w, h, sb, depth, demote, alpha, pad=16):
    rb = 4 * sb * w + pad
    frame = np.full(rb * h, 0xa5, np.uint8)
    buf = np.frombuffer(data, dtype=np.uint8)
    err = C.create_string_buffer(512)
    status = host.j2k_host_test_read_rgba(buf.ctypes.data, len(data), 1, frame.ctypes.data, w, h, rb, sb, depth, int(demote), int(alpha), err, 512)
    assert status == 1, err.value.decode()
    return frame, rb


@pytest.mark.parametrize("name", ["j9", "pal", "k2"])
@pytest.mark.parametrize("demote", [True, False], ids=["demote", "plain"])
def test_read_rgba_into_a_float_world_equals_the_model(host, name, demote):
    data = rc.load(name)
    info = api.read_info(data)
    w, h = info["width"], info["height"]
    for alpha in (True, False):
        iframe, irb = _read(host, data, w, h, 2, 16, demote, alpha)
        fframe, frb = _read(host, data, w, h, 4, 32, demote, alpha)
        want = np.full(frb * h, 0xa5, np.uint8)
        iv = np.lib.stride_tricks.as_strided(iframe.view(np.uint16), shape=(h, w, 4), strides=(irb, 8, 2))
        wv = np.lib.stride_tricks.as_strided(want.view(np.uint32), shape=(h, w, 4), strides=(frb, 16, 4), writeable=True)
        first = 0 if alpha else 1  # (the binding demotes a world that is handed over whole: without A, no Demote)
        wv[:, :, first:] = fm.bits(fm.to_float(iv[:, :, first:], 16, demoted=demote and alpha))
        assert np.array_equal(fframe, want), (alpha,)
