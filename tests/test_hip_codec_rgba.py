"""GPU: HipCodec::ReadRGBA through the C++ interface (j2k_host_test_read_rgba drives it like the three lines at the top of
RGBAinputFile::ReadFile would): the frame of every mode equals the model's, byte for byte; a file the fused path does not
take is "not taken" with the frame untouched; a damaged file throws."""
import ctypes as C
import os

import numpy as np
import pytest

import rgba_cases as rc
from j2k_amd import api

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
    return H


@pytest.fixture(scope="module")
def table():
    import json
    with open(os.path.join(rc.GOLDEN_DIR, "rgba", "rgba.json")) as f:
        return json.load(f)["cases"]


def read(host, data, case):
    frame, lay = rc.blank_frame(case)
    w, h = rc.image_size(case)
    buf = np.frombuffer(data, dtype=np.uint8)
    err = C.create_string_buffer(512)
    rc_ = host.j2k_host_test_read_rgba(buf.ctypes.data, len(data), case["subsample"], frame.ctypes.data, w, h, lay["rowbytes"], lay["sample_bytes"],
                                       case["bits"], int(case["demote"]), int(case["alpha"]), err, 512)
    return rc_, frame, err.value.decode()


@pytest.mark.parametrize("cid", ["k1-8", "k1-8-s2", "k1-16-noalpha-pad6", "j6-16-demote-pad8", "pal-8", "pal-16-demote", "j9-16-demote", "j9-16", "k2-16-s2-demote"])
def test_read_rgba_delivers_the_models_frame(host, table, cid):
    case = next(c for c in rc.cases() if c["id"] == cid)
    status, frame, err = read(host, rc.load(case["file"]), case)
    assert status == 1, err
    assert rc.sha(frame) == table[cid]


def test_a_file_of_the_other_path_is_not_taken(host):
    status, frame, err = read(host, rc.load("j7"), rc._case("j7", 8))
    assert status == 0 and (frame == rc.FILL).all()


def test_a_damaged_file_throws(host):
    data = rc.load("k1")
    for cut in (len(data) // 2, 30):
        status, frame, err = read(host, data[:cut], rc._case("k1", 8))
        assert status == -1 and err.startswith("Error reading file") and (frame == rc.FILL).all()
    status, frame, err = read(host, b"not a jpeg 2000 file at all", rc._case("k1", 8))
    assert status == -1 and err.startswith("Can't read this format")
