"""GPU: whole files through j2k_hip_decode_rgba[_device] / _rgba_sequence[_device] with j2k_hip_decode_set_xyz_to_rgb set: the
frame equals the numpy model (xyz_inverse_model.py, the library's own tables) applied to what the PLANAR decode of the same
call delivers -- the existing decode tests hold that to libopenjp2 -- byte for byte over the whole frame buffer.  The two
cinema goldens (2K; 4K with its progression order change), the whole image, a region, subsample 2, the device form and a
two-frame sequence call; an own lossless X'Y'Z' encode read back against its source; the setting switched off again; the
refusals; and HipCodec::ReadRGBA with SetReadCinemaColour through the C++ interface."""
import ctypes as C
import os

import numpy as np
import pytest

import rgba_model as rm
import xyz_inverse_model as xim
import xyz_model
from conftest import GOLDEN_DIR
from j2k_amd import api, synth

pytestmark = pytest.mark.gpu

J2K_HIP_ERR_PARAM = 1
FILL = 0xA5
D1 = os.path.join("ext", "d1_512x270_rgb12_cinema2k.j2k")
D2 = os.path.join("ext", "d2_1024x540_rgb12_cinema4k_poc.j2k")


def load(name):
    with open(os.path.join(GOLDEN_DIR, name), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def enc():
    e = api.Encoder(0)
    yield e
    e.set_xyz_to_rgb(0)
    e.close()


_tables = {}


def tables(target, comp_depth, dst_depth):
    key = (target, comp_depth, dst_depth)
    if key not in _tables:
        _tables[key] = api.xyz_inverse_tables(target, comp_depth, dst_depth)
    return _tables[key]


def blank(w, h, bits, pad=0):
    frame, lay = synth.ae_frame(np.zeros((4, h, w), dtype=np.int32), bits, row_pad_bytes=pad)
    frame[:] = FILL
    return frame, lay


def expected(planar, target, prec, bits, pad=0, alpha=True):
    """The A,R,G,B frame the RGBA call must leave: the model of the planar decode's samples, A filled with the top."""
    _, h, w = planar.shape
    rgb = xim.rgb(planar.astype(np.int64), target, prec, bits, tables(target, prec, bits))
    frame, lay = blank(w, h, bits, pad)
    return rm.into_ae_frame(frame, lay, list(rgb) + [np.full((h, w), (1 << bits) - 1, dtype=np.int64)], alpha)


_planar = {}


def planar_of(enc, name, subsample=1):
    """The planar decode of a golden at its own depth, once per file and subsample (the reference of every case below)."""
    key = (name, subsample)
    if key not in _planar:
        _planar[key] = enc.decode_planar(load(name), subsample=subsample)
    return _planar[key]


# ------------------------------------------------------------------------------------------------ the cinema goldens
@pytest.mark.parametrize("name", [D1, D2], ids=["2k", "4k-poc"])
@pytest.mark.parametrize("target", [1, 2, 3])
def test_cinema_golden_whole_image_region_subsample_and_device(enc, name, target):
    data = load(name)
    full = planar_of(enc, name)
    assert full.shape[0] == 3 and full.dtype == np.uint16 and full.max() < 4096
    _, h, w = full.shape
    enc.set_xyz_to_rgb(target)
    assert enc.xyz_to_rgb() == target
    try:
        for bits, device in ((8, False), (16, True)):
            frame, lay = blank(w, h, bits, pad=8)
            got = enc.decode_rgba(data, frame, lay, w, h, device=device)
            assert got.tobytes() == expected(full, target, 12, bits, pad=8).tobytes(), (bits, device)
        x, y, rw, rh = 255, 129, 131, 67  # a window across the workgroup's 256th column, odd in every number
        for bits, device in ((16, False), (8, True)):
            frame, lay = blank(rw, rh, bits)
            got = enc.decode_rgba(data, frame, lay, rw, rh, region=(x, y, rw, rh), device=device, alpha=bits == 16)
            assert got.tobytes() == expected(full[:, y:y + rh, x:x + rw], target, 12, bits, alpha=bits == 16).tobytes(), ("region", bits)
        half = planar_of(enc, name, 2)
        _, h2, w2 = half.shape
        frame, lay = blank(w2, h2, 8)
        got = enc.decode_rgba(data, frame, lay, w2, h2, subsample=2)
        assert got.tobytes() == expected(half, target, 12, 8).tobytes()
        frame, lay = blank(40, 30, 16)
        got = enc.decode_rgba(data, frame, lay, 40, 30, subsample=2, region=(w2 - 40, h2 - 30, 40, 30), device=True)
        assert got.tobytes() == expected(half[:, h2 - 30:, w2 - 40:], target, 12, 16).tobytes()
        # the planar calls ignore the setting
        assert enc.decode_planar(data).tobytes() == full.tobytes()
    finally:
        enc.set_xyz_to_rgb(0)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_two_frame_sequence_call(enc, device):
    """Two frames of one geometry in one call: the golden, and the library's own cinema encode of another picture."""
    data = load(D1)
    pl = synth.planes(512, 270, 3, 12, 31)
    src, slay = synth.ae_frame(pl, 12)
    other = enc.encode_host(src, slay, api.make_params(512, 270, 3, 12, dci_profile=3))
    api.sequence_check([data, other])
    refs = [planar_of(enc, D1), enc.decode_planar(other)]
    for target, bits in ((1, 8), (2, 16)):
        enc.set_xyz_to_rgb(target)
        try:
            one, lay = blank(512, 270, bits)
            frames = np.stack([one, one])
            got = enc.decode_rgba_sequence([data, other], frames, lay, 512, 270, device=device)
            for f in range(2):
                assert got[f].tobytes() == expected(refs[f], target, 12, bits).tobytes(), (target, f)
            frames = np.stack([blank(100, 50, bits)[0]] * 2)
            lay = blank(100, 50, bits)[1]
            got = enc.decode_rgba_sequence([other, data], frames, lay, 100, 50, region=(200, 100, 100, 50), device=device)
            for f in range(2):
                assert got[f].tobytes() == expected(refs[1 - f][:, 100:150, 200:300], target, 12, bits).tobytes(), (target, "region", f)
        finally:
            enc.set_xyz_to_rgb(0)


def test_a_file_with_subsampled_components(enc):
    """A raw 4:2:0 file without a colour space is RGB mode: components 1 and 2 are replicated, then converted (as codes)."""
    name = os.path.join("ext", "u1_300x200_ycc420_8_53.j2k")
    data, ref = load(name), planar_of(enc, name)
    enc.set_xyz_to_rgb(3)
    try:
        for region in (None, (1, 1, 255, 101), (3, 2, 2, 3)):
            w, h = (300, 200) if region is None else region[2:]
            want = ref if region is None else ref[:, region[1]:region[1] + h, region[0]:region[0] + w]
            got = enc.decode_rgba(data, *blank(w, h, 16), w, h, region=region)
            assert got.tobytes() == expected(want, 3, 8, 16).tobytes(), region
    finally:
        enc.set_xyz_to_rgb(0)


# ------------------------------------------------------------------------------------------------ there and back
def test_own_lossless_cinema_encode_comes_back_within_the_measured_error(enc):
    """5/3, rgb_to_xyz = 1, depth 12, a 97 x 61 8-bit frame: the file holds exactly the model's codes, the read with target 1 at
    D = 8 is the model of those codes, and no channel is further from the source than the worst error of the round trip over all
    2^24 colours (xyz_inverse_model.ROUND_TRIP_8BIT, asserted by test_xyz_inverse_host.py)."""
    w, h = 97, 61
    pl = synth.planes(w, h, 3, 8, 5)
    pl[:, 0, :6] = [[0, 255, 255, 0, 0, 7], [0, 255, 0, 255, 0, 253], [0, 255, 0, 0, 255, 172]]  # (the last: the worst colour of target 1)
    src, slay = synth.ae_frame(pl, 8)
    cs = enc.encode_host(src, slay, api.make_params(w, h, 3, 12, reversible=True, rgb_to_xyz=1, num_resolutions=4))
    codes = xyz_model.codes(pl, 1, 8, 12, tables=api.xyz_tables(1, 8, 12))
    assert np.array_equal(enc.decode_planar(cs), codes)
    enc.set_xyz_to_rgb(1)
    try:
        frame, lay = blank(w, h, 8)
        got = enc.decode_rgba(cs, frame, lay, w, h)
        r, g, b = np.empty((h, w), np.uint8), np.empty((h, w), np.uint8), np.empty((h, w), np.uint8)
        enc.decode_rgba_channels(cs, r, g, b)
    finally:
        enc.set_xyz_to_rgb(0)
    assert got.tobytes() == expected(codes.astype(np.uint16), 1, 12, 8).tobytes()
    back = np.stack([r, g, b]).astype(np.int64)
    assert np.array_equal(back, xim.rgb(codes, 1, 12, 8, tables(1, 12, 8)))
    err = np.abs(back - pl)
    print(f"worst error against the source {int(err.max())}, {int((err.max(axis=0) == 0).sum())} of {w * h} pixels exact")
    assert err.max() <= xim.ROUND_TRIP_8BIT[1][0]
    assert err[:, 0, 5].max() == xim.ROUND_TRIP_8BIT[1][0]  # (and the bound is met where the exhaustive run found it)


# ------------------------------------------------------------------------------------------------ off again, and a fresh handle
def test_set_1_then_0_is_a_fresh_handles_call(enc):
    fresh = api.Encoder(0)
    try:
        assert fresh.xyz_to_rgb() == 0
        for name in (D1, os.path.join("g3_300x200_rgb8_53_rct.j2k"), os.path.join("rgba", "k1_37x21_sycc420_8_53.jp2"), "j6_40x30_greya8.jp2"):
            data = load(name)
            i = api.read_info(data)
            w, h = i["width"], i["height"]
            want = fresh.decode_rgba(data, *blank(w, h, 16, pad=4), w, h)
            enc.set_xyz_to_rgb(1)
            enc.set_xyz_to_rgb(0)
            assert enc.xyz_to_rgb() == 0
            assert enc.decode_rgba(data, *blank(w, h, 16, pad=4), w, h).tobytes() == want.tobytes(), name
    finally:
        fresh.close()


def test_read_profile_of_the_goldens():
    assert api.read_profile(load(D1)) == 3 and api.read_profile(load(D2)) == 4
    assert api.read_profile(load("g3_300x200_rgb8_53_rct.j2k")) == 0


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_the_setting_and_write_nothing(enc):
    with pytest.raises(api.J2kHipError) as ei:
        enc.set_xyz_to_rgb(4)
    assert ei.value.code == J2K_HIP_ERR_PARAM and "xyz_to_rgb" in str(ei.value) and enc.xyz_to_rgb() == 0
    assert api.load_library().j2k_hip_decode_get_xyz_to_rgb(enc.h, None) == J2K_HIP_ERR_PARAM
    enc.set_xyz_to_rgb(2)
    try:
        for name in ("j6_40x30_greya8.jp2", "g1_64x64_grey_5lvl.j2k", "j5_64x48_rgb8_sycc_97.jp2", os.path.join("rgba", "k1_37x21_sycc420_8_53.jp2")):
            data = load(name)
            i = api.read_info(data)
            w, h = i["width"], i["height"]
            for device in (False, True):
                frame, lay = blank(w, h, 8)
                with pytest.raises(api.J2kHipError) as ei:
                    enc.decode_rgba(data, frame, lay, w, h, device=device)
                assert ei.value.code == J2K_HIP_ERR_PARAM and "xyz_to_rgb" in str(ei.value), (name, str(ei.value))
                assert (frame == FILL).all()
            frames = np.stack([blank(w, h, 8)[0]] * 2)
            with pytest.raises(api.J2kHipError) as ei:
                enc.decode_rgba_sequence([data, data], frames, blank(w, h, 8)[1], w, h)
            assert ei.value.code == J2K_HIP_ERR_PARAM and "xyz_to_rgb" in str(ei.value) and (frames == FILL).all()
        # a palette: crafted from the grey JP2 as the RGBA tests do
        import rgba_cases as rc
        data = rc.load("pal")
        frame, lay = blank(64, 48, 8)
        with pytest.raises(api.J2kHipError) as ei:
            enc.decode_rgba(data, frame, lay, 64, 48)
        assert ei.value.code == J2K_HIP_ERR_PARAM and "xyz_to_rgb" in str(ei.value) and (frame == FILL).all()
        # signed components (the 2K golden with the sign bits of its SIZ set), and components 0..2 of unlike precision (an 8-bit
        # RGB file without a component transform whose third component says 7 bits): the header alone decides
        signed = bytearray(load(D1))
        unlike = bytearray(load("g5_300x200_rgb8_53_ref_literal.j2k"))
        for k in range(3):
            signed[42 + 3 * k] |= 0x80  # (SOC, SIZ marker, Lsiz, 36 bytes, then Ssiz / XRsiz / YRsiz per component)
        unlike[42 + 3 * 2] = 6
        assert api.read_info(bytes(signed))["comp_signed"][:3] == [1, 1, 1] and api.rgba_mode(bytes(signed)) == rm.RGB
        assert api.read_info(bytes(unlike))["comp_depth"][:3] == [8, 8, 7] and api.rgba_mode(bytes(unlike)) == rm.RGB
        for bad, (w, h), word in ((bytes(signed), (512, 270), "signed"), (bytes(unlike), (300, 200), "precision")):
            frame, lay = blank(w, h, 8)
            with pytest.raises(api.J2kHipError) as ei:
                enc.decode_rgba(bad, frame, lay, w, h)
            assert ei.value.code == J2K_HIP_ERR_PARAM and "xyz_to_rgb" in str(ei.value) and word in str(ei.value), str(ei.value)
            assert (frame == FILL).all()
        # the same files decode as ever once the setting is off, and an RGB file converts on the same handle
        enc.set_xyz_to_rgb(0)
        frame, lay = blank(64, 48, 8)
        enc.decode_rgba(data, frame, lay, 64, 48)
        assert not (frame == FILL).all()
    finally:
        enc.set_xyz_to_rgb(0)


def test_a_pending_borrowed_encode_refuses_the_setter(enc):
    w, h = 64, 48
    pl = synth.planes(w, h, 1, 8, 9)
    frame, lay = synth.ae_frame(pl, 8)
    e = api.Encoder(0)
    try:
        e.set_xyz_to_rgb(3)
        e.encode_begin_borrowed(frame, lay, api.make_params(w, h, 1, 8, num_resolutions=3))
        with pytest.raises(api.J2kHipError, match="xyz_to_rgb.*in progress"):
            e.set_xyz_to_rgb(1)
        with pytest.raises(api.J2kHipError, match="in progress"):
            e.xyz_to_rgb()
        cs = e.encode_end()
        assert e.xyz_to_rgb() == 3  # (the refused call changed nothing; an encode does not touch the setting)
        assert np.array_equal(e.decode_planar(cs), pl)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ HipCodec::ReadRGBA
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


def host_read(host, data, w, h, bits):
    frame, lay = blank(w, h, bits)
    buf = np.frombuffer(data, dtype=np.uint8)
    err = C.create_string_buffer(512)
    rc_ = host.j2k_host_test_read_rgba(buf.ctypes.data, len(data), 1, frame.ctypes.data, w, h, lay["rowbytes"], lay["sample_bytes"], bits, 0, 1, err, 512)
    return rc_, frame, err.value.decode()


def test_hip_codec_set_read_cinema_colour(enc, host, monkeypatch):
    """SetReadCinemaColour through the hook's J2K_HOST_TEST_READ_CINEMA knob: on, off, and profileFilesOnly on a file that is
    no cinema frame; without profileFilesOnly that file converts too, and a grey file throws."""
    d1, g3, grey = load(D1), load("g3_300x200_rgb8_53_rct.j2k"), load("g1_64x64_grey_5lvl.j2k")
    ref_d1, ref_g3 = planar_of(enc, D1), planar_of(enc, "g3_300x200_rgb8_53_rct.j2k")
    plain_d1 = host_read(host, d1, 512, 270, 16)
    plain_g3 = host_read(host, g3, 300, 200, 8)
    assert plain_d1[0] == 1 and plain_g3[0] == 1, (plain_d1[2], plain_g3[2])
    for target in (1, 3):
        monkeypatch.setenv("J2K_HOST_TEST_READ_CINEMA", str(target))
        status, frame, err = host_read(host, d1, 512, 270, 16)
        assert status == 1, err
        assert frame.tobytes() == expected(ref_d1, target, 12, 16).tobytes()
        status, frame, err = host_read(host, g3, 300, 200, 8)  # Rsiz 0: read as without the setting
        assert status == 1 and frame.tobytes() == plain_g3[1].tobytes(), err
        status, frame, err = host_read(host, grey, 64, 64, 8)
        assert status == 1, err
        monkeypatch.setenv("J2K_HOST_TEST_READ_CINEMA_ALL", "1")
        status, frame, err = host_read(host, g3, 300, 200, 8)
        assert status == 1 and frame.tobytes() == expected(ref_g3, target, 8, 8).tobytes(), err
        status, frame, err = host_read(host, grey, 64, 64, 8)
        assert status == -1 and "xyz_to_rgb" in err and (frame == FILL).all()
        monkeypatch.delenv("J2K_HOST_TEST_READ_CINEMA_ALL")
    monkeypatch.setenv("J2K_HOST_TEST_READ_CINEMA", "7")
    status, frame, err = host_read(host, d1, 512, 270, 16)
    assert status == -1 and "xyz_to_rgb" in err and (frame == FILL).all()
    monkeypatch.setenv("J2K_HOST_TEST_READ_CINEMA", "0")
    status, frame, err = host_read(host, d1, 512, 270, 16)
    assert status == 1 and frame.tobytes() == plain_d1[1].tobytes()
    monkeypatch.delenv("J2K_HOST_TEST_READ_CINEMA")
    status, frame, err = host_read(host, d1, 512, 270, 16)  # a codec object without the setting, on the same thread's handle
    assert status == 1 and frame.tobytes() == plain_d1[1].tobytes()
