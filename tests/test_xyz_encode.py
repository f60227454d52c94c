"""GPU: whole files with j2k_hip_params.rgb_to_xyz.  The file written from R, G, B with the field set is byte for byte the
file written from the model's X'Y'Z' planes (xyz_model.py with the library's own tables) given as plain 12-bit planar input
without it -- which ties the feature to the paths libopenjp2 already pins; every entry point writes those bytes; the compare
calls take the X'Y'Z' codes as the source samples; HipCodec's CinemaXYZ option reaches the real cinema profile from a 16-bit world."""
import ctypes as C
import os

import numpy as np
import pytest

import xyz_model
from j2k_amd import api, synth

pytestmark = pytest.mark.gpu

J2K_HIP_ERR_PARAM = 1


@pytest.fixture(scope="module")
def enc():
    e = api.Encoder()
    yield e
    e.close()


def world(w, h, seed):
    """A 16-bit R, G, B world (ARGB64) and the model's 12-bit X'Y'Z' codes of it (source 1)."""
    pl = synth.planes(w, h, 3, 16, seed, "A")
    frame, lay = synth.ae_frame(pl, 16, row_pad_bytes=8)
    codes = xyz_model.codes(pl.astype(np.int64), 1, 16, 12, tables=api.xyz_tables(1, 16, 12))
    return pl, frame, lay, codes


CASES = {
    "53_97x61": (97, 61, dict(reversible=True, num_resolutions=4)),
    "dci2k_512x270": (512, 270, dict(dci_profile=3)),
    "97_rates_200x150": (200, 150, dict(reversible=False, ycc=True, rates=[20.0, 5.0])),
}


@pytest.fixture(scope="module")
def files(enc):
    """Per case: (world, the file from the model's planes without the field, the file from R, G, B with it)."""
    out = {}
    for name, (w, h, kw) in CASES.items():
        pl, frame, lay, codes = world(w, h, 7)
        want = enc.encode_planar_host(codes, api.make_params(w, h, 3, 12, **kw))
        got = enc.encode_host(frame, lay, api.make_params(w, h, 3, 12, rgb_to_xyz=1, **kw))
        out[name] = (pl, frame, lay, codes, want, got)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_file_equals_the_file_from_the_models_planes(files, name):
    _, _, _, _, want, got = files[name]
    assert len(want) > 200 and got == want


def test_lossless_file_decodes_to_the_models_codes(enc, files):
    _, _, _, codes, _, got = files["53_97x61"]
    info = api.read_info(got)
    assert (info["width"], info["height"], info["channels"], info["depth"]) == (97, 61, 3, 12)
    assert np.array_equal(enc.decode_planar(got).astype(np.int64), codes)


def test_the_other_sources_and_sample_types_write_their_models_file(enc):
    w, h = 97, 61
    pl = synth.planes(w, h, 3, 8, 3, "A")
    frame, lay = synth.ae_frame(pl, 8)
    p = dict(reversible=True, ycc=True, num_resolutions=4, cblk_style=1, tile_size=64)
    for source in (2, 3):
        codes = xyz_model.codes(pl.astype(np.int64), source, 8, 12, tables=api.xyz_tables(source, 8, 12))
        want = enc.encode_planar_host(codes, api.make_params(w, h, 3, 12, **p))
        assert enc.encode_host(frame, lay, api.make_params(w, h, 3, 12, rgb_to_xyz=source, **p)) == want
    # a float world of the same integers, under the JP2 wrapper
    pl16 = synth.planes(w, h, 3, 16, 4, "A")
    fframe, flay = synth.ae_frame_float(pl16, 16, row_pad_bytes=16)
    iframe, ilay = synth.ae_frame(pl16, 16)
    pj = api.make_params(w, h, 3, 12, reversible=False, num_resolutions=4, jp2=True, rgb_to_xyz=1)
    a, b = enc.encode_host(fframe, flay, pj), enc.encode_host(iframe, ilay, pj)
    assert a == b and a[4:8] == b"jP  "


def test_every_entry_point_writes_the_same_bytes(enc, files):
    L = enc.L
    pl, frame, lay, _, want, _ = files["53_97x61"]
    w, h, kw = CASES["53_97x61"]
    p = api.make_params(w, h, 3, 12, rgb_to_xyz=1, **kw)
    plain = api.make_params(w, h, 3, 12, **kw)
    before = enc.encode_host(frame, lay, plain)  # (rgb_to_xyz = 0 on the same handle, before and after)
    assert before != want
    api.tune("bands", 3)
    try:
        assert enc.encode_host(frame, lay, p) == want and enc.stats()["bands"] == 0
        assert enc.encode_host(frame, lay, p, via_sink=True) == want and enc.stats()["bands"] == 0
    finally:
        api.tune("bands", 0)
    enc.encode_begin_host(frame, lay, p)
    assert enc.encode_end() == want
    enc.encode_begin_borrowed(frame, lay, p)
    assert enc.encode_end() == want
    pl2, frame2, lay2, codes2 = world(w, h, 8)
    other = enc.encode_planar_host(codes2, plain)
    assert other != want
    d, d2 = enc.upload(frame), enc.upload(frame2)
    try:
        assert enc.encode_device(d, lay, p)[2] == want
        assert [f[2] for f in enc.encode_sequence_device([d, d2, d], lay, p)] == [want, other, want]
        # the tile-sharded entry points refuse before any device work and leave the handle usable
        with pytest.raises(api.J2kHipError) as ei:
            enc.encode_tiles_device(d, lay, p, 0, 1)
        assert ei.value.code == J2K_HIP_ERR_PARAM and "rgb_to_xyz" in str(ei.value)
    finally:
        enc.free(d)
        enc.free(d2)
    planes = api.planes_from_layout(frame.ctypes.data, lay, 3)
    out, n = np.empty(1 << 20, np.uint8), C.c_size_t()
    assert L.j2k_hip_encode_tiles(enc.h, C.byref(p), planes, 0, 1, out.ctypes.data, out.nbytes, C.byref(n)) == J2K_HIP_ERR_PARAM
    assert b"rgb_to_xyz" in L.j2k_hip_last_error(enc.h)
    # one process, several handles: the batch writes the same files; the distributed tiles refuse
    planes2 = api.planes_from_layout(frame2.ctypes.data, lay2, 3)
    both = (api.Plane * 6)(*(list(planes) + list(planes2)))
    chunks = [[], []]
    ids = (C.c_void_p * 2)(1, 2)

    @api.WRITE_FN
    def write(user, buf, nbytes):
        chunks[user - 1].append(C.string_at(buf, nbytes))
        return nbytes
    devs = (C.c_int * 2)(0, 0)
    assert L.j2k_hip_encode_batch(devs, 2, 1, C.byref(p), both, 2, write, ids) == 0, L.j2k_hip_multi_last_error()
    assert [b"".join(c) for c in chunks] == [want, other]
    assert L.j2k_hip_encode_tiles_distributed(devs, 2, C.byref(p), planes, write, 1) == J2K_HIP_ERR_PARAM
    assert b"rgb_to_xyz" in L.j2k_hip_multi_last_error()
    assert enc.encode_host(frame, lay, plain) == before


def test_tiles_inside_one_call(enc):
    w, h = 150, 130
    pl, frame, lay, codes = world(w, h, 9)
    kw = dict(reversible=True, ycc=True, num_resolutions=3, tile_size=64)
    want = enc.encode_planar_host(codes, api.make_params(w, h, 3, 12, **kw))
    assert enc.encode_host(frame, lay, api.make_params(w, h, 3, 12, rgb_to_xyz=1, **kw)) == want


def sums(s, d):
    e = d.astype(np.int64) - s.astype(np.int64)
    return dict(differing=int(np.count_nonzero(e)), sum_abs=int(np.abs(e).sum()), sum_sq=int((e * e).sum()), max_abs=int(np.abs(e).max()))


def test_compare_takes_the_codes_as_the_source(enc, files):
    pl, frame, lay, codes, _, got = files["53_97x61"]
    w, h, kw = CASES["53_97x61"]
    p = api.make_params(w, h, 3, 12, rgb_to_xyz=1)
    api.compare_check(p, got)
    same = enc.compare(got, p, frame=frame, layout=lay)
    assert [d["differing"] for d in same] == [0, 0, 0] and all(d["samples"] == w * h for d in same)
    # a file written from another seed: the sums numpy computes from the two model outputs
    _, frame2, lay2, codes2 = world(w, h, 8)
    file2 = enc.encode_host(frame2, lay2, api.make_params(w, h, 3, 12, rgb_to_xyz=1, **kw))
    want = [sums(codes[c], codes2[c]) for c in range(3)]
    assert all(x["differing"] > 0 for x in want)
    for diffs in (enc.compare(file2, p, frame=frame, layout=lay), enc.compare_device(file2, p, frame=frame, layout=lay)):
        assert [{k: d[k] for k in want[c]} for c, d in enumerate(diffs)] == want
    # the stage hook: decoded planes given by the caller
    diffs = enc.stage_compare([codes2[c] for c in range(3)], p, frame=frame, layout=lay)
    assert [{k: d[k] for k in want[c]} for c, d in enumerate(diffs)] == want
    # without the field the same file is compared against the depth-converted R, G, B: something else
    plain = enc.compare(got, api.make_params(w, h, 3, 12), frame=frame, layout=lay)
    assert all(d["differing"] > 0 for d in plain)


@pytest.fixture(scope="module")
def host():
    from j2k_amd import build
    path = os.path.join(os.path.dirname(api.LIBPATH), "libj2k_host.so")
    if not os.path.exists(path):
        build.build_host()
    api.load_library()
    H = C.CDLL(path)
    H.j2k_host_test_write_options.restype = C.c_long
    H.j2k_host_test_write_options.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.c_int, C.c_int, C.c_int, C.c_uint, C.c_void_p, C.c_ulong, C.c_char_p, C.c_ulong]
    return H


CINEMA_XYZ = 16  # HipCodec::CinemaXYZ


def _write(host, frame, lay, w, h, depth, options):
    out = np.empty(frame.nbytes + (1 << 20), dtype=np.uint8)
    err = C.create_string_buffer(512)
    n = host.j2k_host_test_write_options(frame.ctypes.data, w, h, lay["rowbytes"], lay["sample_bytes"], 3, depth, 1, 0, 1, 0, 1, options,
                                         out.ctypes.data, out.nbytes, err, 512)
    assert n >= 0, err.value.decode()
    return out[:n].tobytes()


def test_hip_codec_cinema_xyz_reaches_the_profile_from_a_16_bit_world(enc, host, files, monkeypatch):
    pl, frame, lay, codes, _, _ = files["dci2k_512x270"]
    w, h = 512, 270
    kb = 60  # (settings.fileSize: the frame's budget in KiB, as the CINEMA method has it)
    monkeypatch.setenv("J2K_HOST_TEST_FILESIZE_KB", str(kb))
    monkeypatch.setenv("J2K_HOST_TEST_CINEMA", "2")
    got = _write(host, frame, lay, w, h, 16, CINEMA_XYZ)
    assert got[6:8] == b"\x00\x03"  # Rsiz: the 2K cinema profile
    assert got == enc.encode_host(frame, lay, api.make_params(w, h, 3, 12, num_resolutions=6, dci_profile=3, max_cs_size=kb * 1024, rgb_to_xyz=1, comment=None))
    # without the option the 16-bit world keeps the non-profile branch, as before
    assert _write(host, frame, lay, w, h, 16, 0)[6:8] == b"\x00\x00"
    # an 8-bit and a float world reach it too
    pl8 = synth.planes(w, h, 3, 8, 5, "A")
    f8, l8 = synth.ae_frame(pl8, 8)
    got8 = _write(host, f8, l8, w, h, 8, CINEMA_XYZ)
    assert got8 == enc.encode_host(f8, l8, api.make_params(w, h, 3, 12, num_resolutions=6, dci_profile=3, max_cs_size=kb * 1024, rgb_to_xyz=1, comment=None))
    ff, fl = synth.ae_frame_float(pl, 16)
    assert _write(host, ff, fl, w, h, 16, CINEMA_XYZ) == got
    # without the CINEMA method the option asks for nothing
    monkeypatch.delenv("J2K_HOST_TEST_CINEMA")
    monkeypatch.delenv("J2K_HOST_TEST_FILESIZE_KB")
    assert _write(host, frame, lay, w, h, 16, CINEMA_XYZ) == _write(host, frame, lay, w, h, 16, 0)
