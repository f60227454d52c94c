"""GPU: decode only the first L quality layers of a file (j2k_hip_decode_set_max_layers).

The reference is strip(file, L) of tests/layers_cases.py -- the file cut down to its first L layers -- whose decodes
tests/golden/layers/layers.json holds (plain-C oracle / libopenjp2, tests/test_decode_layers_refs.py).  The planar decode is
held to those hashes; every other entry point to one rule: on the original file with the limit L it fills its whole
destination buffer exactly as the same entry point fills it for strip(file, L) with no limit.  Exact, no tolerance."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import layers_cases as lc
from j2k_amd import api, synth

pytestmark = pytest.mark.gpu

GUARD = 0xA5
L1, L2, L3, L4, L5, L6, L7 = lc.NAMES
PLAIN = [n for n in lc.NAMES if not lc.styled(n)]


@pytest.fixture(scope="module")
def enc():
    e = api.Encoder(0)
    yield e
    e.close()


@pytest.fixture
def limit(enc):
    """Sets the handle's layer limit for one test and puts 0 back."""
    yield enc.set_max_layers
    enc.set_max_layers(0)


@pytest.fixture
def knobs():
    """Sets tuning knobs for one test and puts back what they were."""
    before = {}

    def tune(key, value):
        before.setdefault(key, api.get_tune(key))
        api.tune(key, value)
    yield tune
    for k, v in before.items():
        api.tune(k, v)


_cache = {}


def variant(name, sop, L=None):
    """The fixture (sop) or its SOP-less copy, whole (L = None) or cut down to its first L layers; made once."""
    key = (name, sop, L)
    if key not in _cache:
        cs = lc.load(name) if L is None else lc.strip(lc.load(name), L)
        _cache[key] = cs if sop else lc.drop_sop(cs)
    return _cache[key]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def check_comp_hashes(comps, dec, what):
    """dec (channels, h, w) against the committed per-component hashes: a sub-sampled component is replicated onto the channel's grid."""
    assert len(comps) == dec.shape[0], what
    for c, exp in enumerate(comps):
        dx, dy = exp["dx"], exp["dy"]
        own = dec[c][::dy, ::dx].astype(np.int32)
        assert list(own.shape) == exp["shape"] and sha(own) == exp["sha256"], (what, c)
        assert np.array_equal(dec[c], np.repeat(np.repeat(dec[c][::dy, ::dx], dy, axis=0), dx, axis=1)[:dec.shape[1], :dec.shape[2]]), (what, c)


# ------------------------------------------------------------------------------------------------ the planar decode against layers.json
@pytest.mark.parametrize("sop", [True, False], ids=["sop", "nosop"])
@pytest.mark.parametrize("name", lc.NAMES)
def test_planar_decode_equals_the_committed_hashes(enc, limit, name, sop):
    data = variant(name, sop)
    for L in range(1, lc.layers_of(name) + 1):
        limit(L)
        for sub in (1, 2):
            dec = enc.decode_planar(data, subsample=sub)
            check_comp_hashes(lc.meta()[name]["decoded"][str(L)][str(sub.bit_length() - 1)], dec, (name, L, sub))


@pytest.mark.parametrize("name", lc.NAMES)
def test_zero_all_and_more_layers_are_the_whole_decode(enc, limit, name):
    data, layers = lc.load(name), lc.layers_of(name)
    fresh = api.Encoder(0)
    try:
        assert fresh.max_layers() == 0
        full = fresh.decode_planar(data)
        full_work, full_kernels, full_blocks = fresh.decode_work(), fresh.decode_kernels(), fresh.stats()["num_codeblocks"]
    finally:
        fresh.close()
    check_comp_hashes(lc.meta()[name]["decoded"][str(layers)]["0"], full, name)
    for L in (0, layers, layers + 1000):
        limit(L)
        assert enc.max_layers() == L
        got = enc.decode_planar(data)
        assert got.tobytes() == full.tobytes(), (name, L)
        assert (enc.decode_work(), enc.decode_kernels(), enc.stats()["num_codeblocks"]) == (full_work, full_kernels, full_blocks), (name, L)
    # sticky until set again: 1, then 0
    limit(1)
    first = enc.decode_planar(data)
    assert enc.max_layers() == 1 and not np.array_equal(first, full)
    assert np.array_equal(first, enc.decode_planar(data))  # (still set)
    check_comp_hashes(lc.meta()[name]["decoded"]["1"]["0"], first, name)
    limit(0)
    assert enc.max_layers() == 0 and enc.decode_planar(data).tobytes() == full.tobytes()


@pytest.mark.parametrize("lanes", [0, 2], ids=["waves", "lanes"])
@pytest.mark.parametrize("name", PLAIN)
def test_both_tier1_kernels(enc, limit, knobs, name, lanes):
    knobs("t1dec_lanes", lanes)
    data = lc.load(name)
    for L in range(1, lc.layers_of(name) + 1):
        limit(L)
        dec = enc.decode_planar(data)
        lane_blocks, wave_blocks = enc.decode_kernels()
        assert (lane_blocks == 0 and wave_blocks > 0) if lanes == 0 else lane_blocks > 0, (name, L, lane_blocks, wave_blocks)
        assert lane_blocks + wave_blocks == enc.stats()["num_codeblocks"]
        check_comp_hashes(lc.meta()[name]["decoded"][str(L)]["0"], dec, (name, L, lanes))


@pytest.mark.parametrize("name", [n for n in lc.NAMES if lc.meta()[n]["oracle_reads"]])
def test_decode_work_counts_the_kept_passes_and_bytes(enc, limit, oracle, name):
    data = lc.load(name)
    seen = []
    for L in range(1, lc.layers_of(name) + 1):
        blocks = oracle.file_blocks(lc.strip(data, L))["blocks"]
        limit(L)
        enc.decode_planar(data)
        passes, cw_bytes = enc.decode_work()
        assert passes == sum(b["npasses"] for b in blocks) == lc.meta()[name]["passes"][L - 1], (name, L)
        assert cw_bytes == sum(len(b["data"]) for b in blocks), (name, L)
        assert enc.stats()["num_codeblocks"] == len(blocks) == lc.meta()[name]["blocks_with_passes"][L - 1], (name, L)
        seen.append(passes)
    if name == L1:
        assert all(a < b for a, b in zip(seen, seen[1:])), seen
    # a sequence call: summed over its frames
    limit(1)
    enc.decode_sequence_planar([data, data, data])
    assert enc.decode_work()[0] == 3 * seen[0]


# ------------------------------------------------------------------------------------------------ every other entry point: one rule
def same_fill(enc, call, whole, cut, L):
    """call(data) -> the destination buffer it filled (made afresh, guard bytes everywhere): with the limit L on the whole file
    against no limit on the cut file."""
    enc.set_max_layers(L)
    got = call(whole)
    enc.set_max_layers(0)
    want = call(cut)
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    return got


def guarded(shape, dtype):
    a = np.empty(shape, dtype=dtype)
    a.view(np.uint8)[...] = GUARD
    return a


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_region_off_the_block_grid(enc, limit, device):
    rect = (37, 21, 48, 40)
    data = lc.load(L3)
    seen = set()
    for L in range(1, lc.layers_of(L3) + 1):
        got = same_fill(enc, lambda d: enc.decode_region_planar(d, rect, out=guarded((3, 44, 52), np.uint16), device=device), data, lc.strip(data, L), L)
        assert (got[:, :40, :48].view(np.uint8) != GUARD).any() and (got[:, 40:, :].view(np.uint8) == GUARD).all() and (got[:, :, 48:].view(np.uint8) == GUARD).all()
        seen.add(got.tobytes())
    assert len(seen) == lc.layers_of(L3)
    # ... and at half size, the SOP-less copy
    for L in (1, 2):
        same_fill(enc, lambda d: enc.decode_region_planar(d, (18, 10, 24, 20), subsample=2, out=guarded((3, 20, 24), np.uint16), device=device),
                  variant(L3, False), variant(L3, False, L), L)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name,bits", [(L2, 8), (L3, 16), (L1, 8), (L4, 16), (L6, 8)], ids=["l2-8", "l3-16", "l1-8", "l4-16", "l6-8"])
def test_decode_rgba_into_packed_argb(enc, limit, name, bits, device):
    w, h = lc.CASES[name][0], lc.CASES[name][1]
    _, lay = synth.ae_frame(np.zeros((3, h, w), dtype=np.int32), bits, row_pad_bytes=8)

    def call(d):
        return enc.decode_rgba(d, guarded(h * lay["rowbytes"], np.uint8), lay, w, h, device=device)
    data = lc.load(name)
    seen = set()
    for L in range(1, lc.layers_of(name) + 1):
        seen.add(same_fill(enc, call, data, lc.strip(data, L), L).tobytes())
    assert len(seen) == lc.layers_of(name)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_device_forms_of_the_planar_decode(enc, limit, device):
    """j2k_hip_decode[_device] into the samples of an After Effects frame (every other byte stays)."""
    for name, bits in ((L2, 8), (L5, 16)):
        w, h, nc = lc.CASES[name][:3]
        _, lay = synth.ae_frame(np.zeros((3, h, w), dtype=np.int32), bits)
        data = lc.load(name)
        for L in range(1, lc.layers_of(name)):
            same_fill(enc, lambda d: enc.decode_ae(d, guarded(h * lay["rowbytes"], np.uint8), lay, w, h, nc, device=device), data, lc.strip(data, L), L)


@pytest.mark.parametrize("group", [0, 1], ids=["grouped", "frame-by-frame"])
@pytest.mark.parametrize("name", [L1, L3, L4, L5])
def test_three_frame_sequence(enc, limit, knobs, name, group):
    knobs("decseq_group", group)
    layers = lc.layers_of(name)
    w, h, nc, prec = lc.CASES[name][:4]
    dt = np.uint8 if prec <= 8 else np.uint16
    whole = [variant(name, True), variant(name, False), variant(name, True)]
    _, lay = synth.ae_frame(np.zeros((3, h, w), dtype=np.int32), 8 if prec <= 8 else 16)
    for L in range(1, layers):
        cut = [variant(name, True, L), variant(name, False, L), variant(name, True, L)]
        for device in (False, True):
            got = same_fill(enc, lambda f: enc.decode_sequence_planar(f, out=guarded((3, nc, h + 3, w + 5), dt), device=device), whole, cut, L)
            assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])
            check_comp_hashes(lc.meta()[name]["decoded"][str(L)]["0"], got[0][:, :h, :w], (name, L))
            same_fill(enc, lambda f: enc.decode_rgba_sequence(f, guarded((3, h * lay["rowbytes"]), np.uint8), lay, w, h, device=device), whole, cut, L)
        same_fill(enc, lambda f: enc.decode_sequence_planar(f, subsample=2, region=(3, 2, 20, 17), out=guarded((3, nc, 17, 20), dt)), whole, cut, L)


def test_jp2_wrapped_file(enc, limit):
    """The layer limit reads the codestream inside the boxes."""
    w, h, nc, prec = lc.CASES[L1][:4]
    p = api.make_params(w, h, nc, prec, jp2=True, color_space=2)
    data = lc.load(L1)

    def wrap(cs):
        return api.file_header(p, len(cs)) + cs
    assert api.read_info(wrap(data))["layers"] == 4 and wrap(data)[4:8] == b"jP  "
    _, lay = synth.ae_frame(np.zeros((3, h, w), dtype=np.int32), 8)
    for L in range(1, 4):
        got = same_fill(enc, lambda d: enc.decode_planar(d, out=guarded((nc, h, w), np.uint8)), wrap(data), wrap(lc.strip(data, L)), L)
        check_comp_hashes(lc.meta()[L1]["decoded"][str(L)]["0"], got, L)
        same_fill(enc, lambda d: enc.decode_rgba(d, guarded(h * lay["rowbytes"], np.uint8), lay, w, h), wrap(data), wrap(lc.strip(data, L)), L)


# ------------------------------------------------------------------------------------------------ HipCodec::SetReadLayers
@pytest.fixture(scope="module")
def host():
    from j2k_amd import build
    path = os.path.join(os.path.dirname(api.LIBPATH), "libj2k_host.so")
    if not os.path.exists(path):
        build.build_host()
    api.load_library()
    H = C.CDLL(path)
    H.j2k_host_test_read.restype = C.c_long
    H.j2k_host_test_read.argtypes = [C.c_void_p, C.c_ulong, C.c_uint, C.c_void_p, C.c_uint, C.c_uint, C.c_long, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_ulong]
    H.j2k_host_test_read_rgba.restype = C.c_long
    H.j2k_host_test_read_rgba.argtypes = [C.c_void_p, C.c_ulong, C.c_uint, C.c_void_p, C.c_uint, C.c_uint, C.c_long, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.c_char_p, C.c_ulong]
    H.j2k_host_test_read_files.restype = C.c_long
    H.j2k_host_test_read_files.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_ulong), C.c_uint, C.c_uint, C.c_void_p, C.c_uint, C.c_uint, C.c_int,
                                           C.c_char_p, C.c_ulong]
    return H


def test_hip_codec_set_read_layers(host, monkeypatch):
    """ReadFile, ReadRGBA and ReadFiles through the C++ interface (the hook's J2K_HOST_TEST_READ_LAYERS knob calls
    HipCodec::SetReadLayers): the whole file with L against the cut file without; a codec object without the setting reads
    in full again on the same thread's handle."""
    name = L2
    w, h, nc = lc.CASES[name][:3]
    data = lc.load(name)
    rb = 4 * w + 12

    def read_file(d):
        frame, err = guarded(rb * h, np.uint8), C.create_string_buffer(512)
        buf = np.frombuffer(d, dtype=np.uint8)
        assert host.j2k_host_test_read(buf.ctypes.data, len(d), 1, frame.ctypes.data, w, h, rb, 1, nc, 8, err, 512) == 0, err.value.decode()
        return frame

    def read_rgba(d):
        frame, err = guarded(rb * h, np.uint8), C.create_string_buffer(512)
        buf = np.frombuffer(d, dtype=np.uint8)
        assert host.j2k_host_test_read_rgba(buf.ctypes.data, len(d), 1, frame.ctypes.data, w, h, rb, 1, 8, 0, 1, err, 512) == 1, err.value.decode()
        return frame

    def read_files(files):
        bufs = [np.frombuffer(d, dtype=np.uint8) for d in files]
        ptrs = (C.c_void_p * len(files))(*[b.ctypes.data for b in bufs])
        lens = (C.c_ulong * len(files))(*[len(d) for d in files])
        frames, err = guarded((len(files), nc * w * h), np.uint8), C.create_string_buffer(512)
        assert host.j2k_host_test_read_files(ptrs, lens, len(files), 1, frames.ctypes.data, w, h, nc, err, 512) == 1, err.value.decode()
        return frames

    full = [read_file(data), read_rgba(data), read_files([data, variant(name, False)])]
    seen = {full[0].tobytes()}
    for L in range(1, lc.layers_of(name)):
        cut = lc.strip(data, L)
        monkeypatch.setenv("J2K_HOST_TEST_READ_LAYERS", str(L))
        got = [read_file(data), read_rgba(data), read_files([data, variant(name, False)])]
        monkeypatch.delenv("J2K_HOST_TEST_READ_LAYERS")
        want = [read_file(cut), read_rgba(cut), read_files([cut, variant(name, False, L)])]
        for g, x in zip(got, want):
            assert g.tobytes() == x.tobytes(), L
        seen.add(got[0].tobytes())
        again = [read_file(data), read_rgba(data)]
        assert again[0].tobytes() == full[0].tobytes() and again[1].tobytes() == full[1].tobytes()
    assert len(seen) == lc.layers_of(name)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(enc):
    L = api.load_library()
    v = C.c_uint32(7)
    a, b = C.c_uint64(), C.c_uint64()
    assert L.j2k_hip_decode_set_max_layers(None, 1) == 1  # J2K_HIP_ERR_PARAM
    assert L.j2k_hip_decode_get_max_layers(None, C.byref(v)) == 1 and v.value == 7
    assert L.j2k_hip_debug_decode_work(None, C.byref(a), C.byref(b)) == 1
    assert L.j2k_hip_decode_get_max_layers(enc.h, None) == 1
    # between j2k_hip_encode_begin_borrowed and its _end the handle refuses the setter like every other call
    w, h = 64, 48
    pl = synth.planes(w, h, 1, 8, 9)
    frame, lay = synth.ae_frame(pl, 8)
    p = api.make_params(w, h, 1, 8, num_resolutions=3)
    e = api.Encoder(0)
    try:
        e.set_max_layers(2)
        e.encode_begin_borrowed(frame, lay, p)
        with pytest.raises(api.J2kHipError, match="in progress"):
            e.set_max_layers(1)
        with pytest.raises(api.J2kHipError, match="in progress"):
            e.max_layers()
        cs = e.encode_end()
        assert e.max_layers() == 2  # (the refused call changed nothing; an encode does not touch the setting)
        assert np.array_equal(e.decode_planar(cs), pl)
    finally:
        e.close()
