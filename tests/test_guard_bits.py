"""GPU: frames at and beyond the bit-planes their sub-bands signal (tests/guard_cases.py; tests/test_guard_bits_refs.py holds
the references on the CPU).

An at_limit frame -- a block with exactly Mb bit-planes, zero-bit-plane count 0 -- encodes byte-exactly through every entry
point and decodes back to itself.  An `over` frame -- a block with Mb + 1 -- is refused by every entry point with
J2K_HIP_ERR_OVERFLOW and the guard-bits text: no codestream, not one byte to a sink, no output pointer or length written; the
handle then takes a frame of another geometry, a benign frame of the same geometry, a begin / end pair and a three-frame
sequence, all byte-exact.  The error comes from host Tier-2 (test_guard_bits_refs.py: every `over` block fits its Tier-1
slots), never from a device fault.  What libopenjp2 writes for such a frame decodes here as it decodes there."""
import ctypes as C
import os

import numpy as np
import pytest

import guard_cases as gc
from conftest import golden_case

pytestmark = pytest.mark.gpu

J2K_HIP_ERR_OVERFLOW = 4
GUARD_TEXT = "code-block has more bit-planes than its sub-band signals (guard bits exceeded)"
OTHER = "g1_64x64_grey_5lvl"  # the golden frame of another geometry
SENTINEL = 0x5a5a5a5a


@pytest.fixture(scope="module")
def api():
    from j2k_amd import api
    return api


@pytest.fixture
def enc(api):
    e = api.Encoder(0)
    yield e
    e.close()


@pytest.fixture
def bands3(api):
    before = api.get_tune("bands")
    api.tune("bands", 3)
    yield
    api.tune("bands", before)


class Src:
    """A frame of a case on a handle: the After Effects buffer on the host and on the device."""

    def __init__(self, api, e, c, planes):
        from j2k_amd import synth
        self.api, self.e, self.c = api, e, c
        self.frame, self.lay = synth.ae_frame(planes, c.prec)
        self.p = gc.api_params(api, c)
        self.d = e.upload(self.frame)

    def close(self):
        self.e.free(self.d)

    def views(self, addr):
        return self.api.planes_from_layout(addr, self.lay, self.c.nc)


def _sequence(s, others):
    """Three frames in one call, this one in the middle of two others (device buffers of the same layout)."""
    return s.e.encode_sequence_device([others.d, s.d, others.d], s.lay, s.p)


# entry point -> the file of Src s (whole-frame calls; `ben` = a benign Src of the same geometry for the sequence's other frames)
ENTRIES = {
    "host": lambda s, ben: s.e.encode_host(s.frame, s.lay, s.p),
    "sink": lambda s, ben: s.e.encode_host(s.frame, s.lay, s.p, via_sink=True),
    "begin_end": lambda s, ben: (s.e.encode_begin_host(s.frame, s.lay, s.p), s.e.encode_end())[1],
    "borrowed": lambda s, ben: (s.e.encode_begin_borrowed(s.frame, s.lay, s.p), s.e.encode_end())[1],
    "device": lambda s, ben: s.e.encode_device(s.d, s.lay, s.p)[2],
    "sequence": lambda s, ben: _sequence(s, ben)[1][2],
}
BANDED = ("host", "sink")  # the calls the band pipeline serves (tune("bands", 3))
# the plain 8- and 16-bit frames, where the test also insists that the band pipeline was what ran
SURELY_BANDED = ("over_8_k2_r2", "over_16_k2_r2", "limit_8_k2_r2", "limit_16_k2_r2")


def _ran_banded(enc, c):
    return enc.stats()["bands"] >= 1 or c.name not in SURELY_BANDED


def _golden_other(api, golden):
    from j2k_amd import synth
    g, pl, _, cs = golden_case(golden, OTHER)
    frame, lay = synth.ae_frame(pl, g["prec"])
    kw = g["params"]
    p = api.make_params(g["width"], g["height"], g["ncomp"], g["prec"], reversible=kw.get("reversible", True), ycc=kw.get("mct", False),
                        num_resolutions=kw.get("numres", 6), comment="")
    return frame, lay, p, cs


def _benign(oracle, c):
    pl = gc.benign_frame(c)
    return pl, gc.oracle_file(oracle, c, pl, key="benign")


# ---------------------------------------------------------------------------------------------------------------------- at the limit
@pytest.mark.parametrize("c", gc.AT_LIMIT, ids=lambda c: c.name)
def test_at_limit_frames_are_byte_exact_through_every_entry_point(api, enc, oracle, c):
    want = gc.oracle_file(oracle, c)
    s = Src(api, enc, c, gc.frame(c))
    try:
        for name, call in ENTRIES.items():
            assert call(s, s) == want, name
        assert [f[2] for f in _sequence(s, s)] == [want] * 3
        before = api.get_tune("bands")
        api.tune("bands", 3)
        try:
            for name in BANDED:
                assert ENTRIES[name](s, s) == want, ("bands", name)
                assert _ran_banded(enc, c)
        finally:
            api.tune("bands", before)
        if c.tile:
            from j2k_amd import sharding
            _, parts = sharding.split_tileparts(want)
            for first, count in ((0, 1), (1, 1), (0, 2)):
                assert enc.encode_tiles_host(s.views(s.frame.ctypes.data), s.p, first, count) == b"".join(parts[first:first + count])
        dec = enc.decode_planar(want)
        assert np.array_equal(dec.astype(np.int32), gc.frame(c)) and np.array_equal(dec.astype(np.int32), oracle.decode(want))
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------------------------- over
def _assert_refused(api, call, what):
    with pytest.raises(api.J2kHipError) as ei:
        call()
    assert ei.value.code == J2K_HIP_ERR_OVERFLOW and GUARD_TEXT in str(ei.value), (what, str(ei.value))


def _assert_handle_whole(api, enc, oracle, golden, c, ben_src, ben_file):
    """After a failed call, on the same handle."""
    assert isinstance(enc.stats(), dict)
    frame, lay, p, cs = _golden_other(api, golden)
    assert enc.encode_host(frame, lay, p) == cs                                # another geometry
    assert ENTRIES["host"](ben_src, ben_src) == ben_file                       # the failed frame's geometry, benign content
    assert ENTRIES["begin_end"](ben_src, ben_src) == ben_file                  # nothing was left pending
    with pytest.raises(api.J2kHipError, match="no encode in progress"):
        enc.encode_end()


@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("c", gc.OVER, ids=lambda c: c.name)
def test_over_frames_are_refused_and_leave_the_handle_whole(api, enc, oracle, golden, c, entry):
    """Every entry point: J2K_HIP_ERR_OVERFLOW with the guard-bits text (the rate-controlled case through TilePricer), then the
    handle's next frames are exact.  The sequence call holds the over-range frame between two benign ones; a whole sequence
    of benign frames follows it."""
    ben_pl, ben_file = _benign(oracle, c)
    s, ben = Src(api, enc, c, gc.frame(c)), Src(api, enc, c, ben_pl)
    try:
        assert ENTRIES["device"](ben, ben) == ben_file  # (the geometry and its tables are cached when the refusal comes)
        _assert_refused(api, lambda: ENTRIES[entry](s, ben), entry)
        _assert_handle_whole(api, enc, oracle, golden, c, ben, ben_file)
        if entry == "sequence":
            assert [f[2] for f in _sequence(ben, ben)] == [ben_file] * 3
        _assert_refused(api, lambda: ENTRIES[entry](s, ben), entry + " again")  # and the refusal repeats
        assert ENTRIES["device"](ben, ben) == ben_file
    finally:
        s.close()
        ben.close()


@pytest.mark.parametrize("entry", BANDED)
@pytest.mark.parametrize("c", [c for c in gc.OVER if not c.rates], ids=lambda c: c.name)
def test_over_frames_are_refused_by_the_band_pipeline(api, enc, oracle, golden, bands3, c, entry):
    """tune("bands", 3): Tier-2 runs on the planner thread while the stages come down; its error is the call's."""
    ben_pl, ben_file = _benign(oracle, c)
    s, ben = Src(api, enc, c, gc.frame(c)), Src(api, enc, c, ben_pl)
    try:
        assert ENTRIES[entry](ben, ben) == ben_file and _ran_banded(enc, c)
        _assert_refused(api, lambda: ENTRIES[entry](s, ben), entry)
        _assert_handle_whole(api, enc, oracle, golden, c, ben, ben_file)
        assert ENTRIES[entry](ben, ben) == ben_file and _ran_banded(enc, c)
        assert [f[2] for f in _sequence(ben, ben)] == [ben_file] * 3  # gate words and in-flight counts are back
    finally:
        s.close()
        ben.close()


def test_tile_ranges_of_the_two_tile_frame(api, enc, oracle, golden):
    """j2k_hip_encode_tiles: the benign tile's range is the oracle's tile-part, the other tile's range and the whole grid raise."""
    from j2k_amd import sharding
    c = gc.BY_NAME["over_tiles_8_k2_r2"]
    _, parts = sharding.split_tileparts(gc.oracle_file(oracle, c))
    ben_pl, ben_file = _benign(oracle, c)
    s, ben = Src(api, enc, c, gc.frame(c)), Src(api, enc, c, ben_pl)
    try:
        host = s.views(s.frame.ctypes.data)
        assert enc.encode_tiles_host(host, s.p, 0, 1) == parts[0]
        _assert_refused(api, lambda: enc.encode_tiles_host(host, s.p, 1, 1), "tile 1")
        assert enc.encode_tiles_host(host, s.p, 0, 1) == parts[0]
        _assert_refused(api, lambda: enc.encode_tiles_host(host, s.p, 0, 2), "both tiles")
        _assert_refused(api, lambda: enc.encode_tiles_device(s.d, s.lay, s.p, 1, 1), "tile 1, device")
        assert enc.encode_tiles_device(s.d, s.lay, s.p, 0, 1) == parts[0]
        _assert_handle_whole(api, enc, oracle, golden, c, ben, ben_file)
    finally:
        s.close()
        ben.close()


# ---------------------------------------------------------------------------------------------------------------------- what a failed call leaves
@pytest.mark.parametrize("bands", [0, 3])
@pytest.mark.parametrize("c", [gc.BY_NAME["over_8_k2_r2"], gc.BY_NAME["over_16_k4_r3"]], ids=lambda c: c.name)
def test_a_refused_frame_writes_nothing(api, enc, c, bands):
    """include/j2k_hip.h, "When an encode fails": not one byte reaches the sink (j2k_hip_encode, _encode_end), no output
    pointer or length is written (the buffer and device entry points) -- plain and band-pipelined."""
    s = Src(api, enc, c, gc.frame(c))
    chunks = []

    @api.WRITE_FN
    def sink(user, buf, n):
        chunks.append(C.string_at(buf, n))
        return n
    before = api.get_tune("bands")
    api.tune("bands", bands)
    try:
        L, h = enc.L, enc.h
        host = s.views(s.frame.ctypes.data)
        assert L.j2k_hip_encode(h, C.byref(s.p), host, sink, None) == J2K_HIP_ERR_OVERFLOW and chunks == []
        assert GUARD_TEXT in L.j2k_hip_last_error(h).decode()
        assert L.j2k_hip_encode_begin(h, C.byref(s.p), host) == 0
        assert L.j2k_hip_encode_end(h, sink, None) == J2K_HIP_ERR_OVERFLOW and chunks == []
        out, n = np.full(1 << 16, 0xA5, np.uint8), C.c_size_t(SENTINEL)
        assert L.j2k_hip_encode_to_buffer(h, C.byref(s.p), host, out.ctypes.data, out.size, C.byref(n)) == J2K_HIP_ERR_OVERFLOW
        assert n.value == SENTINEL and bool((out == 0xA5).all())
        dptr, n = C.c_void_p(SENTINEL), C.c_size_t(SENTINEL)
        assert L.j2k_hip_encode_device(h, C.byref(s.p), s.views(s.d), C.byref(dptr), C.byref(n), out.ctypes.data, out.size) == J2K_HIP_ERR_OVERFLOW
        assert (dptr.value, n.value) == (SENTINEL, SENTINEL) and bool((out == 0xA5).all())
        ptrs, lens = (C.c_void_p * 2)(SENTINEL, SENTINEL), (C.c_size_t * 2)(SENTINEL, SENTINEL)
        two = (api.Plane * (2 * c.nc))(*(list(s.views(s.d)) * 2))
        assert L.j2k_hip_encode_sequence_device(h, C.byref(s.p), two, 2, ptrs, lens) == J2K_HIP_ERR_OVERFLOW
        assert list(ptrs) == [SENTINEL] * 2 and list(lens) == [SENTINEL] * 2
    finally:
        api.tune("bands", before)
        s.close()


# ---------------------------------------------------------------------------------------------------------------------- HipCodec
def test_hip_codec_write_file_refuses_and_goes_on(api, oracle):
    """HipCodec::WriteFile always writes six resolutions: the 33 x 33 case is `over` there.  The plug-in's write-error exception,
    the library's text behind it, no file; the next WriteFile on the thread's handle is exact."""
    from j2k_amd import synth
    from oracle.oracle import strip_com
    c = gc.BY_NAME["over_8_rand7_r6"]
    api.load_library()
    H = C.CDLL(os.path.join(os.path.dirname(api.LIBPATH), "libj2k_host.so"))
    H.j2k_host_test_write.restype = C.c_long
    H.j2k_host_test_write.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_long] + [C.c_int] * 8 + [C.c_long, C.c_void_p, C.c_ulong, C.c_char_p, C.c_ulong]

    def write(planes):
        frame, lay = synth.ae_frame(planes, c.prec)
        out, err = np.full(1 << 16, 0xA5, np.uint8), C.create_string_buffer(512)
        n = H.j2k_host_test_write(frame.ctypes.data, c.w, c.h, lay["rowbytes"], lay["sample_bytes"], c.nc, c.prec, 1, 1, 1, 0, 1, -1,
                                  out.ctypes.data, out.size, err, 512)
        return n, out, err.value.decode()

    ben_pl, ben_file = _benign(oracle, c)
    n, out, _ = write(ben_pl)
    assert n > 0 and strip_com(out[:n].tobytes()) == ben_file
    n, out, err = write(gc.frame(c))
    assert n == -1 and err.startswith("Error writing file | ") and GUARD_TEXT in err and bool((out == 0xA5).all())
    n, out, _ = write(ben_pl)
    assert n > 0 and strip_com(out[:n].tobytes()) == ben_file


# ---------------------------------------------------------------------------------------------------------------------- decode
@pytest.mark.parametrize("lanes", [0, 2])
@pytest.mark.parametrize("c", [c for c in gc.OVER if not c.rates], ids=lambda c: c.name)
def test_decode_of_what_libopenjp2_writes_for_over_frames(api, enc, oracle, c, lanes):
    """The oracle's file of the frame is libopenjp2's (test_guard_bits_refs.py): zero-bit-plane count 0 and three passes more
    than Mb bit-planes hold.  Both Tier-1 decoders read it as the oracle and libopenjp2 do -- the passes beyond the last
    bit-plane dropped -- sample for sample, at full size and reduced by one."""
    data = gc.oracle_file(oracle, c)
    before = api.get_tune("t1dec_lanes")
    api.tune("t1dec_lanes", lanes)
    try:
        for sub in (1, 2):
            want = oracle.decode(data, sub.bit_length() - 1)
            assert np.array_equal(enc.decode_planar(data, subsample=sub).astype(np.int32), want), sub
    finally:
        api.tune("t1dec_lanes", before)
    assert not np.array_equal(oracle.decode(data), gc.frame(c))  # (and it is not the frame)
