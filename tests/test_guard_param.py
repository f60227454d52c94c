"""GPU: guard bits by parameter, or as many as the frame needs (j2k_hip_params.guard_bits; DESIGN.md section 8;
tests/test_guard_param_host.py holds the host side on the CPU).

The frames are those of tests/guard_cases.py, the entry points those of tests/test_guard_bits.py.  An `over` frame -- refused
at two guard bits, written wrongly by libopenjp2 -- is written under J2K_HIP_GUARD_AUTO and under a fixed count of three as one
and the same file through every entry point, with 3 in its QCD, and libopenjp2 2.4.0 and 2.5.4, the oracle and this library
all decode it back to the frame.  A frame in range moves by no byte and no statistic.  A fixed count on a frame in range changes
the QCD and the zero-bit-plane counts and nothing of a block.  Rate control, tiles, sequences and HipCodec follow."""
import ctypes as C
import os

import numpy as np
import pytest

import guard_cases as gc
import test_guard_bits as tgb
from test_guard_bits import BANDED, ENTRIES, GUARD_TEXT, SENTINEL, Src

pytestmark = pytest.mark.gpu

J2K_HIP_ERR_PARAM, J2K_HIP_ERR_OVERFLOW = 1, 4
OVER_PLAIN = [c for c in gc.OVER if not c.rates]
AUTO_GUARD_BITS = 32  # HipCodec::AutoGuardBits


@pytest.fixture(scope="module")
def api():
    from j2k_amd import api
    return api


@pytest.fixture
def enc(api):
    e = api.Encoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def opjs():
    """libopenjp2 2.4.0 and 2.5.4, both."""
    from oracle.oracle import OpjReplay, find_openjpeg_libs
    reps = [OpjReplay(p) for p in find_openjpeg_libs()]
    assert {r.version for r in reps} >= {"2.4.0", "2.5.4"}, [r.version for r in reps]
    return reps


@pytest.fixture
def knobs(api):
    before = {}

    def tune(key, value):
        before.setdefault(key, api.get_tune(key))
        api.tune(key, value)
    yield tune
    for k, v in before.items():
        api.tune(k, v)


def _codestream(data: bytes) -> bytes:
    return data[data.index(b"jp2c") + 4:] if data[:12] == b"\x00\x00\x00\x0cjP  \r\n\x87\n" else data


def _guard_of(data: bytes) -> int:
    """Guard bits in the file's QCD."""
    cs = _codestream(data)
    q = 2
    while cs[q:q + 2] != b"\xff\x5c":
        assert cs[q] == 0xff and cs[q:q + 2] != b"\xff\x90"
        q += 2 + int.from_bytes(cs[q + 2:q + 4], "big")
    return cs[q + 4] >> 5


def _opj_decode(opj, data: bytes, reduce: int = 0) -> np.ndarray:
    return np.stack([k["data"] for k in opj.decode_comps(data, reduce=reduce)]).astype(np.int32)


def _ours(enc, data: bytes, sub: int = 1) -> np.ndarray:
    return enc.decode_planar(data, subsample=sub).astype(np.int32)


def _set(g, *srcs):
    for s in srcs:
        s.p.guard_bits = g


def _file_rows(oracle, data):
    """(tile, comp, res, orient, x, y, w, h) -> (numbps, passes, codeword) of every block of the file that holds passes."""
    return {(f["tile"], f["comp"], f["res"], f["orient"]) + f["rect"]: (f["numbps"], f["npasses"], f["data"]) for f in oracle.file_blocks(data)["blocks"]}


# ---------------------------------------------------------------------------------------------------------------------- 1. over frames
@pytest.mark.parametrize("c", OVER_PLAIN, ids=lambda c: c.name)
def test_over_frames_are_written_and_are_lossless(api, enc, oracle, opjs, knobs, c):
    src = gc.frame(c)
    ben_pl, _ = tgb._benign(oracle, c)
    s, ben = Src(api, enc, c, src), Src(api, enc, c, ben_pl)
    try:
        files = {}
        bands_before = api.get_tune("bands")
        for g in (api.GUARD_AUTO, 3):
            _set(g, s, ben)
            for name, call in ENTRIES.items():
                files[(g, name)] = call(s, ben)
                # (the sequence call's last frame is the benign one: two guard bits unless three were asked for)
                assert enc.guard_bits() == (2 if name == "sequence" and g != 3 else 3), (g, name)
            knobs("bands", 3)
            for name in BANDED:
                files[(g, "bands", name)] = ENTRIES[name](s, ben)
                assert tgb._ran_banded(enc, c) and enc.guard_bits() == 3, (g, name)
            knobs("bands", bands_before)
        f = files[(api.GUARD_AUTO, "host")]
        assert [k for k, v in files.items() if v != f] == []
        assert _guard_of(f) == 3
        # the decoders: the frame, exactly -- where libopenjp2's own file of the frame is off by the table's error
        wrong = gc.oracle_file(oracle, c)
        for opj in opjs:
            assert np.array_equal(_opj_decode(opj, f), src), opj.version
            assert int(np.abs(_opj_decode(opj, wrong).astype(np.int64) - src).max()) == c.max_err, opj.version
        assert np.array_equal(oracle.decode(f), src)
        for lanes in (0, 2):
            knobs("t1dec_lanes", lanes)
            assert np.array_equal(_ours(enc, f), src), lanes
        assert [d["differing"] for d in enc.compare(f, s.p, frame=s.frame, layout=s.lay)] == [0] * c.nc
        # the blocks of the file are the classifier's, bit-plane for bit-plane
        rows = {(b["tile"], b["comp"], b["res"], b["orient"], b["tx"], b["ty"], b["w"], b["h"]): b for b in gc.classify(oracle, c)}
        fb = _file_rows(oracle, f)
        assert len(fb) == len([b for b in rows.values() if b["numbps"]])
        over = 0
        for key, (numbps, _, _) in fb.items():
            assert numbps == rows[key]["numbps"] <= rows[key]["Mb"] + 1
            over += numbps == rows[key]["Mb"] + 1
        assert over >= 1
    finally:
        s.close()
        ben.close()


# ---------------------------------------------------------------------------------------------------------------------- 2. in range
def _in_range_frames():
    return [(c.name, c, False) for c in gc.AT_LIMIT] + [("benign_" + c.name, c, True) for c in gc.CASES]


@pytest.mark.parametrize("name,c,benign", _in_range_frames(), ids=[n for n, _, _ in _in_range_frames()])
def test_nothing_moves_in_range(api, enc, oracle, knobs, name, c, benign):
    """0, 2 and auto: the oracle's bytes through every entry point, and stats().bands what it is without the field."""
    pl = gc.benign_frame(c) if benign else gc.frame(c)
    want = gc.oracle_file(oracle, c, pl, key="benign") if benign else gc.oracle_file(oracle, c)
    s = Src(api, enc, c, pl)
    try:
        bands = {}
        bands_before = api.get_tune("bands")
        for g in (0, 2, api.GUARD_AUTO, api.GUARD_AUTO | 2):
            _set(g, s)
            for bd in (bands_before, 3):
                knobs("bands", bd)
                for entry in (ENTRIES if bd == bands_before else BANDED):
                    assert ENTRIES[entry](s, s) == want, (g, bd, entry)
                    assert enc.guard_bits() == 2
                    assert bands.setdefault((bd, entry), enc.stats()["bands"]) == enc.stats()["bands"], (g, bd, entry)
            assert [f[2] for f in tgb._sequence(s, s)] == [want] * 3
        assert bands[(bands_before, "device")] == 0 and bands_before != 3
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------------------------- 3. a fixed count in range
def _fixed_count_frames(oracle):
    from j2k_amd import synth
    from oracle.oracle import make_params
    c = gc.BY_NAME["limit_8_k2_r3"]
    yield "limit_8_k2_r3", gc.frame(c), dict(reversible=True, ycc=True, num_resolutions=c.numres), gc.oracle_file(oracle, c), c.prec
    pl = synth.planes(97, 61, 3, 8, 4711)
    yield "97_ict_97x61_r3", pl, dict(reversible=False, ycc=True, num_resolutions=3), \
        oracle.encode(pl, make_params(97, 61, 3, 8, reversible=False, mct=True, numres=3)), 8


def test_a_fixed_count_on_a_frame_in_range(api, enc, oracle, opjs):
    """g = 3, 5, 7: QCD and the zero-bit-plane counts move; every block keeps its bit-planes, passes and codeword bytes, and
    every decoder returns the samples it returns from the two-guard-bit file, at full size and reduced by one."""
    from j2k_amd import synth
    for name, pl, kw, ref, prec in _fixed_count_frames(oracle):
        nc, h, w = pl.shape
        frame, lay = synth.ae_frame(pl, prec)
        assert enc.encode_host(frame, lay, api.make_params(w, h, nc, prec, **kw)) == ref
        ref_rows = _file_rows(oracle, ref)
        for g in (3, 5, 7):
            p = api.make_params(w, h, nc, prec, guard_bits=g, **kw)
            f = enc.encode_host(frame, lay, p)
            assert enc.guard_bits() == g == _guard_of(f) and f != ref, (name, g)
            d = enc.upload(frame)
            try:
                assert enc.encode_device(d, lay, p)[2] == f
            finally:
                enc.free(d)
            assert _file_rows(oracle, f) == ref_rows, (name, g)
            for red in (0, 1):
                for opj in opjs:
                    assert np.array_equal(_opj_decode(opj, f, red), _opj_decode(opj, ref, red)), (name, g, red, opj.version)
                assert np.array_equal(oracle.decode(f, red), oracle.decode(ref, red)), (name, g, red)
                assert np.array_equal(_ours(enc, f, 1 << red), _ours(enc, ref, 1 << red)), (name, g, red)
            if kw["reversible"]:
                assert np.array_equal(_ours(enc, f), pl)


@pytest.mark.parametrize("c", gc.AT_LIMIT, ids=lambda c: c.name)
def test_one_guard_bit_refuses_an_at_limit_frame(api, enc, oracle, c):
    """Strictly: J2K_HIP_ERR_OVERFLOW with the text it always had, nothing written, and the handle's next frame is exact."""
    s = Src(api, enc, c, gc.frame(c))
    try:
        _set(1, s)
        for entry in ENTRIES:
            tgb._assert_refused(api, lambda: ENTRIES[entry](s, s), entry)
        out, n = np.full(1 << 16, 0xA5, np.uint8), C.c_size_t(SENTINEL)
        host = s.views(s.frame.ctypes.data)
        assert enc.L.j2k_hip_encode_to_buffer(enc.h, C.byref(s.p), host, out.ctypes.data, out.size, C.byref(n)) == J2K_HIP_ERR_OVERFLOW
        assert n.value == SENTINEL and bool((out == 0xA5).all()) and GUARD_TEXT in enc.L.j2k_hip_last_error(enc.h).decode()
        _set(0, s)
        assert ENTRIES["host"](s, s) == gc.oracle_file(oracle, c) and enc.guard_bits() == 2
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------------------------- 4. rate control
def test_rate_control_at_auto(api, enc, oracle, opjs, knobs):
    c = gc.BY_NAME["over_rates_8_k2_r2"]
    s = Src(api, enc, c, gc.frame(c))
    try:
        files = {}
        for dev in (-1, 1):  # rate.hip's per-block work off, and on whatever the frame's size
            knobs("rate_dev", dev)
            for g in (api.GUARD_AUTO, 3):
                _set(g, s)
                files[(dev, g, "host")] = ENTRIES["host"](s, s)
                assert enc.guard_bits() == 3
                files[(dev, g, "device")] = ENTRIES["device"](s, s)
                assert enc.guard_bits() == 3
        f = files[(-1, api.GUARD_AUTO, "host")]
        assert [k for k, v in files.items() if v != f] == []
        assert _guard_of(f) == 3
        # libopenjp2's rule: layer 0 within raw tile bytes / ratio, SOT, SOD and EOC (16 bytes) left out
        assert len(f) <= c.w * c.h * c.nc / c.rates[0] + 16
        want = oracle.decode(f)
        for opj in opjs:
            assert np.array_equal(_opj_decode(opj, f), want), opj.version
        assert np.array_equal(_ours(enc, f), want)
        _set(0, s)
        tgb._assert_refused(api, lambda: ENTRIES["host"](s, s), "strict")
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------------------------- 5. tiles
def test_tiles_one_of_two_exceeds(api, enc, oracle, opjs):
    from j2k_amd import sharding
    c = gc.BY_NAME["over_tiles_8_k2_r2"]
    src = gc.frame(c)
    s = Src(api, enc, c, src)
    try:
        _set(api.GUARD_AUTO, s)
        f = ENTRIES["host"](s, s)
        assert _guard_of(f) == 3 == enc.guard_bits() and ENTRIES["device"](s, s) == f
        for opj in opjs:
            assert np.array_equal(_opj_decode(opj, f), src)
        assert np.array_equal(oracle.decode(f), src) and np.array_equal(_ours(enc, f), src)
        # the tile-range entry points with three guard bits: the same file, put together as a tile-sharded job does
        _set(3, s)
        host = s.views(s.frame.ctypes.data)
        header, parts = sharding.split_tileparts(f)
        assert api.main_header(s.p) == header
        for first, count in ((0, 1), (1, 1), (0, 2)):
            assert enc.encode_tiles_host(host, s.p, first, count) == b"".join(parts[first:first + count]), (first, count)
            assert enc.encode_tiles_device(s.d, s.lay, s.p, first, count) == b"".join(parts[first:first + count]), (first, count)
        assert sharding.assemble(s.p, [enc.encode_tiles_host(host, s.p, 0, 1), enc.encode_tiles_device(s.d, s.lay, s.p, 1, 1)]) == f
        # ... and with auto they have no frame to decide by
        for g in (api.GUARD_AUTO, api.GUARD_AUTO | 3):
            _set(g, s)
            for call in (lambda: enc.encode_tiles_host(host, s.p, 0, 1), lambda: enc.encode_tiles_host(host, s.p, 0, 2),
                         lambda: enc.encode_tiles_device(s.d, s.lay, s.p, 1, 1)):
                with pytest.raises(api.J2kHipError) as ei:
                    call()
                assert ei.value.code == J2K_HIP_ERR_PARAM and "guard_bits" in str(ei.value)
            chunks = []

            @api.WRITE_FN
            def sink(user, buf, n):
                chunks.append(n)
                return n
            dev = (C.c_int * 1)(0)
            assert enc.L.j2k_hip_encode_tiles_distributed(dev, 1, C.byref(s.p), host, sink, None) == J2K_HIP_ERR_PARAM and chunks == []
            assert b"guard_bits" in enc.L.j2k_hip_multi_last_error()
        _set(3, s)
        assert enc.encode_tiles_host(host, s.p, 1, 1) == parts[1]  # (the handle is whole)
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------------------------- 6. sequence
@pytest.mark.parametrize("c", [gc.BY_NAME["over_8_k2_r2"], gc.BY_NAME["over_16_k4_r3"]], ids=lambda c: c.name)
def test_sequence_gives_every_frame_its_own_count(api, enc, oracle, c):
    ben_pl, ben_file = tgb._benign(oracle, c)
    s, ben = Src(api, enc, c, gc.frame(c)), Src(api, enc, c, ben_pl)
    try:
        _set(api.GUARD_AUTO, s, ben)
        single = [ENTRIES["device"](x, x) for x in (ben, s, ben)]
        assert single[0] == ben_file
        got = [f[2] for f in tgb._sequence(s, ben)]
        assert [_guard_of(f) for f in got] == [2, 3, 2] and enc.guard_bits() == 2
        assert got == single
        got = [f[2] for f in enc.encode_sequence_device([ben.d, ben.d, s.d], s.lay, s.p)]
        assert got == [single[0], single[0], single[1]] and enc.guard_bits() == 3
    finally:
        s.close()
        ben.close()


# ---------------------------------------------------------------------------------------------------------------------- big frames
def test_a_frame_of_4096_blocks_and_more_is_planned_again_by_the_worker_threads(api, enc, oracle, opjs, knobs):
    """From 4096 code-blocks on, Tier-2 writes the packets of the (resolution, component) pairs on worker threads, and the
    band pipeline's planner waits there for its stages: the excess is thrown on a worker while others still wait.  1536 x 1024,
    32 x 32 code-blocks, two resolutions: 4608 blocks, every LL block of the chroma components one bit-plane over."""
    from j2k_amd import synth
    w, h, prec = 1536, 1024, 8
    y, x = np.arange(h)[:, None] // 2, np.arange(w)[None, :] // 2
    g = (((x + y) & 1) * 255).astype(np.int32)
    src = np.stack([255 - g, g, 255 - g]).astype(np.int32)
    frame, lay = synth.ae_frame(src, prec)
    kw = dict(reversible=True, ycc=True, num_resolutions=2, cblk=(32, 32))
    assert len(api.frame_blocks(api.make_params(w, h, 3, prec, **kw))) == 4608
    d = enc.upload(frame)
    try:
        with pytest.raises(api.J2kHipError) as ei:
            enc.encode_device(d, lay, api.make_params(w, h, 3, prec, **kw))
        assert ei.value.code == J2K_HIP_ERR_OVERFLOW and GUARD_TEXT in str(ei.value)
        f = enc.encode_device(d, lay, api.make_params(w, h, 3, prec, guard_bits=3, **kw))[2]
        assert _guard_of(f) == 3 == enc.guard_bits()
        pa = api.make_params(w, h, 3, prec, guard_bits=api.GUARD_AUTO, **kw)
        assert enc.encode_device(d, lay, pa)[2] == f and enc.guard_bits() == 3
        knobs("bands", 4)
        for via_sink in (False, True):
            assert enc.encode_host(frame, lay, pa, via_sink=via_sink) == f
            assert enc.stats()["bands"] == 4 and enc.guard_bits() == 3
        with pytest.raises(api.J2kHipError) as ei:  # (strictly: the planner's error is the call's, and the handle goes on)
            enc.encode_host(frame, lay, api.make_params(w, h, 3, prec, **kw))
        assert ei.value.code == J2K_HIP_ERR_OVERFLOW and GUARD_TEXT in str(ei.value)
        assert enc.encode_host(frame, lay, pa) == f
    finally:
        enc.free(d)
    assert np.array_equal(_ours(enc, f), src) and np.array_equal(oracle.decode(f), src)
    for opj in opjs:
        assert np.array_equal(_opj_decode(opj, f), src), opj.version


# ---------------------------------------------------------------------------------------------------------------------- 7. HipCodec
def test_hip_codec_auto_guard_bits(api, enc, oracle):
    """HipCodec::WriteFile always writes six resolutions: the 33 x 33 case is `over` there.  With AutoGuardBits the file is
    written -- three guard bits -- and HipCodec::ReadFile returns the frame; a frame in range is written as without the option."""
    from j2k_amd import synth
    from oracle.oracle import strip_com
    c = gc.BY_NAME["over_8_rand7_r6"]
    api.load_library()
    H = C.CDLL(os.path.join(os.path.dirname(api.LIBPATH), "libj2k_host.so"))
    H.j2k_host_test_write_options.restype = C.c_long
    H.j2k_host_test_write_options.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_long] + [C.c_int] * 8 + [C.c_uint, C.c_void_p, C.c_ulong, C.c_char_p, C.c_ulong]
    H.j2k_host_test_read.restype = C.c_long
    H.j2k_host_test_read.argtypes = [C.c_void_p, C.c_ulong, C.c_uint, C.c_void_p, C.c_uint, C.c_uint, C.c_long, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_ulong]

    def write(planes, options, honour=1):
        frame, lay = synth.ae_frame(planes, c.prec)
        out, err = np.full(1 << 16, 0xA5, np.uint8), C.create_string_buffer(512)
        n = H.j2k_host_test_write_options(frame.ctypes.data, c.w, c.h, lay["rowbytes"], lay["sample_bytes"], c.nc, c.prec, 1, 1, 1, 0, honour,
                                          options, out.ctypes.data, out.size, err, 512)
        return n, out, err.value.decode(), frame, lay

    ben_pl, ben_file = tgb._benign(oracle, c)
    n, out, _, _, _ = write(ben_pl, AUTO_GUARD_BITS)
    assert n > 0 and strip_com(out[:n].tobytes()) == ben_file
    n, out, err, frame, lay = write(gc.frame(c), AUTO_GUARD_BITS)
    assert n > 0, err
    f = out[:n].tobytes()
    assert _guard_of(f) == 3 and np.array_equal(oracle.decode(strip_com(f)), gc.frame(c))
    back, err = np.zeros_like(frame), C.create_string_buffer(512)
    back[lay["channel_offsets"][0]::4] = 0xff  # (three channels: alpha is not the file's to write)
    assert H.j2k_host_test_read(np.frombuffer(f, np.uint8).ctypes.data, len(f), 1, back.ctypes.data, c.w, c.h, lay["rowbytes"], 1, c.nc, 8, err, 512) == 0, err.value
    assert np.array_equal(back, frame)
    # ReferenceLiteral takes the option too: a frame in range is written as without it
    n0, out0, _, _, _ = write(ben_pl, 0, honour=0)
    n1, out1, _, _, _ = write(ben_pl, AUTO_GUARD_BITS, honour=0)
    assert n0 == n1 > 0 and bytes(out0[:n0]) == bytes(out1[:n1]) and _guard_of(bytes(out1[:n1])) == 2
    # and without the option the frame is refused as ever (tests/test_guard_bits.py says how the handle goes on)
    n, out, err, _, _ = write(gc.frame(c), 0)
    assert n == -1 and GUARD_TEXT in err
