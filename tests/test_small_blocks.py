"""GPU: the whole encoder and decoder with code-blocks down to 4 x 4 and precincts down to 2 x 2 (1 x 1 code-blocks).

The cases are those of tests/small_block_cases.py; tests/test_small_block_refs.py shows on the CPU that their references agree
(the oracle's encoder, libopenjp2's decoder of its bytes).  Here: every encode is byte-identical to the oracle through the
host entry points (a sample of six through every entry point) and to libopenjp2's own PCRL / CPRL files; the paths that big
frames take -- coder groups, the rate control's device side, the band pipeline's split last band, handles in flight -- run on a
300 x 200 frame of more than 8192 blocks; every decode of the oracle's bytes equals the oracle's at every sub-sampling under
both Tier-1 kernels; windows swept across block, precinct and tile boundaries equal the crop of the whole decode; and what the
GPU wrote, the GPU reads back."""
import threading

import numpy as np
import pytest

import small_block_cases as cases
from j2k_amd import synth

pytestmark = pytest.mark.gpu

ALL = cases.CASES + [cases.REGION_EXTRA]


@pytest.fixture(scope="module")
def api():
    from j2k_amd import api
    return api


@pytest.fixture(scope="module")
def enc(api):
    e = api.Encoder(0)
    yield e
    e.close()


def _encode(api, e, c, via_sink=False, **override):
    """After Effects frame for 3- and 4-channel cases, planar buffers for grey."""
    p = cases.api_params(api, c, **override)
    if c.nc >= 3:
        frame, lay = synth.ae_frame(cases.planes(c), c.prec)
        return e.encode_host(frame, lay, p, via_sink=via_sink)
    return e.encode_planar_host(cases.planes(c), p, via_sink=via_sink)


_ENCODED = {}


def _encoded(api, e, c):
    """The host encode of a case, made once."""
    if c.name not in _ENCODED:
        _ENCODED[c.name] = _encode(api, e, c)
    return _ENCODED[c.name]


_DECODED = {}


def _expected(oracle, c, sub):
    """(channels, h, w) int32: the oracle's decode of the oracle's file at this sub-sampling, once, never changed."""
    key = (c.name, sub)
    if key not in _DECODED:
        exp = oracle.decode(cases.oracle_file(oracle, c), sub.bit_length() - 1)
        exp.setflags(write=False)
        _DECODED[key] = exp
    return _DECODED[key]


# -- encode parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ALL, ids=lambda c: c.name)
def test_encode_is_byte_identical_to_the_oracle(api, enc, oracle, c):
    want = cases.oracle_file(oracle, c)
    ours = _encoded(api, enc, c)
    assert len(ours) == len(want) and ours == want
    assert _encode(api, enc, c, via_sink=True) == want


@pytest.mark.parametrize("name", cases.EXT_NAMES)
def test_pcrl_and_cprl_encodes_are_byte_identical_to_libopenjp2(api, enc, name):
    want = cases.ext_bytes(name)
    p = cases.ext_api_params(api, name)
    frame, lay = synth.ae_frame(cases.ext_planes(name), 8)
    assert enc.encode_host(frame, lay, p) == want
    assert enc.encode_host(frame, lay, p, via_sink=True) == want
    assert np.array_equal(enc.decode_planar(want), cases.ext_planes(name))


@pytest.mark.parametrize("name", cases.ENTRY_POINT_NAMES)
def test_every_entry_point_writes_the_same_bytes(api, enc, oracle, name):
    c = cases.BY_NAME[name]
    want = cases.oracle_file(oracle, c)
    p = cases.api_params(api, c)
    frame, lay = synth.ae_frame(cases.planes(c), c.prec, row_pad_bytes=8)
    frame2, _ = synth.ae_frame(cases.planes(c, seed_offset=1000), c.prec, row_pad_bytes=8)
    assert enc.encode_host(frame, lay, p) == want
    assert enc.encode_host(frame, lay, p, via_sink=True) == want
    enc.encode_begin_host(frame, lay, p)
    assert enc.encode_end() == want
    enc.encode_begin_borrowed(frame, lay, p)
    assert enc.encode_end() == want
    d, d2 = enc.upload(frame), enc.upload(frame2)
    try:
        assert enc.encode_device(d, lay, p)[2] == want
        other = enc.encode_device(d2, lay, p)[2]
        assert other != want
        seq = enc.encode_sequence_device([d, d2], lay, p)
        assert [s[2] for s in seq] == [want, other]
    finally:
        enc.free(d)
        enc.free(d2)


# -- the big frames' paths on a frame that encodes in milliseconds ---------------------------------------------------------------
def test_many_block_frames_take_the_big_frame_paths(api, enc, oracle):
    for c in cases.MANY:
        assert _encode(api, enc, c) == cases.oracle_file(oracle, c)
        assert enc.stats()["num_codeblocks"] >= 8192, c.name  # (the table's blocks, empty ones included: what the paths are gated by)


@pytest.mark.parametrize("groups", [2, 3, 4, 5, 6, 7])
def test_coder_groups_on_many_small_blocks(api, enc, oracle, groups):
    before = api.get_tune("groups")
    api.tune("groups", groups)
    try:
        for c in cases.MANY:
            assert _encode(api, enc, c) == cases.oracle_file(oracle, c), (c.name, groups)
    finally:
        api.tune("groups", before)


@pytest.mark.parametrize("scan", [0, 1, 40])
def test_rate_control_on_the_device_at_its_natural_threshold(api, enc, oracle, scan):
    """rate_dev stays 0: more than 8192 blocks put the allocation's per-block work on the device by themselves."""
    assert api.get_tune("rate_dev") == 0
    before = api.get_tune("rate_dev_scan")
    api.tune("rate_dev_scan", scan)
    try:
        for c in cases.MANY:
            if c.rates:
                assert _encode(api, enc, c) == cases.oracle_file(oracle, c), (c.name, scan)
                assert _encode(api, enc, c, via_sink=True) == cases.oracle_file(oracle, c), (c.name, scan, "sink")
    finally:
        api.tune("rate_dev_scan", before)


@pytest.mark.parametrize("bands", [3, 5])
def test_band_pipeline_splits_the_last_band_of_many_small_blocks(api, enc, oracle, bands):
    before = api.get_tune("bands")
    api.tune("bands", bands)
    try:
        for c in cases.MANY:
            if c.rates:  # (a byte budget is not band-pipelined)
                continue
            for via_sink in (False, True):
                assert _encode(api, enc, c, via_sink=via_sink) == cases.oracle_file(oracle, c), (c.name, bands, via_sink)
                assert 1 <= enc.stats()["bands"] <= bands
    finally:
        api.tune("bands", before)


def test_three_handles_in_flight_on_many_small_blocks(api, oracle):
    """One host thread per handle, all three on the same many-block frame at the same time (a barrier lines them up before
    every frame), frame after frame: their GPU phases overlap, every file stays exact."""
    jobs = []
    for c in cases.MANY:
        frame, lay = synth.ae_frame(cases.planes(c), c.prec)
        jobs.append((c.name, frame, lay, cases.api_params(api, c), cases.oracle_file(oracle, c)))
    errors = []
    line_up = threading.Barrier(3, timeout=60)

    def work(k):
        e = api.Encoder(0)
        try:
            for name, frame, lay, p, want in jobs:
                line_up.wait()
                for it in range(3):
                    if e.encode_host(frame, lay, p, via_sink=bool((it + k) & 1)) != want:
                        errors.append((k, it, name))
        except Exception as ex:  # (a thread's exception must fail the test, not vanish)
            errors.append((k, repr(ex)))
            line_up.abort()
        finally:
            e.close()

    ths = [threading.Thread(target=work, args=(k,)) for k in range(3)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errors


# -- decode parity, from the oracle's bytes --------------------------------------------------------------------------------------
KERNELS = [("wave-per-block", 0, 1), ("lane-per-block-no-tail", 2, 0), ("lane-per-block-tail-half", 2, 2)]


@pytest.mark.parametrize("label,lanes,tail", KERNELS, ids=[k[0] for k in KERNELS])
@pytest.mark.parametrize("kind", cases.KINDS)
def test_decode_equals_the_oracle_under_both_tier1_kernels(api, enc, oracle, kind, label, lanes, tail):
    lanes_before, tail_before = api.get_tune("t1dec_lanes"), api.get_tune("t1dec_tail")
    api.tune("t1dec_lanes", lanes)
    api.tune("t1dec_tail", tail)
    try:
        for c in (c for c in ALL if c.kind == kind or (kind == "size" and c.kind == "region")):
            data = cases.oracle_file(oracle, c)
            for sub in (1, 2, 4):
                if sub > cases.max_subsample(c):
                    continue
                dec = enc.decode_planar(data, subsample=sub)
                assert np.array_equal(dec.astype(np.int32), _expected(oracle, c, sub)), (c.name, sub, label)
                nb = enc.stats()["num_codeblocks"]
                lane_blocks, wave_blocks = enc.decode_kernels()
                assert lane_blocks + wave_blocks == nb > 0, (c.name, sub)
                if c.style:  # (code-block styles are the lane kernel's alone)
                    assert wave_blocks == 0
                elif lanes == 0:
                    assert lane_blocks == 0
                elif tail == 0:
                    assert wave_blocks == 0
                elif nb >= 2:
                    assert lane_blocks > 0 and wave_blocks > 0, (c.name, sub)
            if c.rev and not c.rates:
                assert np.array_equal(enc.decode_planar(data), cases.planes(c)), c.name
    finally:
        api.tune("t1dec_lanes", lanes_before)
        api.tune("t1dec_tail", tail_before)


def test_decode_by_the_cost_estimates_equals_the_oracle(api, enc, oracle):
    """The knobs at their defaults: the decode picks its kernels by the file.  The many-block files and the densest precincts."""
    assert (api.get_tune("t1dec_lanes"), api.get_tune("t1dec_tail")) == (1, 1)
    for c in cases.MANY + [cases.BY_NAME["prec_p2_4x4_rgb8_53"], cases.BY_NAME["prec_p2_64x64_rgb8_53_tile40"]]:
        for sub in (1, 2):
            dec = enc.decode_planar(cases.oracle_file(oracle, c), subsample=sub)
            assert np.array_equal(dec.astype(np.int32), _expected(oracle, c, sub)), (c.name, sub)


# -- region decode ---------------------------------------------------------------------------------------------------------------
# rows and columns of the sweeps, at full size: beside a block boundary of the top resolution, beside a precinct / tile
# boundary, and the image's last
REGION_LINES = {
    "size_4x4_grey12_97": dict(rows=(7, 8, 38), cols=(15, 16, 52)),            # 53 x 39: 4 x 4 blocks of the top bands meet at every 8th sample
    "prec_p8_4x4_rgb8_53": dict(rows=(7, 8, 44), cols=(31, 32, 66)),           # 67 x 45: 8 x 8 precincts of the top resolution
    "region_8x4_rgb8_53_tile40": dict(rows=(39, 40, 60), cols=(39, 40, 89)),   # 90 x 61: tiles of 40
}
REGION_SWEEPS = [(n, sub, win, axis) for n in cases.REGION_NAMES for sub in (1, 2) for win in ((1, 1), (5, 3)) for axis in ("rows", "cols")]


@pytest.mark.parametrize("name,sub,win,axis", REGION_SWEEPS, ids=[f"{n}-sub{s}-{w[0]}x{w[1]}-{a}" for n, s, w, a in REGION_SWEEPS])
def test_windows_swept_across_block_and_tile_boundaries(enc, oracle, name, sub, win, axis):
    c = cases.BY_NAME[name]
    data = cases.oracle_file(oracle, c)
    exp = _expected(oracle, c, sub)
    _, h, w = exp.shape
    assert np.array_equal(enc.decode_planar(data, subsample=sub).astype(np.int32), exp)
    ww, wh = win
    lines = sorted({v // sub for v in REGION_LINES[name][axis]})
    assert len(lines) == 3
    if axis == "rows":  # every x along three rows
        windows = [(x, min(y, h - wh), ww, wh) for y in lines for x in range(w - ww + 1)]
    else:               # every y along three columns
        windows = [(min(x, w - ww), y, ww, wh) for x in lines for y in range(h - wh + 1)]
    assert 3 * 15 <= len(windows) <= 400
    for (x, y, _, _) in windows:
        got = enc.decode_region_planar(data, (x, y, ww, wh), subsample=sub)
        assert np.array_equal(got.astype(np.int32), exp[:, y:y + wh, x:x + ww]), (name, sub, (x, y, ww, wh))


# -- round trip ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [k for k in cases.KINDS if k != "rates"])
def test_gpu_decode_of_the_gpu_encode_returns_the_frame(api, enc, kind):
    n = 0
    for c in ALL:
        if (c.kind == kind or (kind == "size" and c.kind == "region")) and c.rev and not c.rates:
            assert np.array_equal(enc.decode_planar(_encoded(api, enc, c)), cases.planes(c)), c.name
            n += 1
    assert n >= 1
