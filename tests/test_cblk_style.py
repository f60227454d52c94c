"""GPU: encoding under a code-block style (bypass, reset, termall, pterm, segsym and their combinations) is byte-identical
to libopenjp2 for the same mode, through every entry point, and decodes back.  The fixtures carry everything: files written
by libopenjp2 (tests/golden/styles/, tests/golden/ext/) and the seeds of their inputs."""
import hashlib

import numpy as np
import pytest

import cblk_style_cases as cases
from j2k_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from j2k_amd import api
    return api


@pytest.fixture(scope="module")
def enc(api):
    e = api.Encoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def encoded(api, enc):
    """name -> the host encode of the fixture's input, made once."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = enc.encode_planar_host(cases.planes(name), cases.params(api, name))
        return cache[name]
    return get


@pytest.mark.parametrize("name", cases.NAMES)
def test_styled_encode_is_byte_identical_to_libopenjp2(encoded, name):
    ours, want = encoded(name), cases.golden_bytes(name)
    assert len(ours) == len(want) == cases.entry(name)["length"]
    assert ours == want


@pytest.mark.parametrize("name", cases.NAMES)
def test_styled_encode_decodes_back(enc, encoded, name):
    g = cases.entry(name)
    dec = enc.decode_planar(encoded(name))
    if g["ext"].get("reversible", True):
        assert np.array_equal(dec, cases.planes(name))
    got = [hashlib.sha256(np.ascontiguousarray(dec[c], dtype=np.int32).tobytes()).hexdigest() for c in range(g["ncomp"])]
    assert got == cases.decoded_hashes(name)  # what libopenjp2 decodes from its own file


@pytest.mark.parametrize("name", cases.ENTRY_POINT_NAMES)
def test_every_entry_point_writes_the_same_bytes(api, enc, name):
    g = cases.entry(name)
    want = cases.golden_bytes(name)
    p = cases.params(api, name)
    frame, lay = synth.ae_frame(cases.planes(name), g["prec"], row_pad_bytes=8)
    frame2, _ = synth.ae_frame(cases.planes(name, seed_offset=1000), g["prec"], row_pad_bytes=8)
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
        if name == cases.TILED_NAME:
            ntiles = -(-g["width"] // 64) * -(-g["height"] // 64)
            parts = [enc.encode_tiles_device(d, lay, p, a, b) for (a, b) in [(0, 2), (2, ntiles - 2)]]
            assert api.main_header(p) + b"".join(parts) + b"\xff\xd9" == want
    finally:
        enc.free(d)
        enc.free(d2)


def test_styled_host_call_is_not_band_pipelined(api, enc):
    name = "ya_200x150_rgb16_97_all_five_cblk32"
    g = cases.entry(name)
    frame, lay = synth.ae_frame(cases.planes(name), g["prec"])
    api.tune("bands", 3)  # (small frames are banded only on request: a style-0 call would now be)
    try:
        enc.encode_host(frame, lay, cases.params(api, name, cblk_style=0))
        assert enc.stats()["bands"] >= 1
        assert enc.encode_host(frame, lay, cases.params(api, name)) == cases.golden_bytes(name)
        assert enc.stats()["bands"] == 0
    finally:
        api.tune("bands", 0)


def test_style_zero_is_untouched_by_a_styled_frame_in_between(api, enc):
    name = "y7_128_grey16_53_bypass_termall"
    pl = cases.planes(name)
    plain, styled = cases.params(api, name, cblk_style=0), cases.params(api, name)
    first = enc.encode_planar_host(pl, plain)
    assert enc.encode_planar_host(pl, styled) == cases.golden_bytes(name)
    assert enc.encode_planar_host(pl, plain) == first
    assert first != cases.golden_bytes(name)
