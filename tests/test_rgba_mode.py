"""CPU: j2k_hip_rgba_mode -- how a file's components become R, G, B, A, from the header alone -- and the committed hashes of
the whole-file RGBA cases against a live libopenjp2."""
import json
import os

import pytest

import rgba_cases as rc
from conftest import GOLDEN_DIR
from j2k_amd import api

J2K_HIP_ERR_UNSUPPORTED = 6


@pytest.mark.parametrize("name", sorted(rc.MODES))
def test_every_file_gets_its_mode(name):
    data = rc.load(name)
    if rc.MODES[name] is None:
        with pytest.raises(api.J2kHipError) as ei:
            api.rgba_mode(data)
        assert ei.value.code == J2K_HIP_ERR_UNSUPPORTED
    else:
        assert api.rgba_mode(data) == rc.MODES[name]


def test_the_modes_cover_all_four():
    assert {m for m in rc.MODES.values() if m} == {api.RGBA_RGB, api.RGBA_GREY, api.RGBA_PALETTE, api.RGBA_SYCC}
    assert api.read_info(rc.load("pal"))["lut_size"] == 200 and tuple(api.read_info(rc.load("pal"))["lut_column"][:3]) == rc.PAL_COLUMNS
    assert rc.palette("pal")[1] == (2, 0, 1)  # R takes the column whose lut_column is 0 ...


def test_cmyk_is_unsupported_and_the_text_names_the_colour_space():
    with pytest.raises(api.J2kHipError) as ei:
        api.rgba_mode(rc.load("j7"))
    assert ei.value.code == J2K_HIP_ERR_UNSUPPORTED and "CMYK" in str(ei.value) and "colour space" in str(ei.value)
    assert api.read_info(rc.load("j7"))["color_space"] == 5  # (the header itself is read: only the conversion is refused)


def _swap_cdef_channels(jp2: bytes, a: int, b: int) -> bytes:
    """The cdef box's entries for channels a and b exchange their channel numbers (Cn)."""
    i = jp2.index(b"cdef") + 4
    n = int.from_bytes(jp2[i:i + 2], "big")
    out = bytearray(jp2)
    for k in range(n):
        at = i + 2 + 6 * k
        cn = int.from_bytes(jp2[at:at + 2], "big")
        if cn in (a, b):
            out[at:at + 2] = (b if cn == a else a).to_bytes(2, "big")
    return bytes(out)


def test_an_opacity_channel_that_is_not_the_last_is_unsupported():
    for name in ("j3", "jr1"):
        data = rc.load(name)
        assert api.read_info(data)["alpha"] == 4 and api.rgba_mode(data) == api.RGBA_RGB
        moved = _swap_cdef_channels(data, 0, 3)
        assert api.read_info(moved)["alpha"] == 1  # opacity on channel 0
        with pytest.raises(api.J2kHipError) as ei:
            api.rgba_mode(moved)
        assert ei.value.code == J2K_HIP_ERR_UNSUPPORTED and "opacity" in str(ei.value)
    grey = rc.load("j6")
    assert api.read_info(grey)["alpha"] == 2 and api.rgba_mode(grey) == api.RGBA_GREY
    with pytest.raises(api.J2kHipError) as ei:
        api.rgba_mode(_swap_cdef_channels(grey, 0, 1))
    assert ei.value.code == J2K_HIP_ERR_UNSUPPORTED


@pytest.mark.parametrize("name", ["j1", "k1", "g3", "pal"])
def test_what_read_info_refuses_is_refused_the_same_way(name):
    data = rc.load(name)
    def outcome(fn, d):
        try:
            fn(d)
            return None
        except api.J2kHipError as e:
            return e.code, str(e)
    refused = 0
    for cut in (0, 3, 20, 60, 100, len(data) // 3):  # (a cut behind the headers is no damage either function can see)
        a, b = outcome(api.read_info, data[:cut]), outcome(api.rgba_mode, data[:cut])
        assert a == b, cut
        refused += a is not None
    assert refused >= 3
    from test_read_fallback import _with_palette
    too_big = _with_palette(rc.load("j2"), 300, 3)[0]  # a palette beyond the reference's limits: the fallback's file in both
    with pytest.raises(api.J2kHipError) as a:
        api.read_info(too_big)
    with pytest.raises(api.J2kHipError) as b:
        api.rgba_mode(too_big)
    assert a.value.code == b.value.code == J2K_HIP_ERR_UNSUPPORTED and str(a.value) == str(b.value)


def test_committed_hashes_match_a_live_libopenjp2(opj):
    """rgba.json = rgba_model over libopenjp2's component samples, for every case of rgba_cases (skipped where no libopenjp2
    is installed, like the other fixtures' reproduction)."""
    with open(os.path.join(GOLDEN_DIR, "rgba", "rgba.json")) as f:
        table = json.load(f)["cases"]
    cases = rc.cases()
    assert sorted(table) == sorted(c["id"] for c in cases)
    for c in cases:
        assert rc.sha(rc.expected_from_opj(opj, c)) == table[c["id"]], c["id"]
