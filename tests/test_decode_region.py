"""Region decode end to end (run with -m gpu): j2k_hip_decode_region / _region_device against the crop of the whole image.

The expected samples come from outside the code under test: the generator's planes for lossless files at full size, the
oracle's decode otherwise, and for the files libopenjp2 wrote (tests/golden/ext) libopenjp2's components, replicated and
offset as tests/test_read_fallback.py builds them.  One file per way a window can go wrong: one block per band; odd sizes
with 9/7; tiles (a window across four of them, one inside one); sub-sampled components with odd window origins (the
replication phase); image and tile origin offsets; code-block styles with segments (the lane kernel); a region of
interest by MAXSHIFT; JP2 with four channels.  Work is really skipped: j2k_hip_stats.num_codeblocks of a window decode
is held to a bound that no decode of everything meets."""
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR
from j2k_amd import api, synth

pytestmark = pytest.mark.gpu

# name -> (file under tests/golden, where the expected samples come from)
FILES = {
    "g1_64x64_grey_5lvl": ("g1_64x64_grey_5lvl.j2k", "lossless"),
    "g9_97x61_grey12_97_4lvl": ("g9_97x61_grey12_97_4lvl.j2k", "oracle"),
    "g4_300x200_rgb16_53_rct_tile128": ("g4_300x200_rgb16_53_rct_tile128.j2k", "lossless"),
    "u1_300x200_ycc420_8_53": ("ext/u1_300x200_ycc420_8_53.j2k", "opj"),
    "u2_301x199_ycc422_10_97_tile128": ("ext/u2_301x199_ycc422_10_97_tile128.j2k", "opj"),
    "u6_200x150_rgb8_53_offset": ("ext/u6_200x150_rgb8_53_offset.j2k", "opj"),
    "s4_300x200_rgb16_97_all_styles_2layers_tile128": ("ext/s4_300x200_rgb16_97_all_styles_2layers_tile128.j2k", "opj"),
    "r2_300x200_rgb10_97_ict_roi_comp0_shift7_r12": ("ext/r2_300x200_rgb10_97_ict_roi_comp0_shift7_r12.j2k", "opj"),
    "j3_64x48_rgba8_srgb_alpha": ("j3_64x48_rgba8_srgb_alpha.jp2", "lossless"),
}
CASES = [(n, s) for n in FILES for s in ((1, 2, 4) if n == "g1_64x64_grey_5lvl" else (1, 2))]
G4 = "g4_300x200_rgb16_53_rct_tile128"


@pytest.fixture(scope="module")
def enc():
    e = api.Encoder(0)
    yield e
    e.close()


def _load(name):
    with open(os.path.join(GOLDEN_DIR, FILES[name][0]), "rb") as f:
        return f.read()


_EXPECTED = {}


def _expected(request, golden, oracle, name, sub):
    """(channels, h, w) int32: the whole image at this subsample, computed once per (file, subsample) and never changed."""
    key = (name, sub)
    if key in _EXPECTED:
        return _EXPECTED[key]
    data, g, red, kind = _load(name), golden[name], sub.bit_length() - 1, FILES[name][1]
    h, w = -(-g["height"] >> red), -(-g["width"] >> red)
    if kind == "opj":
        opj = request.getfixturevalue("opj")
        chans = []
        for comp in opj.decode_comps(data, red)[:4]:
            full = np.repeat(np.repeat(comp["data"], comp["dy"], axis=0), comp["dx"], axis=1)[:h, :w]
            chans.append(full + (1 << (comp["prec"] - 1)) if comp["sgnd"] else full)
        exp = np.stack(chans).astype(np.int32)
    elif kind == "lossless" and red == 0:
        exp = synth.planes(g["width"], g["height"], g["ncomp"], g["prec"], g["seed"], g["dist"])
    else:
        exp = oracle.decode(data, red)
    assert exp.shape[1:] == (h, w)
    exp.setflags(write=False)
    _EXPECTED[key] = exp
    return exp


def _windows(name, sub, w, h):
    """(0, 0, 1, 1), the last pixel, a rectangle across the middle at an odd origin, the whole image; for the tiled file a
    window across its four tiles and one inside one tile."""
    ws = [(0, 0, 1, 1), (w - 1, h - 1, 1, 1), ((w // 3) | 1, (h // 3) | 1, max(w // 3, 1), max(h // 3, 1)), (0, 0, w, h)]
    if name == G4:
        ws += [(120 // sub, 120 // sub, 16 // sub, 16 // sub), (10, 10, 40 // sub, 40 // sub)]
        assert 120 // sub < 128 // sub < 120 // sub + 16 // sub
    if name.startswith("u"):
        ws += [(33 // sub | 1, 17 // sub | 1, 51, 37)]
    return ws


@pytest.mark.parametrize("name,sub", CASES, ids=[f"{n}-sub{s}" for n, s in CASES])
def test_region_is_the_crop_of_the_whole_image(request, enc, golden, oracle, name, sub):
    data = _load(name)
    exp = _expected(request, golden, oracle, name, sub)
    nc, h, w = exp.shape
    whole = enc.decode_planar(data, subsample=sub)
    full_blocks = enc.stats()["num_codeblocks"]
    assert np.array_equal(whole.astype(np.int32), exp)
    for (x, y, ww, wh) in _windows(name, sub, w, h):
        got = enc.decode_region_planar(data, (x, y, ww, wh), subsample=sub)
        assert got.shape == (nc, wh, ww) and got.dtype == whole.dtype
        assert np.array_equal(got.astype(np.int32), exp[:, y:y + wh, x:x + ww]), (name, sub, (x, y, ww, wh))
        assert enc.stats()["num_codeblocks"] <= full_blocks
        if (x, y, ww, wh) == (0, 0, w, h):
            assert got.tobytes() == whole.tobytes()
            assert enc.stats()["num_codeblocks"] == full_blocks


@pytest.mark.parametrize("lanes", [0, 2], ids=["wave-per-block", "lane-per-block"])
def test_region_under_both_tier1_kernels(request, enc, golden, oracle, lanes):
    exp = _expected(request, golden, oracle, G4, 1)
    api.tune("t1dec_lanes", lanes)
    try:
        for (x, y, ww, wh) in _windows(G4, 1, 300, 200):
            got = enc.decode_region_planar(_load(G4), (x, y, ww, wh))
            assert np.array_equal(got.astype(np.int32), exp[:, y:y + wh, x:x + ww]), (lanes, (x, y, ww, wh))
    finally:
        api.tune("t1dec_lanes", 1)


@pytest.mark.parametrize("name", [G4, "u2_301x199_ycc422_10_97_tile128", "j3_64x48_rgba8_srgb_alpha"])
def test_region_into_device_channels(request, enc, golden, oracle, name):
    for sub in (1, 2):
        exp = _expected(request, golden, oracle, name, sub)
        _, h, w = exp.shape
        for (x, y, ww, wh) in _windows(name, sub, w, h)[1:3]:
            got = enc.decode_region_planar(_load(name), (x, y, ww, wh), subsample=sub, device=True)
            assert np.array_equal(got.astype(np.int32), exp[:, y:y + wh, x:x + ww]), (name, sub, (x, y, ww, wh))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_region_into_ae_frame_touches_only_the_windows_samples(request, enc, golden, oracle, device):
    """An ARGB64 frame of the image's size with row padding: the window's R, G, B samples land at the top-left, every other
    byte -- A samples, the pixels outside the window's extent, the padding -- keeps its fill."""
    exp = _expected(request, golden, oracle, G4, 1)
    ref, lay = synth.ae_frame(np.zeros((3, 200, 300), dtype=np.int32), 16, row_pad_bytes=12)
    for (x, y, ww, wh) in ((121, 77, 58, 41), (0, 0, 300, 200), (299, 199, 1, 1)):
        frame = np.full_like(ref, 0xA5)
        enc.decode_ae(_load(G4), frame, lay, 300, 200, 3, device=device, region=(x, y, ww, wh))
        px = np.lib.stride_tricks.as_strided(frame.view(np.uint16), shape=(200, 300, 4), strides=(lay["rowbytes"], 8, 2))
        assert np.array_equal(px[:wh, :ww, 1:].transpose(2, 0, 1).astype(np.int32), exp[:, y:y + wh, x:x + ww])
        px[:wh, :ww, 1:] = 0xA5A5
        assert (frame == 0xA5).all(), (x, y, ww, wh)


def test_region_into_a_smaller_destination(request, enc, golden, oracle):
    """planes[i].width / .height limit what is copied: the destination receives the window's top-left part."""
    for name, sub in ((G4, 1), ("u1_300x200_ycc420_8_53", 2)):
        exp = _expected(request, golden, oracle, name, sub)
        x, y, ww, wh = 45, 31, 90, 60
        out = np.full((exp.shape[0], 25, 37), 7, dtype=np.uint16 if name == G4 else np.uint8)
        enc.decode_region_planar(_load(name), (x, y, ww, wh), subsample=sub, out=out)
        assert np.array_equal(out.astype(np.int32), exp[:, y:y + 25, x:x + 37]), name


@pytest.mark.parametrize("rev", [True, False], ids=["53", "97"])
def test_region_decodes_fewer_code_blocks(enc, oracle, rev):
    """512 x 512 noise, 4 resolutions, 32 x 32 code-blocks: 256 blocks, all coded.  The window (200, 200, 48, 48) needs 31 of
    them by the support of the filters (3 + 12 + 12 + 4); at most 64 -- a quarter of the image's -- may be decoded, which
    leaves room for windows rounded to pairs or vector widths and none for an implementation that decodes everything."""
    noise = np.random.default_rng(512).integers(0, 256, size=(1, 512, 512)).astype(np.int32)
    cs = enc.encode_planar_host(noise, api.make_params(512, 512, 1, 8, reversible=rev, num_resolutions=4, cblk=(32, 32)))
    exp = noise if rev else oracle.decode(cs)
    assert np.array_equal(enc.decode_planar(cs).astype(np.int32), exp)
    assert enc.stats()["num_codeblocks"] == 256
    got = enc.decode_region_planar(cs, (200, 200, 48, 48))
    nblocks = enc.stats()["num_codeblocks"]
    print(f"window (200, 200, 48, 48) of 512 x 512, {'5/3' if rev else '9/7'}: {nblocks} of 256 code-blocks decoded")
    assert np.array_equal(got.astype(np.int32), exp[:, 200:248, 200:248])
    assert nblocks <= 64


def test_region_errors_leave_destination_and_handle_alone(request, enc, golden, oracle):
    name = "g9_97x61_grey12_97_4lvl"
    data = _load(name)
    exp = _expected(request, golden, oracle, name, 1)
    #            w == 0          x + w beyond the width   inside at subsample 1, outside the 49 x 31 image at 2
    for rect, sub in (((5, 5, 0, 4), 1), ((90, 0, 8, 8), 1), ((60, 40, 8, 8), 2), ((0, 0, 4, 0), 1), ((0, 60, 1, 2), 1)):
        out = np.full((1, 8, 8), 0x1234, dtype=np.uint16)
        with pytest.raises(api.J2kHipError) as ei:
            enc.decode_region_planar(data, rect, subsample=sub, out=out)
        assert ei.value.code == 1 and "region" in str(ei.value), (rect, str(ei.value))  # J2K_HIP_ERR_PARAM
        assert (out == 0x1234).all()
        assert np.array_equal(enc.decode_planar(data).astype(np.int32), exp)
    got = enc.decode_region_planar(data, (60, 40, 8, 8))
    assert np.array_equal(got.astype(np.int32), exp[:, 40:48, 60:68])


def test_region_of_empty_code_blocks(enc, oracle):
    """A constant plane: no code-block holds a pass, the Tier-1 table is empty and nothing is refused."""
    const = np.full((1, 136, 200), 128, dtype=np.int32)
    cs = enc.encode_planar_host(const, api.make_params(200, 136, 1, 8, reversible=True, num_resolutions=4))
    exp = oracle.decode(cs)
    for rect in ((0, 0, 1, 1), (77, 31, 40, 50), (0, 0, 200, 136)):
        x, y, ww, wh = rect
        got = enc.decode_region_planar(cs, rect)
        assert enc.stats()["num_codeblocks"] == 0
        assert np.array_equal(got.astype(np.int32), exp[:, y:y + wh, x:x + ww])
