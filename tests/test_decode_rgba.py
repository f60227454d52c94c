"""GPU: whole files straight to R, G, B, A (j2k_hip_decode_rgba) -- every mode, sub-sampled chroma, subsample, regions,
Demote, device destinations -- against tests/golden/rgba/rgba.json (rgba_model over libopenjp2's component samples) and
against rgba_model over what j2k_hip_decode itself delivers for the same file.  Exact equality; the whole frame is compared,
so every byte that is no R, G, B, A sample must keep its fill."""
import json
import os

import numpy as np
import pytest

import rgba_cases as rc
import rgba_model as rm
from conftest import GOLDEN_DIR
from j2k_amd import api

pytestmark = pytest.mark.gpu

CASES = rc.cases()


@pytest.fixture(scope="module")
def enc():
    e = api.Encoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(GOLDEN_DIR, "rgba", "rgba.json")) as f:
        return json.load(f)["cases"]


def run(enc, case):
    frame, lay = rc.blank_frame(case)
    w, h = rc.image_size(case)
    return enc.decode_rgba(rc.load(case["file"]), frame, lay, w, h, depth=case["bits"], subsample=case["subsample"], region=case["region"],
                           demote=case["demote"], device=case["device"], alpha=case["alpha"])


def own_components(enc, case):
    """The file's components as j2k_hip_decode delivers them, each on its own grid at its own precision (the top-left sample
    of every sub-sampling cell of the replicated channel), in the form of OpjReplay.decode_comps."""
    data = rc.load(case["file"])
    i = api.read_info(data)
    red = case["subsample"].bit_length() - 1
    shape = (-(-i["height"] >> red), -(-i["width"] >> red))
    out = []
    for c in range(i["channels"]):
        prec = i["comp_depth"][c] or i["depth"]
        chans = [np.zeros(shape, dtype=np.uint16) for _ in range(c + 1)]  # (channel c at its own precision: no conversion)
        enc.decode_channels(data, chans, depth=prec, subsample=case["subsample"])
        out.append(dict(data=chans[c][::i["sub_y"][c], ::i["sub_x"][c]].astype(np.int64), prec=prec, sgnd=0, dx=i["sub_x"][c], dy=i["sub_y"][c]))
    return out


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_file_matches_libopenjp2_through_the_model_and_the_plain_decode(enc, table, case):
    got = run(enc, case)
    assert rc.sha(got) == table[case["id"]]
    want = rc.expected_from_comps(case, own_components(enc, case))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("case", [c for c in CASES if c["file"] == "k4" or c["id"] in ("k1-8", "k2-16-demote", "pal-16", "j6-16-demote-pad8")],
                         ids=lambda c: c["id"])
def test_device_destination(enc, table, case):
    assert rc.sha(run(enc, rc.device_variant(case))) == table[case["id"]]


def test_the_full_window_is_the_whole_image(enc):
    for bits in (8, 16):
        whole = dict(rc._case("k4", bits), region=None)
        window = rc._case("k4", bits, region=(0, 0, 130, 70))
        assert np.array_equal(run(enc, whole), run(enc, window))


def test_channels_anywhere(enc):
    """The planar / arbitrary-view form: planar channels, one of them bottom-up, no alpha."""
    data = rc.load("k1")
    case = rc._case("k1", 8)
    w, h = rc.image_size(case)
    want = rm.file_rgba(rm.SYCC, own_components(enc, case), w, h, 8, 8)
    r, g, b, a = (np.full((h + 1, w + 3), rc.FILL, dtype=np.uint8) for _ in range(4))
    enc.decode_rgba_channels(data, r[:h, :w], g[h - 1::-1, :w], b[:h, :w], None)
    assert np.array_equal(r[:h, :w], want[0]) and np.array_equal(g[:h, :w][::-1], want[1]) and np.array_equal(b[:h, :w], want[2])
    for v in (r, g, b):
        assert (v[h:] == rc.FILL).all() and (v[:, w:] == rc.FILL).all()
    assert (a == rc.FILL).all()
    enc.decode_rgba_channels(data, r[:h, :w], g[:h, :w], b[:h, :w], a[:h - 2, :w - 5])  # a shorter, narrower alpha
    assert (a[:h - 2, :w - 5] == 255).all() and (a[h - 2:] == rc.FILL).all() and (a[:, w - 5:] == rc.FILL).all()


def test_refusals_leave_the_frame_untouched_and_the_handle_intact(enc):
    before = enc.decode_planar(rc.load("j1"))
    k1, case = rc.load("k1"), rc._case("k1", 16)
    frame, lay = rc.blank_frame(case)
    w, h = rc.image_size(case)

    def refused(code, data, fr, la, **kw):
        with pytest.raises(api.J2kHipError) as ei:
            enc.decode_rgba(data, fr, la, w, h, **kw)
        assert ei.value.code == code and (fr == rc.FILL).all()

    f8, l8 = rc.blank_frame(rc._case("k1", 8))
    refused(1, k1, f8, l8, demote=True)                               # Demote with 8-bit samples
    refused(1, k1, frame, lay, depth=12, demote=True)                 # ... and at a depth that is not 16
    refused(1, k1, frame, lay, region=(30, 0, 8, 8))                  # a region that leaves the image
    refused(1, k1, frame, lay, region=(0, 0, 0, 4))
    refused(6, rc.load("j7"), frame, lay)                             # CMYK: J2K_HIP_ERR_UNSUPPORTED
    refused(1, k1[:len(k1) // 2], frame, lay)                         # a damaged file
    # channels of unlike depth, a missing G, a struct of another size
    import ctypes as C
    buf = np.frombuffer(k1, dtype=np.uint8)
    for breakage in ("depth", "base", "size"):
        dst = api.RgbaDst()
        dst.struct_size = C.sizeof(api.RgbaDst)
        for k, p in enumerate((dst.r, dst.g, dst.b, dst.a)):
            api._set_outplane(p, frame.ctypes.data + 2 * ((k + 1) % 4), lay["colbytes"], lay["rowbytes"], 16, 16, w, h)
        if breakage == "depth":
            dst.b.depth = 10
        elif breakage == "base":
            dst.g.base = None
        else:
            dst.struct_size -= 8
        assert enc.L.j2k_hip_decode_rgba(enc.h, buf.ctypes.data, len(k1), 1, None, C.byref(dst)) == 1 and (frame == rc.FILL).all()
    assert np.array_equal(enc.decode_planar(rc.load("j1")), before)  # j2k_hip_decode in the same handle gives what it gave
    assert rc.sha(run(enc, rc._case("k1", 8))) == rc.sha(run(enc, rc._case("k1", 8)))
