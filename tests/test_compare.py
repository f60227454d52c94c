"""GPU: j2k_hip_compare / j2k_hip_compare_device, whole calls.  The expectation is always the numpy model of the definition
(compare_model.py) applied to the source frame and to what the existing decode returns for the file; every integer field is
compared exactly, mse and psnr to the last bit of the header's double formulas."""
import ctypes as C
import hashlib
import math

import numpy as np
import pytest

import compare_model as cm
from conftest import golden_case
from j2k_amd import synth

pytestmark = pytest.mark.gpu

J2K_HIP_ERR_PARAM = 1
F32 = np.float32


@pytest.fixture(scope="module")
def api():
    from j2k_amd import api
    return api


@pytest.fixture(scope="module")
def enc(api):
    e = api.Encoder(0)
    yield e
    e.close()


def _params_from_golden(api, g, **over):
    kw = g["params"]
    args = dict(reversible=kw.get("reversible", True), ycc=kw.get("mct", False), layers=kw.get("layers", 1), tile_size=kw.get("tile", 0),
                num_resolutions=kw.get("numres", 6), cblk=tuple(kw.get("cblk", (64, 64))), comment="")
    args.update(over)
    return api.make_params(g["width"], g["height"], g["ncomp"], g["prec"], **args)


def _model(enc, data, sources, depth, subs=None):
    """compare_model on the sources and on what Encoder.decode_planar returns (at the handle's current layer limit)."""
    dec = enc.decode_planar(data)
    subs = subs or [(1, 1)] * len(sources)
    return cm.diffs(sources, [cm.own_grid(dec[c], subs[c]) for c in range(len(sources))], depth)


def _all_zero(diffs):
    return all(d["differing"] == 0 and d["sum_sq"] == 0 and d["sum_abs"] == 0 and d["max_abs"] == 0 and d["psnr"] == math.inf and d["mse"] == 0.0
               and (d["first_x"], d["first_y"]) == (0, 0) for d in diffs)


def test_lossless_golden_is_all_zero(api, enc, golden):
    g, pl, _, cs = golden_case(golden, "g3_300x200_rgb8_53_rct")
    frame, lay = synth.ae_frame(pl, g["prec"], row_pad_bytes=8)
    p = _params_from_golden(api, g)
    got = enc.compare(cs, p, frame=frame, layout=lay)
    assert len(got) == 3 and _all_zero(got) and [d["samples"] for d in got] == [300 * 200] * 3
    assert got == _model(enc, cs, list(pl), 8)
    assert enc.compare_device(cs, p, frame=frame, layout=lay) == got
    assert enc.compare(cs, p, planar=pl) == got


@pytest.mark.parametrize("name", ["g9_97x61_grey12_97_4lvl", "g9_150x130_rgb8_97_tile64", "g6_300x200_rgb16_97_ict"])
def test_lossy_goldens(api, enc, golden, name):
    """9/7 files: one component of 12 bits, tiles of 64 on 150 x 130, 16 bits with the ICT."""
    g, pl, _, cs = golden_case(golden, name)
    frame, lay = synth.ae_frame(pl, g["prec"], row_pad_bytes=8)
    p = _params_from_golden(api, g)
    got = enc.compare(cs, p, frame=frame, layout=lay)
    want = _model(enc, cs, list(pl), g["prec"])
    assert got == want
    assert all(d["differing"] > 0 and d["sum_sq"] > 0 and 0 < d["psnr"] < math.inf for d in got)
    assert enc.compare_device(cs, p, frame=frame, layout=lay) == got
    assert enc.compare(cs, p, planar=pl) == got
    # the coding fields of the parameters are not read
    assert enc.compare(cs, api.make_params(g["width"], g["height"], g["ncomp"], g["prec"], reversible=True, layers=3, tile_size=32), planar=pl) == got


def test_layer_limit_applies_to_the_compare(api, enc):
    """Three rate-controlled layers: the compare at max_layers 1, 2 and 0 is the model of the decode at that limit."""
    pl = synth.planes(128, 128, 3, 8, 4711, "A")
    frame, lay = synth.ae_frame(pl, 8)
    p = api.make_params(128, 128, 3, 8, reversible=False, ycc=True, rates=[40.0, 20.0, 8.0], comment="")
    cs = enc.encode_host(frame, lay, p)
    assert api.read_info(cs)["layers"] == 3
    results = []
    try:
        for limit in (1, 2, 0):
            enc.set_max_layers(limit)
            got = enc.compare(cs, p, frame=frame, layout=lay)
            assert got == _model(enc, cs, list(pl), 8), limit
            assert enc.compare_device(cs, p, frame=frame, layout=lay) == got
            results.append(got)
    finally:
        enc.set_max_layers(0)
    assert results[0] != results[1] and results[1] != results[2] and results[0] != results[2]


@pytest.mark.parametrize("rev", [True, False], ids=["53", "97"])
def test_rgb_to_sycc_420(api, enc, rev):
    w, h = 65, 33
    pl = synth.planes(w, h, 3, 8, 99, "B")
    frame, lay = synth.ae_frame(pl, 8, row_pad_bytes=4)
    subs = [(1, 1), (2, 2), (2, 2)]
    p = api.make_params(w, h, 3, 8, reversible=rev, num_resolutions=4, comment="", sub=subs, rgb_to_sycc=True)
    cs = enc.encode_host(frame, lay, p)
    info = api.read_info(cs)
    assert info["sub_x"][:3] == [1, 2, 2] and info["sub_y"][:3] == [1, 2, 2]
    sources = cm.source_components([pl[c].astype(np.uint8) for c in range(3)], [8] * 3, 8, rgb_to_sycc=(2, 2))
    got = enc.compare(cs, p, frame=frame, layout=lay)
    assert [d["samples"] for d in got] == [w * h, 33 * 17, 33 * 17]
    assert got == _model(enc, cs, sources, 8, subs)
    assert _all_zero(got) if rev else all(d["differing"] > 0 for d in got)
    assert enc.compare_device(cs, p, frame=frame, layout=lay) == got


def test_comp_sub_planes(api, enc):
    """Components given at their own sizes (4:2:2), 9/7."""
    w, h = 65, 33
    subs = [(1, 1), (2, 1), (2, 1)]
    pl = synth.planes(w, h, 3, 10, 7, "B")
    comps = [np.ascontiguousarray(pl[c][:-(-h // sy), :-(-w // sx)]) for c, (sx, sy) in enumerate(subs)]
    p = api.make_params(w, h, 3, 10, reversible=False, num_resolutions=3, comment="", sub=subs)
    cs = enc.encode_components_host(comps, p)
    got = enc.compare(cs, p, comps=comps)
    assert got == _model(enc, cs, comps, 10, subs) and all(d["differing"] > 0 for d in got)
    assert enc.compare_device(cs, p, comps=comps) == got


def test_float_source(api, enc):
    """An ARGB128 frame of floats standing for 16-bit samples, written to a 12-bit file."""
    w, h = 65, 33
    rng = np.random.default_rng(3)
    x = rng.uniform(-0.05, 1.05, size=(4, h, w)).astype(F32)
    x[1, 0, :4] = np.array([np.nan, np.inf, -1.0, 1.0], F32)
    rowbytes = 16 * w + 16
    buf = np.zeros(h * rowbytes, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf.view(F32), shape=(h, w, 4), strides=(rowbytes, 16, 4), writeable=True)
    for slot, c in zip((1, 2, 3, 0), x):
        view[:, :, slot] = c
    lay = dict(sample_bytes=4, colbytes=16, rowbytes=rowbytes, channel_offsets=(0, 4, 8, 12), depth=16)
    sources = cm.source_components(list(x), [16] * 4, 12)
    for rev in (True, False):
        p = api.make_params(w, h, 4, 12, reversible=rev, ycc=True, num_resolutions=4, comment="")
        cs = enc.encode_host(buf, lay, p)
        got = enc.compare(cs, p, frame=buf, layout=lay)
        assert got == _model(enc, cs, sources, 12)
        assert _all_zero(got) if rev else all(d["differing"] > 0 for d in got[:3])
        assert enc.compare_device(cs, p, frame=buf, layout=lay) == got


def test_one_sample_altered_after_the_encode(api, enc, golden):
    g, pl, _, cs = golden_case(golden, "g4_300x200_rgb16_53_rct_tile128")
    p = _params_from_golden(api, g)
    for c, x, y in ((0, 0, 0), (1, 299, 199), (2, 137, 64)):
        changed = pl.copy()
        changed[c, y, x] ^= 0x40
        frame, lay = synth.ae_frame(changed, g["prec"])
        for got in (enc.compare(cs, p, frame=frame, layout=lay), enc.compare_device(cs, p, frame=frame, layout=lay)):
            for k in range(3):
                if k == c:
                    assert (got[k]["differing"], got[k]["first_x"], got[k]["first_y"], got[k]["max_abs"], got[k]["sum_sq"]) == (1, x, y, 0x40, 0x40 ** 2)
                else:
                    assert _all_zero([got[k]])
            assert got == _model(enc, cs, list(changed), 16)


def test_the_handle_encodes_and_decodes_as_before(api, enc, golden):
    g, pl, _, cs = golden_case(golden, "g6_300x200_rgb8_97_ict")
    frame, lay = synth.ae_frame(pl, g["prec"], row_pad_bytes=8)
    p = _params_from_golden(api, g)
    assert enc.compare(cs, p, frame=frame, layout=lay)[0]["differing"] > 0
    assert enc.encode_host(frame, lay, p) == cs
    dec = enc.decode_planar(cs)
    assert hashlib.sha256(np.ascontiguousarray(dec.astype(np.int32)).tobytes()).hexdigest() == g["decoded_sha256"]
    assert enc.compare_device(cs, p, frame=frame, layout=lay)[0]["differing"] > 0
    assert enc.encode_host(frame, lay, p) == cs


def test_a_mismatching_file_is_refused_like_compare_check(api, enc, golden):
    g, pl, _, cs = golden_case(golden, "g3_300x200_rgb8_53_rct")
    frame, lay = synth.ae_frame(pl, g["prec"])
    file = np.frombuffer(cs, dtype=np.uint8)
    for kw in (dict(width=299), dict(depth=12), dict(channels=4)):
        a = dict(width=300, height=200, channels=3, depth=8)
        a.update(kw)
        p = api.make_params(a["width"], a["height"], a["channels"], a["depth"])
        with pytest.raises(api.J2kHipError) as want:
            api.compare_check(p, cs)
        diffs = (api.Diff * 4)()
        C.memset(diffs, 0xA5, C.sizeof(diffs))
        for d in diffs:
            d.struct_size = C.sizeof(api.Diff)
        before = bytes(diffs)
        planes = api.planes_from_layout(frame.ctypes.data, lay, 3)
        for fn in (enc.L.j2k_hip_compare, enc.L.j2k_hip_compare_device):  # (refused before the planes are looked at: host pointers do no harm)
            rc = fn(enc.h, C.byref(p), planes, file.ctypes.data, file.size, diffs, 4)
            assert rc == J2K_HIP_ERR_PARAM == want.value.code
            assert f"j2k_hip error {rc}: {enc.L.j2k_hip_last_error(enc.h).decode()}" == str(want.value)
            assert bytes(diffs) == before
    # a file cut short compares what decodes
    cut = cs[:len(cs) * 6 // 10]
    p = _params_from_golden(api, g)
    got = enc.compare(cut, p, frame=frame, layout=lay)
    assert got == _model(enc, cut, list(pl), 8) and any(d["differing"] > 0 for d in got)
