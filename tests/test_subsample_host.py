"""CPU: sub-sampled components on the write side (j2k_hip_params.comp_sub_x / comp_sub_y / rgb_to_sycc) as far as it goes
without a device -- SIZ and the whole main header against libopenjp2's files, the JP2 boxes, what is refused, the numpy model
of the RGB -> Y Cb Cr front end (sycc_model.py), and the fixtures against a live libopenjp2 where one is installed."""
import importlib.util
import json
import os
import struct

import numpy as np
import pytest

import rgba_model
import subsample_cases as cases
import sycc_model
from j2k_amd import api

J2K_HIP_ERR_PARAM = 1
S422, S420 = [(1, 1), (2, 1), (2, 1)], [(1, 1), (2, 2), (2, 2)]


@pytest.mark.parametrize("name", cases.NAMES)
def test_main_header_matches_libopenjp2_and_siz_carries_the_factors(name):
    want = cases.main_header_of(cases.golden_bytes(name))
    got = cases.strip_com(api.main_header(cases.params(api, name)))
    assert got == want
    siz = got.index(b"\xff\x51")
    nc = struct.unpack(">H", got[siz + 38:siz + 40])[0]
    assert [(got[siz + 41 + 3 * c], got[siz + 42 + 3 * c]) for c in range(nc)] == cases.subs(name)


def _boxes(b: bytes):
    out, pos = [], 0
    while pos < len(b):
        n, typ = struct.unpack(">I4s", b[pos:pos + 8])
        out.append((typ, b[pos + 8:pos + n] if n else b[pos + 8:]))
        pos += n if n else len(b)
    return out


@pytest.mark.parametrize("alpha", [False, True])
def test_jp2_boxes_of_a_sycc_420_image(alpha):
    """The replay's JP2 writer (OpjReplay.encode_jp2) takes components of one size only, so the boxes are checked field by
    field against T.800 Annex I instead of against libopenjp2's bytes: ihdr (I.5.3.1) holds the reference grid's size -- it
    knows nothing of sub-sampling --, colr (I.5.3.3) the enumerated colour space 18 (sYCC), cdef (I.5.3.6) Y, Cb, Cr as
    colours 1, 2, 3 and the fourth component as opacity of the whole image."""
    nc = 4 if alpha else 3
    p = api.make_params(97, 61, nc, 8, jp2=True, color_space=3, alpha_channel=3 if alpha else -1, sub=S420 + [(1, 1)] * (nc - 3), rgb_to_sycc=True)
    fh = api.file_header(p, 1000)
    top = _boxes(fh[:-8])
    assert [t for t, _ in top] == [b"jP  ", b"ftyp", b"jp2h"]
    assert fh[-8:] == struct.pack(">I4s", 1008, b"jp2c")
    inner = dict(_boxes(top[2][1]))
    assert inner[b"ihdr"] == struct.pack(">IIHBBBB", 61, 97, nc, 7, 7, 0, 0)  # height, width, NC, BPC = 8 bits unsigned, C = 7, UnkC, IPR
    assert inner[b"colr"] == struct.pack(">BBBI", 1, 0, 0, 18)  # METH 1, PREC 0, APPROX 0, EnumCS 18 = sYCC
    if alpha:
        assert inner[b"cdef"] == struct.pack(">H", 4) + b"".join(struct.pack(">HHH", *e) for e in [(0, 0, 1), (1, 0, 2), (2, 0, 3), (3, 1, 0)])
    else:
        assert b"cdef" not in inner
    # and the sub-sampling changes no box: the same image as three full-size sYCC components
    q = api.make_params(97, 61, nc, 8, jp2=True, color_space=3, alpha_channel=3 if alpha else -1)
    assert api.file_header(q, 1000) == fh


REFUSALS = [
    ("factor 3", dict(sub=[(1, 1), (3, 1), (3, 1)]), "comp_sub"),
    ("factor 8", dict(sub=[(1, 1), (1, 8), (1, 1)]), "comp_sub"),
    ("component 0", dict(sub=[(2, 1), (2, 1), (2, 1)]), "component 0"),
    ("ycc with sub-sampling", dict(sub=S422, ycc=True), "ycc"),
    ("ycc with rgb_to_sycc", dict(rgb_to_sycc=True, ycc=True), "rgb_to_sycc"),
    ("layer_psnr with sub-sampling", dict(sub=S420, psnr=[35.0]), "layer_psnr"),
    ("layer_psnr with rgb_to_sycc", dict(rgb_to_sycc=True, psnr=[35.0]), "layer_psnr"),
    ("rgb_to_sycc 4:1:1", dict(rgb_to_sycc=True, sub=[(1, 1), (4, 1), (4, 1)]), "rgb_to_sycc"),
    ("rgb_to_sycc unlike chroma", dict(rgb_to_sycc=True, sub=[(1, 1), (2, 1), (2, 2)]), "rgb_to_sycc"),
    ("rgb_to_sycc 1x2", dict(rgb_to_sycc=True, sub=[(1, 1), (1, 2), (1, 2)]), "rgb_to_sycc"),
]


@pytest.mark.parametrize("what, kw, word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_name_their_field(what, kw, word):
    with pytest.raises(api.J2kHipError) as ei:
        api.main_header(api.make_params(128, 128, 3, 8, reversible=False, **kw))
    assert ei.value.code == J2K_HIP_ERR_PARAM
    assert word in str(ei.value)
    assert "comp_sub" in str(ei.value) or "rgb_to_sycc" in str(ei.value)


def test_more_refusals():
    for nc, kw, word in [(1, dict(rgb_to_sycc=True), "rgb_to_sycc"), (2, dict(rgb_to_sycc=True), "rgb_to_sycc"),
                         (4, dict(rgb_to_sycc=True, sub=S420 + [(2, 2)]), "rgb_to_sycc")]:
        with pytest.raises(api.J2kHipError) as ei:
            api.main_header(api.make_params(128, 128, nc, 8, **kw))
        assert ei.value.code == J2K_HIP_ERR_PARAM and word in str(ei.value), (nc, kw)
    for kw in (dict(sub=S422), dict(rgb_to_sycc=True)):
        with pytest.raises(api.J2kHipError) as ei:
            api.main_header(api.make_params(512, 270, 3, 12, reversible=False, dci_profile=3, **kw))
        assert ei.value.code == J2K_HIP_ERR_PARAM and "dci_profile" in str(ei.value), kw
        assert "comp_sub" in str(ei.value) or "rgb_to_sycc" in str(ei.value)
    api.main_header(api.make_params(512, 270, 3, 12, reversible=False, dci_profile=3))  # the same without is fine
    # what combines: a byte budget, a code-block style
    api.main_header(api.make_params(128, 128, 3, 8, sub=S420, rates=[20.0, 5.0]))
    api.main_header(api.make_params(128, 128, 3, 8, sub=S420, cblk_style=1 | 4))
    api.main_header(api.make_params(128, 128, 4, 8, sub=S422 + [(1, 1)], rgb_to_sycc=True))


def test_all_ones_factors_write_the_header_they_always_wrote(golden):
    g = golden["g3_300x200_rgb8_53_rct"]
    with open(os.path.join(cases.GOLDEN_DIR, "g3_300x200_rgb8_53_rct.j2k"), "rb") as f:
        want = cases.main_header_of(f.read())
    kw = dict(ycc=g["params"]["mct"], num_resolutions=g["params"]["numres"], comment="")
    assert api.main_header(api.make_params(300, 200, 3, 8, **kw)) == want
    assert api.main_header(api.make_params(300, 200, 3, 8, sub=[(1, 1)] * 3, **kw)) == want
    assert api.main_header(api.make_params(300, 200, 3, 8, sub=[(0, 0)] * 3, **kw)) == want


# ---------------------------------------------------------------------------------------------- the model of the front end
def test_model_rows_sum_as_stated():
    assert sycc_model.Y_R + sycc_model.Y_G + sycc_model.Y_B == 65536
    assert sycc_model.CB_R + sycc_model.CB_G + sycc_model.CB_B == 0
    assert sycc_model.CR_R + sycc_model.CR_G + sycc_model.CR_B == 0


@pytest.mark.parametrize("depth", [8, 10, 12, 16])
@pytest.mark.parametrize("sub", [(1, 1), (2, 1), (2, 2)])
def test_model_grey_gives_neutral_chroma_and_extremes_clamp(depth, sub):
    top, h = (1 << depth) - 1, 1 << (depth - 1)
    ramp = np.arange(0, top + 1, max(1, (top + 1) // 256), dtype=np.int64)
    grey = np.tile(ramp, (3, 1))  # three rows, odd height for the vertical factor
    y, cb, cr = sycc_model.sycc_planes([grey, grey, grey], depth, sub)
    assert np.array_equal(y, grey)
    assert np.all(cb == h) and np.all(cr == h)
    assert cb.shape == (-(-3 // sub[1]), -(-ramp.size // sub[0]))
    # the extremes: pure blue drives Cb to h + top / 2 rounded up = top + 1, pure red Cr: both clamp to top; their opposites reach 0 or 1
    z, t = np.zeros((2, 2), np.int64), np.full((2, 2), top, np.int64)
    _, cb, cr = sycc_model.sycc_planes([z, z, t], depth, sub)
    assert np.all(cb == top) and np.all(cr >= 0)
    _, cb, cr = sycc_model.sycc_planes([t, z, z], depth, sub)
    assert np.all(cr == top) and np.all(cb >= 0)
    _, cb, cr = sycc_model.sycc_planes([t, t, z], depth, sub)
    assert np.all((cb >= 0) & (cb <= 1))


def test_model_edges_repeat_the_last_column_and_row():
    r = np.array([[10, 20, 200], [30, 40, 100], [250, 0, 7]], dtype=np.int64)
    g, b = r[::-1].copy(), r.T.copy()
    rp, gp, bp = (np.pad(p, ((0, 1), (0, 1)), mode="edge") for p in (r, g, b))
    want = sycc_model.sycc_planes([rp, gp, bp], 8, (2, 2))
    got = sycc_model.sycc_planes([r, g, b], 8, (2, 2))
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert got[1].shape == (2, 2)


def _round_trip_bound(depth):
    """Largest |R, G, B error| of model -> rgba_model at 4:4:4, from the model's own numbers: Y, Cb and Cr are each within
    0.5 of their exact values (the rounding; h + 127.5.. clamps by at most that too) plus what the 16-bit coefficients are off
    the matrix the reader inverts; the reader multiplies the chroma errors by its own gains and rounds once more (0.5)."""
    top = (1 << depth) - 1
    ideal_y = (0.299, 0.587, 0.114)
    ideal_cb = (-0.299 / 1.772, -0.587 / 1.772, 0.5)
    ideal_cr = (0.5, -0.587 / 1.402, -0.114 / 1.402)
    coef = lambda got, ideal: sum(abs(a / 65536.0 - b) for a, b in zip(got, ideal)) * top
    ey = 0.5 + coef((sycc_model.Y_R, sycc_model.Y_G, sycc_model.Y_B), ideal_y)
    ecb = 0.5 + coef((sycc_model.CB_R, sycc_model.CB_G, sycc_model.CB_B), ideal_cb)
    ecr = 0.5 + coef((sycc_model.CR_R, sycc_model.CR_G, sycc_model.CR_B), ideal_cr)
    fl = top * 2.0 ** -22  # the reader's float32 arithmetic
    return [int(np.floor(ey + float(rgba_model.K_CR_R) * ecr + 0.5 + fl)),
            int(np.floor(ey + float(rgba_model.K_CR_G) * ecr + float(rgba_model.K_CB_G) * ecb + 0.5 + fl)),
            int(np.floor(ey + float(rgba_model.K_CB_B) * ecb + 0.5 + fl))]


def test_model_round_trip_through_the_rgba_reader_at_444():
    """A property of the definition, not of the kernel.  Bound computed by _round_trip_bound: 1, 1, 1 at 8 bits.
    Observed maxima (8 bits; exhaustive grey ramp: 0, 0, 0; 4096 seeded colours + the cube's corners): R 1, G 1, B 1."""
    depth = 8
    bound = _round_trip_bound(depth)
    ramp = np.arange(256, dtype=np.int64)[None, :]
    rng = np.random.default_rng(20240611)
    col = rng.integers(0, 256, size=(3, 64, 64), dtype=np.int64)
    corners = np.array([[(i >> k) & 1 for i in range(8)] for k in range(3)], dtype=np.int64)[:, None, :] * 255
    worst = [0, 0, 0]
    for planes in ([ramp, ramp, ramp], list(col), list(corners)):
        ycc = sycc_model.sycc_planes(planes, depth)
        h, w = planes[0].shape
        back = rgba_model.rgba(rgba_model.SYCC, ycc, [depth] * 3, [(1, 1)] * 3, w, h, depth, 8)
        for c in range(3):
            worst[c] = max(worst[c], int(np.abs(back[c] - planes[c]).max()))
        if planes[0] is ramp:
            assert all(np.array_equal(back[c], ramp) for c in range(3))
    print("round-trip bound", bound, "observed", worst)
    assert all(w <= b for w, b in zip(worst, bound)), (worst, bound)


def test_fixtures_match_a_live_libopenjp2():
    from oracle.oracle import OpjReplay, find_openjpeg_libs
    try:
        if not find_openjpeg_libs():
            raise OSError("no libopenjp2 found")
        OpjReplay()
    except OSError as e:
        pytest.skip(f"libopenjp2 replay unavailable: {e}")
    spec = importlib.util.spec_from_file_location("make_subsample_golden", os.path.join(cases.GOLDEN_DIR, "make_subsample_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    meta, files = gen.generate()
    assert sorted(files) == cases.NAMES
    for name, cs in files.items():
        assert cs == cases.golden_bytes(name), name
        assert json.loads(json.dumps(meta[name])) == cases.CASES[name], name
