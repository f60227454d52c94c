"""CPU: the header side of j2k_hip_compare (include/j2k_hip.h: j2k_hip_compare_check -- does a file describe the image of the
parameters?  headers only, no device), and the numpy model of the definition (compare_model.py) on values worked out by hand."""
import math
import os

import numpy as np
import pytest

import compare_model as cm
import subsample_cases as sub_cases
from conftest import GOLDEN_DIR
from j2k_amd import api
from test_read_fallback import _with_coc

J2K_HIP_ERR_PARAM, J2K_HIP_ERR_UNSUPPORTED = 1, 6


def load(name):
    for ext in (".j2k", ".jp2"):
        path = os.path.join(GOLDEN_DIR, name + ext)
        if os.path.exists(path):
            return open(path, "rb").read()
    return None


def refused(params, data):
    with pytest.raises(api.J2kHipError) as ei:
        api.compare_check(params, data)
    return ei.value


def test_compare_check_accepts_every_encoder_fixture(golden):
    """Every committed file of golden.json and of the sub-sampling fixtures against the geometry that wrote it; the coding
    fields are left at their defaults or set to nonsense for that file: they are not read."""
    seen = 0
    for name, g in golden.items():
        data = None if name.startswith("_") else load(name)
        if data is None:
            continue
        api.compare_check(api.make_params(g["width"], g["height"], g["ncomp"], g["prec"]), data)
        api.compare_check(api.make_params(g["width"], g["height"], g["ncomp"], g["prec"], reversible=False, ycc=g["ncomp"] >= 3, layers=7,
                                          tile_size=32, num_resolutions=3, progression=4, cblk_style=1, jp2=True, rates=[50.0, 10.0]), data)
        seen += 1
    assert seen >= 30
    for name in sub_cases.NAMES:
        api.compare_check(sub_cases.params(api, name), sub_cases.golden_bytes(name))
        g = sub_cases.entry(name)
        api.compare_check(api.make_params(g["width"], g["height"], len(g["sub"]), g["prec"], sub=sub_cases.subs(name)), sub_cases.golden_bytes(name))


def test_compare_check_names_the_field_that_differs():
    g3 = load("g3_300x200_rgb8_53_rct")  # 300 x 200, three components of 8 bits
    for kw, field in ((dict(width=301), "width"), (dict(height=199), "height"), (dict(channels=4), "channels"), (dict(channels=1), "channels"),
                      (dict(depth=10), "depth")):
        a = dict(width=300, height=200, channels=3, depth=8)
        a.update(kw)
        e = refused(api.make_params(a["width"], a["height"], a["channels"], a["depth"]), g3)
        assert e.code == J2K_HIP_ERR_PARAM and field in str(e), (kw, str(e))
    # sub-sampling factors: a full-size file against 4:2:0 parameters, and a 4:2:2 file against full-size and 4:2:0 parameters
    e = refused(api.make_params(300, 200, 3, 8, sub=[(1, 1), (2, 2), (2, 2)]), g3)
    assert e.code == J2K_HIP_ERR_PARAM and "comp_sub_x" in str(e)
    name = sub_cases.by_prefix("q1")
    g = sub_cases.entry(name)
    subs = sub_cases.subs(name)
    assert any(s != (1, 1) for s in subs)
    e = refused(api.make_params(g["width"], g["height"], len(subs), g["prec"]), sub_cases.golden_bytes(name))
    assert e.code == J2K_HIP_ERR_PARAM and "comp_sub_x" in str(e)
    other = [(1, 1)] + [(sx, 4 if sy == 1 else 1) for sx, sy in subs[1:]]
    e = refused(api.make_params(g["width"], g["height"], len(subs), g["prec"], sub=other), sub_cases.golden_bytes(name))
    assert e.code == J2K_HIP_ERR_PARAM and "comp_sub_y" in str(e)


def test_compare_check_refuses_a_signed_component():
    data = open(os.path.join(GOLDEN_DIR, "ext", "u5_97x61_grey12_signed_53.j2k"), "rb").read()
    info = api.read_info(data)
    assert info["comp_signed"][0] == 1 and (info["width"], info["height"], info["channels"], info["depth"]) == (97, 61, 1, 12)
    e = refused(api.make_params(97, 61, 1, 12), data)
    assert e.code == J2K_HIP_ERR_PARAM and "signed" in str(e)


def test_compare_check_refuses_a_component_of_2_to_the_32_samples():
    """By the parameters alone: the file is not looked at."""
    g3 = load("g3_300x200_rgb8_53_rct")
    for w, h in ((65536, 65536), (1 << 20, 4096)):
        e = refused(api.make_params(w, h, 1, 8), g3)
        assert e.code == J2K_HIP_ERR_PARAM and "width" in str(e) and "height" in str(e) and "2^32" in str(e)
    # one sample fewer is a geometry like any other: the refusal is then the file's width
    e = refused(api.make_params(65536, 65535, 1, 8), g3)
    assert e.code == J2K_HIP_ERR_PARAM and "2^32" not in str(e)
    # 4:2:0: the chroma components are small enough, component 0 is not
    e = refused(api.make_params(65536, 65536, 3, 8, sub=[(1, 1), (2, 2), (2, 2)]), g3)
    assert e.code == J2K_HIP_ERR_PARAM and "2^32" in str(e)


def test_compare_check_keeps_read_infos_texts():
    g6 = load("g6_300x200_rgb16_97_ict")
    p = api.make_params(300, 200, 3, 16)
    api.compare_check(p, g6)
    for bad, code in ((g6[:60], J2K_HIP_ERR_PARAM), (_with_coc(g6, (1,), -1), J2K_HIP_ERR_UNSUPPORTED), (b"", J2K_HIP_ERR_PARAM)):
        e = refused(p, bad)
        assert e.code == code
        if bad:
            with pytest.raises(api.J2kHipError) as ei:
                api.read_info(bad)
            assert ei.value.code == code and str(ei.value) == str(e)
    assert "COC" in str(refused(p, _with_coc(g6, (1,), -1)))
    # the parameters' own refusals come first and keep the encoder's texts
    e = refused(api.make_params(300, 200, 5, 16), g6)
    assert e.code == J2K_HIP_ERR_PARAM and "channels" in str(e)
    e = refused(api.make_params(300, 200, 3, 8, sub=[(2, 1), (1, 1), (1, 1)]), g6)
    assert e.code == J2K_HIP_ERR_PARAM and "comp_sub_x" in str(e)


def test_the_model_on_hand_made_values():
    s = np.array([[10, 20, 30], [40, 50, 60]])
    d = np.array([[10, 23, 30], [36, 50, 60]])
    got = cm.diff(s, d, 8)
    assert got == dict(samples=6, differing=2, sum_abs=7, sum_sq=25, max_abs=4, first_x=1, first_y=0, mse=25 / 6,
                       psnr=10.0 * math.log10(255.0 * 255.0 / (25 / 6)))
    same = cm.diff(s, s, 8)
    assert same["psnr"] == math.inf and same["mse"] == 0.0 and (same["differing"], same["first_x"], same["first_y"], same["max_abs"]) == (0, 0, 0, 0)
    big = cm.diff(np.zeros((300, 300), np.int64), np.full((300, 300), 65535), 16)
    assert big["sum_sq"] == 90000 * 65535 ** 2 > 1 << 32 and big["sum_abs"] == 90000 * 65535 and big["psnr"] == 0.0
    # stored samples -> source samples: Promote on 16-bit samples only, the depth conversions, floats
    assert cm.source_samples(np.array([[255, 128]], np.uint8), 8, 12).tolist() == [[4095, 2056]]
    assert cm.source_samples(np.array([[65535, 32768]], np.uint16), 16, 10).tolist() == [[1023, 512]]
    assert cm.source_samples(np.array([[31, 16]], np.uint8), 5, 16).tolist() == [[65535, 33825]]
    assert cm.source_samples(np.array([[32768, 16384, 1]], np.uint16), 16, 16, promote=True).tolist() == [[65535, 32768, 2]]
    assert cm.source_samples(np.array([[200]], np.uint8), 8, 8, promote=True).tolist() == [[200]]
    assert cm.source_samples(np.array([[1.0, 0.5, -1.0, np.nan]], np.float32), 8, 8).tolist() == [[255, 128, 0, 0]]
    assert cm.own_grid(np.arange(12).reshape(3, 4), (2, 2)).tolist() == [[0, 2], [8, 10]]
