"""CPU: the code-block style parameter of the write side (j2k_hip_params.cblk_style) as far as it goes without a device --
the COD marker of the main header against libopenjp2's files, what is refused, and the fixtures against a live libopenjp2
where one is installed."""
import importlib.util
import json
import os

import pytest

import cblk_style_cases as cases
from j2k_amd import api

J2K_HIP_ERR_PARAM = 1


def _main_header_of(cs: bytes) -> bytes:
    return cs[:cs.index(b"\xff\x90")]  # SOC up to the first SOT


@pytest.mark.parametrize("name", cases.NAMES)
def test_main_header_carries_the_style(name):
    want = _main_header_of(cases.golden_bytes(name))
    got = api.main_header(cases.params(api, name))
    assert got == want
    cod = got.index(b"\xff\x52")
    assert got[cod + 12] == cases.entry(name)["ext"]["mode"]


@pytest.mark.parametrize("style, word", [(8, "vertically causal"), (64, "unknown"), (1 | 8, "vertically causal"), (128 | 1, "unknown")])
def test_styles_that_are_not_written_are_refused(style, word):
    with pytest.raises(api.J2kHipError) as ei:
        api.main_header(api.make_params(64, 64, 1, 8, cblk_style=style))
    assert ei.value.code == J2K_HIP_ERR_PARAM
    assert "cblk_style" in str(ei.value) and word in str(ei.value)


@pytest.mark.parametrize("style", [1, 4, 1 | 2 | 4 | 16 | 32])
@pytest.mark.parametrize("what, kw", [("layer_rates", dict(rates=[20.0, 5.0])), ("layer_psnr", dict(psnr=[35.0])), ("dci_profile", dict(dci_profile=3))])
def test_a_style_excludes_rate_control_and_cinema_profiles(style, what, kw):
    w, h, nc, prec = (512, 270, 3, 12) if what == "dci_profile" else (128, 128, 3, 8)
    with pytest.raises(api.J2kHipError) as ei:
        api.main_header(api.make_params(w, h, nc, prec, reversible=False, ycc=True, cblk_style=style, **kw))
    assert ei.value.code == J2K_HIP_ERR_PARAM
    assert "cblk_style" in str(ei.value) and what in str(ei.value)
    # the same parameters without the style are fine
    api.main_header(api.make_params(w, h, nc, prec, reversible=False, ycc=True, **kw))


def test_style_zero_writes_the_header_it_always_wrote(golden):
    g = golden["g9_97x61_grey12_97_4lvl"]
    with open(os.path.join(cases.GOLDEN_DIR, "g9_97x61_grey12_97_4lvl.j2k"), "rb") as f:
        want = _main_header_of(f.read())
    kw = dict(reversible=False, num_resolutions=g["params"]["numres"], comment="")
    assert api.main_header(api.make_params(97, 61, 1, 12, **kw)) == want
    assert api.main_header(api.make_params(97, 61, 1, 12, cblk_style=0, **kw)) == want


def test_fixtures_match_a_live_libopenjp2():
    from oracle.oracle import OpjReplay, find_openjpeg_libs
    try:
        if not find_openjpeg_libs():
            raise OSError("no libopenjp2 found")
        OpjReplay()
    except OSError as e:
        pytest.skip(f"libopenjp2 replay unavailable: {e}")
    spec = importlib.util.spec_from_file_location("make_style_golden", os.path.join(cases.GOLDEN_DIR, "make_style_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    meta, files = gen.generate()
    assert sorted(files) == sorted(cases.STYLES)
    for name, cs in files.items():
        assert cs == cases.golden_bytes(name), name
        assert json.loads(json.dumps(meta[name])) == cases.STYLES[name], name  # (tuples become lists on their way through JSON)
