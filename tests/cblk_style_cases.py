"""The encoder goldens of the code-block styles, shared by test_cblk_style_host.py (CPU) and test_cblk_style.py (GPU):
tests/golden/styles/ (make_style_golden.py) and the four files of tests/golden/ext/ that the write side can produce too."""
import json
import os

from j2k_amd import synth

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

EXT_AS_ENCODER_GOLDENS = ["s1_300x200_rgb16_53_bypass", "s3_200x150_grey12_53_termall_pterm",
                          "s5_257x131_rgb10_53_bypass_termall_cblk32_rpcl", "u7_128_grey8_53_bypass_termall"]

with open(os.path.join(GOLDEN_DIR, "styles", "styles.json")) as _f:
    STYLES = {k: v for k, v in json.load(_f).items() if not k.startswith("_")}
with open(os.path.join(GOLDEN_DIR, "golden.json")) as _f:
    _g = json.load(_f)
    EXT = {k: _g[k] for k in EXT_AS_ENCODER_GOLDENS}

NAMES = sorted(STYLES) + EXT_AS_ENCODER_GOLDENS
# the other entry points are held to the same bytes for these: bypass alone, all five styles, the tiled case
ENTRY_POINT_NAMES = ["y1_97x61_grey16_53_bypass", "ya_200x150_rgb16_97_all_five_cblk32", "y9_150x130_rgb10_53_bypass_reset_segsym_tile64_rpcl"]
TILED_NAME = "y9_150x130_rgb10_53_bypass_reset_segsym_tile64_rpcl"


def entry(name):
    return STYLES[name] if name in STYLES else EXT[name]


def golden_bytes(name):
    sub = "styles" if name in STYLES else "ext"
    with open(os.path.join(GOLDEN_DIR, sub, name + ".j2k"), "rb") as f:
        return f.read()


def planes(name, seed_offset=0):
    g = entry(name)
    return synth.planes(g["width"], g["height"], g["ncomp"], g["prec"], g["seed"] + seed_offset, g["dist"])


def params(api, name, **override):
    """j2k_hip_params for the fixture's encode_ext kwargs (no COM: the fixtures are stored without theirs)."""
    g = entry(name)
    kw = g["ext"]
    tile = kw.get("tile", (0, 0))
    assert tile[0] == tile[1]
    args = dict(reversible=kw.get("reversible", True), ycc=kw.get("mct", False), layers=kw.get("layers", 1), tile_size=tile[0],
                num_resolutions=kw["numres"], cblk=tuple(kw.get("cblk", (64, 64))), comment="", progression=kw.get("prog", 0),
                precincts=[tuple(p) for p in kw["precincts"]] if kw.get("precincts") else None, cblk_style=kw["mode"])
    args.update(override)
    return api.make_params(g["width"], g["height"], g["ncomp"], g["prec"], **args)


def decoded_hashes(name):
    """sha256 of every component's int32 samples as libopenjp2 decodes the fixture."""
    g = entry(name)
    dc = g["decoded_comps"]
    return [c["sha256"] for c in (dc["0"] if isinstance(dc, dict) else dc)]
