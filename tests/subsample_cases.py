"""The encoder goldens of sub-sampled components (tests/golden/subsample/, make_subsample_golden.py), shared by
test_subsample_host.py (CPU) and test_subsample.py (GPU)."""
import json
import os

import numpy as np

from j2k_amd import synth

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

with open(os.path.join(GOLDEN_DIR, "subsample", "subsample.json")) as _f:
    CASES = {k: v for k, v in json.load(_f).items() if not k.startswith("_")}

NAMES = sorted(CASES)


def by_prefix(p):
    (name,) = [n for n in NAMES if n.startswith(p + "_")]
    return name


# held to the same bytes through every entry point: plain 4:2:2, CPRL with precincts on 9/7, tiles + RPCL + a byte budget
ENTRY_POINT_NAMES = [by_prefix("q1"), by_prefix("q5"), by_prefix("q9")]
TRANSFORM_NAMES = [by_prefix("q2"), by_prefix("q3"), by_prefix("qd")]


def entry(name):
    return CASES[name]


def golden_bytes(name):
    with open(os.path.join(GOLDEN_DIR, "subsample", name + ".j2k"), "rb") as f:
        return f.read()


def subs(name):
    return [tuple(s) for s in CASES[name]["sub"]]


def components(name, seed_offset=0):
    """Component c = the top-left ceil(h / dy) x ceil(w / dx) crop of plane c of the seeded image (the generator's rule)."""
    g = CASES[name]
    w, h = g["width"], g["height"]
    pl = synth.planes(w, h, len(g["sub"]), g["prec"], g["seed"] + seed_offset, g["dist"])
    return [np.ascontiguousarray(pl[c][:-(-h // dy), :-(-w // dx)]) for c, (dx, dy) in enumerate(subs(name))]


def params(api, name, **override):
    """j2k_hip_params for the fixture's encode_ext kwargs (no COM: the fixtures are stored without theirs)."""
    g = CASES[name]
    kw = g["ext"]
    tile = kw.get("tile", (0, 0))
    assert tile[0] == tile[1]
    args = dict(reversible=kw.get("reversible", True), layers=kw.get("layers", 1), tile_size=tile[0], num_resolutions=kw["numres"],
                comment="", progression=kw.get("prog", 0), precincts=[tuple(p) for p in kw["precincts"]] if kw.get("precincts") else None,
                cblk_style=kw.get("mode", 0), rates=[float(r) for r in kw["rates"]] if kw.get("rates") else None, sub=subs(name))
    if g.get("comment_length"):  # a byte budget takes the main header, COM included, off: a comment as long as libopenjp2's
        args["comment"] = "x" * g["comment_length"]
    args.update(override)
    return api.make_params(g["width"], g["height"], len(g["sub"]), g["prec"], **args)


def strip_com(cs: bytes) -> bytes:
    """Without the COM marker segments of the main header, as the fixtures are stored."""
    out, i = bytearray(cs[:2]), 2
    while i < len(cs):
        if cs[i:i + 2] == b"\xff\x90":
            out += cs[i:]
            break
        ln = int.from_bytes(cs[i + 2:i + 4], "big")
        if cs[i:i + 2] != b"\xff\x64":
            out += cs[i:i + 2 + ln]
        i += 2 + ln
    return bytes(out)


def decoded_hashes(name):
    """sha256 of every component's int32 samples as libopenjp2 decodes the fixture."""
    return [c["sha256"] for c in CASES[name]["decoded_comps"]]


def main_header_of(cs: bytes) -> bytes:
    return cs[:cs.index(b"\xff\x90")]  # SOC up to the first SOT
