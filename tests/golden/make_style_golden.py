#!/usr/bin/env python3
"""Generate the encoder goldens of the code-block styles: tests/golden/styles/<name>.j2k and styles.json.

Inputs come from the seeded generator in j2k_amd/synth.py; expected outputs come from every libopenjp2 that
oracle.find_openjpeg_libs() returns, driven through oracle/opj_replay.c's general encoder (cparameters.mode = the COD
SPcod code-block style byte: 1 bypass, 2 reset, 4 termall, 16 pterm, 32 segsym).  All libraries must write the same
bytes.  COM marker segments are stripped (they embed the library version).  Every case is also encoded with style 0
from the same input, and the styled file must differ from that one in more than the style byte of COD: the style
provably took effect in the fixture.

    python tests/golden/make_style_golden.py            # (re)write the files
    python tests/golden/make_style_golden.py --check    # compare with the committed files, write nothing
    python tests/golden/make_style_golden.py --dec [--check]

--dec: the decode-only fixtures tests/golden/styles_dec/<name>.j2k and styles_dec.json instead -- files with vertically
causal contexts (style bit 8), which libopenjp2 writes and this project only reads.  They stay out of styles.json, whose
every entry the encoder tests write; odd sizes, so that blocks are partial in both directions and a stripe is short.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from j2k_amd import synth  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "styles")

# name -> (width, height, ncomp, prec, seed, dist, encode_ext kwargs)
STYLES = {
    "y1_97x61_grey16_53_bypass": (97, 61, 1, 16, 201, "A", dict(numres=3, mode=1)),
    "y2_64x64_grey16_53_1res_bypass": (64, 64, 1, 16, 202, "B", dict(numres=1, mode=1)),
    "y3_97x61_grey12_53_reset": (97, 61, 1, 12, 203, "B", dict(numres=3, mode=2)),
    "y4_97x61_grey12_97_termall": (97, 61, 1, 12, 204, "A", dict(numres=3, mode=4, reversible=False)),
    "y5_97x61_grey12_53_pterm": (97, 61, 1, 12, 205, "A", dict(numres=3, mode=16)),
    "y6_97x61_grey12_97_segsym": (97, 61, 1, 12, 206, "B", dict(numres=3, mode=32, reversible=False)),
    "y7_128_grey16_53_bypass_termall": (128, 128, 1, 16, 207, "A", dict(numres=2, mode=1 | 4)),
    "y8_128_grey16_53_bypass_pterm_3layers": (128, 128, 1, 16, 208, "B", dict(numres=2, mode=1 | 16, layers=3)),
    "y9_150x130_rgb10_53_bypass_reset_segsym_tile64_rpcl": (150, 130, 3, 10, 209, "B", dict(numres=3, mct=True, mode=1 | 2 | 32, tile=(64, 64), prog=2,
                                                                                             precincts=[(32, 32)])),
    "ya_200x150_rgb16_97_all_five_cblk32": (200, 150, 3, 16, 210, "A", dict(numres=4, mct=True, mode=55, cblk=(32, 32), reversible=False)),
    "yb_17x9_grey16_53_all_five": (17, 9, 1, 16, 211, "A", dict(numres=2, mode=55)),
    "yc_65x33_rgba8_53_bypass_termall": (65, 33, 4, 8, 212, "B", dict(numres=2, mct=True, mode=1 | 4)),
}

# the decode-only fixtures (--dec): every one has the vertically causal bit
STYLES_DEC = {
    "z1_97x61_grey16_53_vcausal": (97, 61, 1, 16, 221, "A", dict(numres=3, mode=8)),
    "z2_97x61_grey12_97_vcausal_bypass_termall": (97, 61, 1, 12, 222, "B", dict(numres=3, mode=8 | 1 | 4, reversible=False)),
    "z3_17x9_grey16_53_all_six": (17, 9, 1, 16, 223, "A", dict(numres=2, mode=63)),
    "z4_65x33_rgb8_53_vcausal_reset_segsym_cblk32": (65, 33, 3, 8, 224, "B", dict(numres=2, mct=True, mode=8 | 2 | 32, cblk=(32, 32))),
    "z5_128_grey16_53_vcausal_bypass_3layers": (128, 128, 1, 16, 225, "B", dict(numres=2, mode=8 | 1, layers=3)),
}


def sha(b):
    return hashlib.sha256(b).hexdigest()


def differs_beyond_cod_style(styled: bytes, plain: bytes) -> bool:
    """True when the two codestreams differ somewhere else than in SPcod's code-block style byte."""
    cod = styled.index(b"\xff\x52")
    style_at = cod + 12  # marker 2, Lcod 2, Scod 1, SGcod 4, levels 1, cblk w/h 2: then the style
    if len(styled) != len(plain):
        return True
    return any(a != b for i, (a, b) in enumerate(zip(styled, plain)) if i != style_at)


def generate(table=None):
    table = STYLES if table is None else table
    from oracle.oracle import OpjReplay, find_openjpeg_libs, strip_com
    reps = [OpjReplay(l) for l in find_openjpeg_libs()]
    meta = {"_generator": dict(libraries=[r.version for r in reps], note="COM segments stripped before hashing/storing")}
    files = {}
    for name, (w, h, nc, prec, seed, dist, kw) in table.items():
        pl = synth.planes(w, h, nc, prec, seed, dist)
        comps = [np.ascontiguousarray(pl[c]) for c in range(nc)]
        outs = [strip_com(r.encode_ext(comps, prec=prec, **kw)) for r in reps]
        assert all(o == outs[0] for o in outs[1:]), (name, "the libraries disagree")
        cs = outs[0]
        plain = strip_com(reps[0].encode_ext(comps, prec=prec, **dict(kw, mode=0)))
        assert differs_beyond_cod_style(cs, plain), (name, "the style changed nothing but the COD byte")
        decs = [r.decode_comps(cs, 0) for r in reps]
        for d in decs[1:]:
            assert all(np.array_equal(a["data"], b["data"]) for a, b in zip(decs[0], d)), (name, "the libraries decode differently")
        if kw.get("reversible", True):
            assert all(np.array_equal(a, b["data"]) for a, b in zip(comps, decs[0])), (name, "not lossless")
        files[name] = cs
        meta[name] = dict(width=w, height=h, ncomp=nc, prec=prec, seed=seed, dist=dist, ext=kw, length=len(cs), sha256=sha(cs),
                          decoded_comps=[dict(shape=list(c["data"].shape), sha256=sha(c["data"].tobytes())) for c in decs[0]])
        print(name, len(cs), "style 0:", len(plain))
    return meta, files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed files instead of writing them")
    ap.add_argument("--dec", action="store_true", help="the decode-only fixtures (tests/golden/styles_dec) instead")
    args = ap.parse_args()
    out_dir, index = (os.path.join(HERE, "styles_dec"), "styles_dec.json") if args.dec else (OUT, "styles.json")
    meta, files = generate(STYLES_DEC if args.dec else STYLES)
    if args.check:
        committed = json.load(open(os.path.join(out_dir, index)))
        assert committed == json.loads(json.dumps(meta)), index + " differs"
        for name, cs in files.items():
            assert open(os.path.join(out_dir, name + ".j2k"), "rb").read() == cs, name
        print("all", len(files), "files match")
        return
    os.makedirs(out_dir, exist_ok=True)
    for name, cs in files.items():
        with open(os.path.join(out_dir, name + ".j2k"), "wb") as f:
            f.write(cs)
    with open(os.path.join(out_dir, index), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
