#!/usr/bin/env python3
"""Generate the encoder goldens of sub-sampled components: tests/golden/subsample/<name>.j2k and subsample.json.

Inputs come from the seeded generator in j2k_amd/synth.py: synth.planes(w, h, ncomp, prec, seed, dist), component c being the
top-left ceil(h / dy) x ceil(w / dx) crop of its plane.  Expected outputs come from every libopenjp2 that
oracle.find_openjpeg_libs() returns, driven through oracle/opj_replay.c's general encoder with per-component dx, dy.  All
libraries must write the same bytes.  COM marker segments are stripped (they embed the library version); where a byte budget
applies, the length of the libraries' comment is recorded, because the budget takes the main header -- COM included -- off.

Asserted here: every 5/3 case decodes back to its input; a case with rates is at most 60 % of the same encode without rates
(unless its last layer is "the rest"); every file's SIZ carries the factors.

    python tests/golden/make_subsample_golden.py            # (re)write the files
    python tests/golden/make_subsample_golden.py --check    # compare with the committed files, write nothing
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
OUT = os.path.join(HERE, "subsample")

S422, S420, S411 = [(1, 1), (2, 1), (2, 1)], [(1, 1), (2, 2), (2, 2)], [(1, 1), (4, 1), (4, 1)]

# name -> (width, height, sub, prec, seed, dist, encode_ext kwargs)
CASES = {
    "q1_97x61_422_8_53": (97, 61, S422, 8, 301, "A", dict(numres=3)),
    "q2_97x61_420_10_97_4res": (97, 61, S420, 10, 302, "B", dict(numres=4, reversible=False)),
    "q3_131x67_420_alpha_8_53_rpcl": (131, 67, S420 + [(1, 1)], 8, 303, "B", dict(numres=3, prog=2)),
    "q4_150x130_422_12_53_pcrl_tile64": (150, 130, S422, 12, 304, "A", dict(numres=3, prog=3, tile=(64, 64))),
    "q5_131x67_422_8_97_cprl_precincts": (131, 67, S422, 8, 305, "A", dict(numres=3, prog=4, reversible=False, precincts=[(32, 32), (16, 16)])),
    "q6_128_422_8_97_rates_80_20": (128, 128, S422, 8, 306, "B", dict(numres=3, reversible=False, rates=[80, 20])),
    "q7_97x61_411_16_53": (97, 61, S411, 16, 307, "A", dict(numres=3)),
    "q8_17x9_420_8_53_2res": (17, 9, S420, 8, 308, "A", dict(numres=2)),
    "q9_200x150_420_8_97_rpcl_tile128_rates_80_30_12": (200, 150, S420, 8, 309, "A", dict(numres=4, reversible=False, prog=2, tile=(128, 128), rates=[80, 30, 12])),
    "qa_65x33_422_8_53_bypass_termall": (65, 33, S422, 8, 310, "B", dict(numres=2, mode=1 | 4)),
    "qb_3x3_420_8_53_1res": (3, 3, S420, 8, 311, "A", dict(numres=1)),
    "qc_130x70_mixed_2x1_1x2_8_53_rpcl": (130, 70, [(1, 1), (2, 1), (1, 2)], 8, 312, "A", dict(numres=3, prog=2)),
    "qd_150x130_411_8_53_rpcl_tile50": (150, 130, S411, 8, 313, "A", dict(numres=3, prog=2, tile=(50, 50))),
    "qe_150x130_420_8_97_cprl_tile50": (150, 130, S420, 8, 314, "B", dict(numres=3, prog=4, tile=(50, 50), reversible=False)),
    "qf_1x1_420_8_53_1res": (1, 1, S420, 8, 315, "A", dict(numres=1)),
    "qg_1x37_422_8_53_1res": (1, 37, S422, 8, 316, "A", dict(numres=1)),
    "qj_128_420_8_53_rates_30_8_0": (128, 128, S420, 8, 317, "B", dict(numres=3, rates=[30, 8, 0])),
}


def sha(b):
    return hashlib.sha256(b).hexdigest()


def components(w, h, sub, prec, seed, dist):
    """Component c = the top-left ceil(h / dy) x ceil(w / dx) crop of plane c of the seeded image."""
    pl = synth.planes(w, h, len(sub), prec, seed, dist)
    return [np.ascontiguousarray(pl[c][:-(-h // dy), :-(-w // dx)]) for c, (dx, dy) in enumerate(sub)]


def siz_factors(cs: bytes):
    siz = cs.index(b"\xff\x51")
    nc = int.from_bytes(cs[siz + 38:siz + 40], "big")
    return [(cs[siz + 40 + 3 * c + 1], cs[siz + 40 + 3 * c + 2]) for c in range(nc)]


def generate(table=None):
    table = CASES if table is None else table
    from oracle.oracle import OpjReplay, find_openjpeg_libs, strip_com
    reps = [OpjReplay(l) for l in find_openjpeg_libs()]
    meta = {"_generator": dict(libraries=[r.version for r in reps], note="COM segments stripped before hashing/storing")}
    files = {}
    # (a byte budget takes the main header off, COM included: the test gives its own encode a comment of this length)
    com = len(reps[0].comment)
    assert all(len(r.comment) == com for r in reps), "the libraries' COM segments differ in length"
    for name, (w, h, sub, prec, seed, dist, kw) in table.items():
        comps = components(w, h, sub, prec, seed, dist)
        outs = [strip_com(r.encode_ext(comps, x1=w, y1=h, sub=sub, prec=prec, **kw)) for r in reps]
        assert all(o == outs[0] for o in outs[1:]), (name, "the libraries disagree")
        cs = outs[0]
        assert siz_factors(cs) == [tuple(s) for s in sub], (name, "SIZ does not carry the factors")
        norates = None
        if kw.get("rates"):
            norates = len(strip_com(reps[0].encode_ext(comps, x1=w, y1=h, sub=sub, prec=prec, **{k: v for k, v in kw.items() if k != "rates"})))
            if kw["rates"][-1] > 1:
                assert len(cs) <= 0.6 * norates, (name, "the byte budget does not bind", len(cs), norates)
        decs = [r.decode_comps(cs, 0) for r in reps]
        for d in decs[1:]:
            assert all(np.array_equal(a["data"], b["data"]) for a, b in zip(decs[0], d)), (name, "the libraries decode differently")
        assert [(d["dx"], d["dy"]) for d in decs[0]] == [tuple(s) for s in sub], name
        if kw.get("reversible", True) and not (kw.get("rates") and kw["rates"][-1] > 1):
            assert all(np.array_equal(a, b["data"]) for a, b in zip(comps, decs[0])), (name, "not lossless")
        files[name] = cs
        meta[name] = dict(width=w, height=h, sub=sub, prec=prec, seed=seed, dist=dist, ext=kw, length=len(cs), sha256=sha(cs),
                          length_without_rates=norates, comment_length=com if kw.get("rates") else None,
                          decoded_comps=[dict(shape=list(c["data"].shape), sha256=sha(c["data"].tobytes())) for c in decs[0]])
        print(name, len(cs), "" if norates is None else f"without rates: {norates}")
    return meta, files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed files instead of writing them")
    args = ap.parse_args()
    meta, files = generate()
    index = "subsample.json"
    if args.check:
        committed = json.load(open(os.path.join(OUT, index)))
        assert committed == json.loads(json.dumps(meta)), index + " differs"
        for name, cs in files.items():
            assert open(os.path.join(OUT, name + ".j2k"), "rb").read() == cs, name
        print("all", len(files), "files match")
        return
    os.makedirs(OUT, exist_ok=True)
    for name, cs in files.items():
        with open(os.path.join(OUT, name + ".j2k"), "wb") as f:
            f.write(cs)
    with open(os.path.join(OUT, index), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
