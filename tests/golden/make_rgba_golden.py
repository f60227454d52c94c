"""Writes the fixtures of the RGBA tests into tests/golden/rgba/: four small sYCC files with sub-sampled chroma, made by a real
libopenjp2 (OpjReplay.encode_ext) and wrapped into JP2 with colour space sYCC (Oracle.jp2_wrap), and rgba.json -- for every
case of tests/rgba_cases.py the SHA-256 of the expected frame, rgba_model applied to libopenjp2's own component samples.

    python tests/golden/make_rgba_golden.py            (needs libopenjp2; no device)

The files are written only where they are missing (an encoder of another version would change their bytes); rgba.json is
always rewritten."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import rgba_cases as rc  # noqa: E402
from j2k_amd import synth  # noqa: E402
from oracle.oracle import OpjReplay, Oracle, make_params  # noqa: E402

# name -> (width, height, chroma sub-sampling, precision, reversible, resolutions, image origin, tile)
SPECS = {
    "k1": (37, 21, (2, 2), 8, True, 3, (0, 0), (0, 0)),
    "k2": (65, 33, (2, 1), 10, False, 4, (0, 0), (0, 0)),
    "k3": (41, 23, (2, 2), 8, True, 3, (3, 1), (0, 0)),
    "k4": (130, 70, (2, 2), 8, True, 3, (0, 0), (64, 64)),
}


def make_file(opj, orc, name):
    w, h, sub, prec, rev, numres, (x0, y0), tile = SPECS[name]
    subs = [(1, 1), sub, sub]
    comps = []
    for c, (dx, dy) in enumerate(subs):  # a component's grid: ceil(x1 / dx) - ceil(x0 / dx) columns
        cw = -(-(x0 + w) // dx) - -(-x0 // dx)
        ch = -(-(y0 + h) // dy) - -(-y0 // dy)
        comps.append(synth.planes(cw, ch, 1, prec, 100 * (ord(name[1]) - 48) + c, "A")[0])
    cs = opj.encode_ext(comps, x0=x0, y0=y0, x1=x0 + w, y1=y0 + h, sub=subs, prec=prec, reversible=rev, mct=False, numres=numres, tile=tile)
    return orc.jp2_wrap(cs, make_params(w, h, 3, prec), color_space=3)


def main():
    opj, orc = OpjReplay(), Oracle()
    os.makedirs(os.path.join(rc.GOLDEN_DIR, "rgba"), exist_ok=True)
    for name in SPECS:
        path = os.path.join(rc.GOLDEN_DIR, rc.FILES[name])
        if not os.path.exists(path):
            data = make_file(opj, orc, name)
            with open(path, "wb") as f:
                f.write(data)
            print("wrote", path, len(data), "bytes")
    table = {c["id"]: rc.sha(rc.expected_from_opj(opj, c)) for c in rc.cases()}
    with open(os.path.join(rc.GOLDEN_DIR, "rgba", "rgba.json"), "w") as f:
        json.dump(dict(libopenjp2=opj.version, cases=table), f, indent=1, sort_keys=True)
        f.write("\n")
    print(len(table), "cases")


if __name__ == "__main__":
    main()
