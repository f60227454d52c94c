#!/usr/bin/env python3
"""Generate tests/golden/cut/cut.json: what libopenjp2 decodes from files cut short that the plain-C oracle does not read.

The cases are tests/cut_cases.py's for OPJ_FILES: the first k tile-parts of a committed fixture with an EOC appended -- the
only cuts libopenjp2 2.4.0 / 2.5.4 decode (a cut inside a tile-part they refuse).  Per case and reduce 0 and 1 the index holds
the shape and sha256 (of the int32 samples) of every component, from every libopenjp2 that oracle.find_openjpeg_libs()
returns; all libraries must agree.  It also records the tiles of which no tile-part is inside the cut: their samples must be
component value 0 in every component, which the maker asserts.

    python tests/golden/make_cut_golden.py            # (re)write the index
    python tests/golden/make_cut_golden.py --check    # compare with the committed index, write nothing
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cut_cases as cc  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "cut", "cut.json")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.int32).tobytes()).hexdigest()


def generate(*reps):
    """The index, from the libopenjp2 replays `reps` (default: every installed library)."""
    if not reps:
        from oracle.oracle import OpjReplay, find_openjpeg_libs
        reps = [OpjReplay(p) for p in find_openjpeg_libs()]
    assert reps, "no libopenjp2 installed"
    cases = {}
    for tag in cc.OPJ_FILES:
        w = cc.walk(cc.load(tag))
        for c in cc.cases(tag):
            data, decoded = cc.cut_bytes(c), {}
            for red in (0, 1):
                ds = [r.decode_comps(data, red) for r in reps]
                for d in ds[1:]:
                    assert all(np.array_equal(a["data"], b["data"]) for a, b in zip(ds[0], d)), (c["id"], red)
                for t in cc.missing_tiles(tag, c):
                    for comp in ds[0]:
                        x0, y0, x1, y1 = cc.tile_rect(w, t, red, (comp["dx"], comp["dy"]))
                        assert x1 > x0 and y1 > y0 and not comp["data"][y0:y1, x0:x1].any(), (c["id"], red, t)
                decoded[str(red)] = [dict(shape=list(comp["data"].shape), sha256=sha(comp["data"])) for comp in ds[0]]
            cases[c["id"]] = dict(file=cc.OPJ_FILES[tag], end=c["end"], missing_tiles=cc.missing_tiles(tag, c), decoded=decoded)
    return dict(note="libopenjp2's decode of the first `end` bytes of `file` plus an EOC; per reduce factor and component", cases=cases)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    index = generate()
    if args.check:
        with open(OUT) as f:
            assert json.load(f) == json.loads(json.dumps(index)), "the committed index differs"
        print("cut.json is up to date")
        return
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(index, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(index['cases'])} cases to {OUT}")


if __name__ == "__main__":
    main()
