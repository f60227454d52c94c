#!/usr/bin/env python3
"""Generate the damaged-file fixtures: tests/golden/damaged/<name>.j2k (clean) and damaged.json.

Six small files (tests/damaged_cases.py: FILES) written by libopenjp2 with SOP and EPH markers through oracle/opj_replay.c's
general encoder; all installed libraries must write the same bytes (COM segments stripped).  With both markers a packet
body -- code-block bytes and nothing else -- is what lies between a packet's EPH and the next SOP or the end of its
tile-part, so damage can be kept out of packet headers and lengths: the damaged file has the clean file's structure.

Per file and mode damaged.json holds the damage as DATA, a patch list [[offset, byte], ...] (no recipe that depends on a
library's random numbers), and libopenjp2's decode of the patched file: sha256 per component of its int32 samples at reduce
0 and 1.  All libraries must decode alike.  Modes: flip (single bits), marker (FF + a byte above 8F), ff_run (FF FF FF),
random (every body byte drawn anew).  A draw that writes a SOP's bytes into a body is drawn again.

    python tests/golden/make_damaged_golden.py            # (re)write the files
    python tests/golden/make_damaged_golden.py --check    # compare with the committed files, write nothing
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
import damaged_cases as dm  # noqa: E402
from j2k_amd import synth  # noqa: E402

OUT = dm.GOLDEN
PLACES = 12  # damaged places per file of the modes that have places


def sha(b):
    return hashlib.sha256(b).hexdigest()


def patch_list(cs, bodies, mode, seed):
    """[[offset, byte]] of one mode; the bytes that come out as they were are left out."""
    rng = np.random.default_rng(seed)
    inside = np.concatenate([np.arange(a, b) for a, b in bodies])
    new = bytearray(cs)
    if mode == "random":
        new_bytes = rng.integers(0, 256, size=len(inside), dtype=np.uint8)
        for off, b in zip(inside.tolist(), new_bytes.tolist()):
            new[off] = b
    else:
        width = {"flip": 1, "marker": 2, "ff_run": 3}[mode]
        # places spread over the bodies that are long enough, never across a body's end
        fits = [(a, b) for a, b in bodies if b - a >= width + 1]
        for k in range(PLACES):
            a, b = fits[(k * len(fits)) // PLACES]
            off = int(rng.integers(a, b - width + 1))
            if mode == "flip":
                new[off] ^= 1 << int(rng.integers(0, 8))
            elif mode == "marker":
                new[off:off + 2] = bytes([0xFF, dm.MARKER_BYTES[k % 3]])
            else:
                new[off:off + 3] = b"\xff\xff\xff"
    return [[i, new[i]] for i in range(len(cs)) if new[i] != cs[i]], bytes(new)


def generate():
    from oracle.oracle import OpjReplay, find_openjpeg_libs, strip_com
    reps = [OpjReplay(l) for l in find_openjpeg_libs()]
    meta = {"_generator": dict(libraries=[r.version for r in reps], note="COM segments stripped; sha256 of int32 samples per component")}
    files = {}

    def decoded(name, data):
        out = {}
        for reduce in (0, 1):
            decs = [r.decode_comps(data, reduce) for r in reps]
            for d in decs[1:]:
                assert all(np.array_equal(a["data"], b["data"]) for a, b in zip(decs[0], d)), (name, "the libraries decode differently")
            out[str(reduce)] = [sha(np.ascontiguousarray(c["data"], dtype=np.int32).tobytes()) for c in decs[0]]
        return out

    for k, (name, (w, h, nc, prec, seed, dist, kw)) in enumerate(dm.FILES.items()):
        pl = synth.planes(w, h, nc, prec, seed, dist)
        comps = [np.ascontiguousarray(pl[c]) for c in range(nc)]
        outs = [strip_com(r.encode_ext(comps, prec=prec, sop=True, eph=True, **kw)) for r in reps]
        assert all(o == outs[0] for o in outs[1:]), (name, "the libraries disagree")
        cs = outs[0]
        assert w <= 128 and h <= 64 and len(cs) <= 21000, (name, len(cs))
        bodies = dm.packet_bodies(cs)
        assert cs.count(dm.SOP) == len(bodies)
        modes = {}
        for j, mode in enumerate(dm.FILE_MODES):
            for attempt in range(100):
                patch, bad = patch_list(cs, bodies, mode, [4000 + k, j, attempt])
                if bad.count(dm.SOP) == cs.count(dm.SOP) and dm.packet_bodies(bad) == bodies:
                    break
            else:
                raise AssertionError((name, mode, "every draw wrote a SOP"))
            modes[mode] = dict(patch=patch, decoded=decoded(name + "/" + mode, bad))
            assert modes[mode]["decoded"]["0"] != decoded(name, cs)["0"], (name, mode, "the damage does not show")
        files[name] = cs
        meta[name] = dict(width=w, height=h, ncomp=nc, prec=prec, seed=seed, dist=dist, ext=dict(kw, sop=True, eph=True), length=len(cs),
                          sha256=sha(cs), body_bytes=sum(b - a for a, b in bodies), decoded=decoded(name, cs), modes=modes)
        print(name, len(cs), "bytes,", len(bodies), "packets,", {m: len(v["patch"]) for m, v in modes.items()})
    return meta, files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed files instead of writing them")
    args = ap.parse_args()
    meta, files = generate()
    index = os.path.join(OUT, "damaged.json")
    if args.check:
        assert json.load(open(index)) == json.loads(json.dumps(meta)), "damaged.json differs"
        for name, cs in files.items():
            assert open(os.path.join(OUT, name + ".j2k"), "rb").read() == cs, name
        print("all", len(files), "files match")
        return
    os.makedirs(OUT, exist_ok=True)
    for name, cs in files.items():
        with open(os.path.join(OUT, name + ".j2k"), "wb") as f:
            f.write(cs)
    with open(index, "w") as f:
        json.dump(meta, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
