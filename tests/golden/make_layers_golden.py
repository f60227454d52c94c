#!/usr/bin/env python3
"""Generate the quality-layer fixtures: tests/golden/layers/<name>.j2k and layers.json.

Inputs come from the seeded generator in j2k_amd/synth.py; the files come from every libopenjp2 that
oracle.find_openjpeg_libs() returns, driven through oracle/opj_replay.c's general encoder with SOP markers and one
compression ratio per layer (tests/layers_cases.py: CASES).  All libraries must write the same bytes, COM stripped.

For every L in 1..layers and reduce 0 and 1, layers.json holds the per-component shape and sha256 of the decode of
strip(cs, L) -- the file cut down to its first L layers (tests/layers_cases.py) -- which is what a decode of the whole
file with the layer limit L has to deliver.  The plain-C oracle gives the samples where it reads the file, libopenjp2's
decode_comps otherwise; where both read it they must agree, and so must all libraries.

The maker also asserts what makes the fixtures prove something (tests/test_decode_layers_refs.py repeats it):
the decodes at L = 1..layers differ pairwise; somewhere the number of blocks with passes grows with L (a block first
included in a later layer); the absolute error against the source never rises with L and is 0 at L = layers where the
last ratio is 0 and the wavelet is 5/3; and in the bypass file some block ends inside a raw segment at some L.

    python tests/golden/make_layers_golden.py            # (re)write the files
    python tests/golden/make_layers_golden.py --check    # compare with the committed files, write nothing
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
from j2k_amd import synth  # noqa: E402
import layers_cases as lc  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "layers")


def sha(b):
    return hashlib.sha256(b).hexdigest()


def source_comps(name):
    w, h, nc, prec, seed, dist, kw = lc.CASES[name]
    pl = synth.planes(w, h, nc, prec, seed, dist)
    sub = kw.get("sub", [(1, 1)] * nc)
    return [np.ascontiguousarray(pl[c][::sub[c][1], ::sub[c][0]]) for c in range(nc)]


def oracle_blocks(oracle, data):
    """The oracle's Tier-2 of a file, or None where it does not read it."""
    try:
        return oracle.file_blocks(data)["blocks"]
    except RuntimeError:
        return None


def reference_decode(oracle, reps, data, red, name):
    """Per-component samples of `data` at resolution `red`: every library, and the oracle where it reads the file."""
    ds = [r.decode_comps(data, red) for r in reps]
    for d in ds[1:]:
        assert all(np.array_equal(a["data"], b["data"]) for a, b in zip(ds[0], d)), (name, red, "the libraries decode differently")
    oracle_reads = all(c["dx"] == 1 and c["dy"] == 1 for c in ds[0])
    if oracle_reads:
        try:
            own = oracle.decode(data, red)
        except RuntimeError:
            oracle_reads = False
    if oracle_reads:
        assert all(np.array_equal(own[c], d["data"]) for c, d in enumerate(ds[0])), (name, red, "the oracle and libopenjp2 disagree")
    return ds[0], oracle_reads


def check_conditions(name, comps, decs, nblocks, passes):
    """decs[L - 1] = component samples of strip(cs, L) at full size; nblocks / passes: per L, from the oracle (None: not read)."""
    kw = lc.CASES[name][6]
    n = len(decs)
    for a in range(n):
        for b in range(a + 1, n):
            assert any(not np.array_equal(x, y) for x, y in zip(decs[a], decs[b])), (name, "layers", a + 1, b + 1, "decode alike")
    err = [sum(int(np.abs(d.astype(np.int64) - s).sum()) for d, s in zip(dec, comps)) for dec in decs]
    assert all(e1 <= e0 for e0, e1 in zip(err, err[1:])), (name, "the error rises with L", err)
    if kw.get("reversible", True) and kw["rates"][-1] == 0.0:
        assert err[-1] == 0, (name, "not lossless at the last layer")
    if nblocks[0] is not None:
        assert all(b1 >= b0 for b0, b1 in zip(nblocks, nblocks[1:])), (name, nblocks)
    if kw.get("mode", 0) == 1:  # bypass: ten MQ passes, then (raw significance, raw refinement), (MQ cleanup) in turn
        assert any(p > 10 and (p - 10) % 3 == 1 for per_l in passes[:-1] for p in per_l), (name, "no block ends inside a raw segment")
    return err


def generate():
    from oracle.oracle import OpjReplay, Oracle, find_openjpeg_libs, strip_com
    reps = [OpjReplay(l) for l in find_openjpeg_libs()]
    oracle = Oracle()
    meta = {"_generator": dict(libraries=[r.version for r in reps], note="COM segments stripped before hashing/storing")}
    files = {}
    grows = False
    for name, (w, h, nc, prec, seed, dist, kw) in lc.CASES.items():
        comps = source_comps(name)
        outs = [strip_com(r.encode_ext(comps, x1=w, y1=h, prec=prec, sop=True, **kw)) for r in reps]
        assert all(o == outs[0] for o in outs[1:]), (name, "the libraries disagree")
        cs = outs[0]
        layers = lc.layers_of(name)
        assert all(n % layers == 0 for n in lc.packets_per_tile_part(cs)), name
        assert lc.strip(cs, layers) == cs, name
        decoded, decs, nblocks, passes, oracle_reads = {}, [], [], [], True
        for L in range(1, layers + 1):
            cut = lc.strip(cs, L)
            per_red = {}
            for red in (0, 1):
                d, reads = reference_decode(oracle, reps, cut, red, name)
                oracle_reads = oracle_reads and reads
                per_red[str(red)] = [dict(shape=list(c["data"].shape), sha256=sha(c["data"].tobytes()), prec=c["prec"], dx=c["dx"], dy=c["dy"]) for c in d]
                if red == 0:
                    decs.append([c["data"] for c in d])
            decoded[str(L)] = per_red
            blocks = oracle_blocks(oracle, cut)
            nblocks.append(None if blocks is None else len(blocks))
            passes.append([] if blocks is None else [b["npasses"] for b in blocks])
        err = check_conditions(name, comps, decs, nblocks, passes)
        grows = grows or (nblocks[0] is not None and nblocks[-1] > nblocks[0])
        files[name] = cs
        meta[name] = dict(width=w, height=h, ncomp=nc, prec=prec, seed=seed, dist=dist, ext=kw, layers=layers, length=len(cs), sha256=sha(cs),
                          decoded=decoded, oracle_reads=oracle_reads, blocks_with_passes=nblocks,
                          passes=[None if b is None else sum(p) for b, p in zip(nblocks, passes)], abs_error=err)
        print(name, len(cs), "blocks", nblocks, "error", err, "oracle" if oracle_reads else "libopenjp2 only")
    assert grows, "no fixture has a block first included in a later layer"
    return meta, files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed files instead of writing them")
    args = ap.parse_args()
    meta, files = generate()
    if args.check:
        committed = json.load(open(os.path.join(OUT, "layers.json")))
        assert committed == json.loads(json.dumps(meta)), "layers.json differs"
        for name, cs in files.items():
            assert open(os.path.join(OUT, name + ".j2k"), "rb").read() == cs, name
        print("all", len(files), "files match")
        return
    os.makedirs(OUT, exist_ok=True)
    for name, cs in files.items():
        with open(os.path.join(OUT, name + ".j2k"), "wb") as f:
            f.write(cs)
    with open(os.path.join(OUT, "layers.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
