"""The reference of a decode with a layer limit, checked without a device: the stripper of tests/layers_cases.py, the committed
hashes of tests/golden/layers/layers.json against the plain-C oracle, the generator against the committed files, the
conditions that make the fixtures prove something -- and the planner itself: plan_decode(file, ..., L) against
plan_decode(strip(file, L)) block for block, as a stand-alone program under ASan + UBSan (tests/native/decode_layers_host.cpp)."""
import hashlib
import importlib.util
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN_DIR, ROOT
from j2k_amd import api, synth

import layers_cases as lc


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def source_comps(name):
    w, h, nc, prec, seed, dist, kw = lc.CASES[name]
    pl = synth.planes(w, h, nc, prec, seed, dist)
    sub = kw.get("sub", [(1, 1)] * nc)
    return [pl[c][::sub[c][1], ::sub[c][0]] for c in range(nc)]


@pytest.mark.parametrize("name", lc.NAMES)
def test_stripper_self_checks(name):
    cs, layers = lc.load(name), lc.layers_of(name)
    m = lc.meta()[name]
    assert hashlib.sha256(cs).hexdigest() == m["sha256"] and m["layers"] == layers
    assert api.read_info(cs)["layers"] == layers
    assert all(n and n % layers == 0 for n in lc.packets_per_tile_part(cs))
    assert lc.strip(cs, layers) == cs
    sizes = []
    for L in range(1, layers + 1):
        cut = lc.strip(cs, L)
        assert api.read_info(cut)["layers"] == L
        assert [n * layers for n in lc.packets_per_tile_part(cut)] == [n * L for n in lc.packets_per_tile_part(cs)]
        sizes.append(len(cut))
        bare = lc.drop_sop(cut)
        assert api.read_info(bare)["layers"] == L and lc.SOP not in bare
        assert len(cut) - len(bare) == 6 * sum(lc.packets_per_tile_part(cut))
    assert sizes == sorted(set(sizes)) and sizes[-1] == len(cs)


@pytest.mark.parametrize("name", [n for n in lc.NAMES if lc.meta()[n]["oracle_reads"]])
def test_committed_hashes_against_the_oracle(oracle, name):
    cs = lc.load(name)
    for L in range(1, lc.layers_of(name) + 1):
        for red in (0, 1):
            dec = oracle.decode(lc.strip(cs, L), red)
            want = lc.meta()[name]["decoded"][str(L)][str(red)]
            assert len(want) == dec.shape[0]
            for c, exp in enumerate(want):
                assert list(dec[c].shape) == exp["shape"] and sha(dec[c]) == exp["sha256"], (name, L, red, c)
            # the SOP segments carry nothing the samples depend on
            if red == 0:
                assert np.array_equal(oracle.decode(lc.drop_sop(lc.strip(cs, L)), 0), dec)


def test_generator_reproduces_the_committed_files(opj):
    """With a live libopenjp2: the maker writes the committed files and index again (it asserts the conditions below itself)."""
    spec = importlib.util.spec_from_file_location("make_layers_golden", os.path.join(GOLDEN_DIR, "make_layers_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    meta, files = gen.generate()
    assert sorted(files) == sorted(lc.NAMES)
    for name, cs in files.items():
        assert cs == lc.load(name), name
        assert json.loads(json.dumps(meta[name])) == lc.meta()[name], name


def test_fixture_conditions(oracle):
    """What makes the fixtures prove something: the decodes at L = 1..layers differ pairwise; somewhere a block is first included
    in a later layer; the error against the source never rises with L and is 0 at the last layer of a lossless file; in the
    bypass file a block ends inside a raw segment (its significance pass kept without its refinement pass)."""
    grows, partial_raw = False, 0
    try:
        from oracle.oracle import OpjReplay
        opj = OpjReplay()
    except OSError:
        opj = None  # (the sub-sampled file is libopenjp2's alone: left out where no library is installed)
    for name in lc.NAMES:
        cs, layers, kw = lc.load(name), lc.layers_of(name), lc.CASES[name][6]
        m = lc.meta()[name]
        src = source_comps(name)
        if not m["oracle_reads"] and opj is None:
            continue
        hashes, errs, nblocks = [], [], []
        for L in range(1, layers + 1):
            cut = lc.strip(cs, L)
            comps = list(oracle.decode(cut, 0)) if m["oracle_reads"] else [c["data"] for c in opj.decode_comps(cut, 0)]
            assert [sha(c) for c in comps] == [e["sha256"] for e in m["decoded"][str(L)]["0"]], (name, L)
            hashes.append(tuple(sha(c) for c in comps))
            errs.append(sum(int(np.abs(d.astype(np.int64) - s).sum()) for d, s in zip(comps, src)))
            if m["oracle_reads"]:
                blocks = oracle.file_blocks(cut)["blocks"]
                nblocks.append(len(blocks))
                assert sum(b["npasses"] for b in blocks) == m["passes"][L - 1]
                if kw.get("mode", 0) == 1 and L < layers:
                    partial_raw += sum(1 for b in blocks if b["npasses"] > 10 and (b["npasses"] - 10) % 3 == 1 and b["segs"][-1][1] == 1)
        assert len(set(hashes)) == layers, name
        assert errs == m["abs_error"] and all(b <= a for a, b in zip(errs, errs[1:])), (name, errs)
        if kw.get("reversible", True) and kw["rates"][-1] == 0.0:
            assert errs[-1] == 0, name
        if nblocks:
            assert nblocks == m["blocks_with_passes"] and nblocks == sorted(nblocks), (name, nblocks)
            grows = grows or nblocks[-1] > nblocks[0]
    assert lc.meta()["l1_128_grey8_53_lrcp_4layers"]["blocks_with_passes"] == [7, 12, 16, 16]
    assert grows and partial_raw


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_planner_with_a_limit_equals_the_planner_of_the_stripped_file(tmp_path):
    """decode_plan.cpp under ASan + UBSan: every fixture, its SOP-less copy and a PPT / PPM repack of the single-tile SOP + EPH
    fixture, every L, reduce 0 and 1, whole and windowed; L = 0 / layers / layers + 7; 200 mutations per file at L = 1."""
    import test_read_fallback as rf
    csrc = os.path.join(ROOT, "j2k_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "native", "decode_layers_host.cpp")] + [os.path.join(csrc, f) for f in ("decode_plan.cpp", "geometry.cpp")]
    exe = str(tmp_path / "decode_layers_host")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I" + os.path.join(ROOT, "include"), *srcs, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    variants = []  # (tag, layers, file, [strip_1 ..])
    for name in lc.NAMES:
        cs, layers = lc.load(name), lc.layers_of(name)
        strips = [lc.strip(cs, L) for L in range(1, layers + 1)]
        variants.append((name, layers, cs, strips))
        variants.append((name + "_nosop", layers, lc.drop_sop(cs), [lc.drop_sop(s) for s in strips]))
        if "_eph" in name:
            for where in ("ppt", "ppm"):
                variants.append((name + "_" + where, layers, rf._repack_headers(cs, where), [rf._repack_headers(s, where) for s in strips]))
    assert sum(1 for v in variants if v[0].endswith(("_ppt", "_ppm"))) == 2
    lines = []
    for tag, layers, data, strips in variants:
        paths = [str(tmp_path / (tag + ".j2k"))] + [str(tmp_path / f"{tag}.L{L + 1}.j2k") for L in range(layers)]
        for p, d in zip(paths, [data] + strips):
            with open(p, "wb") as f:
                f.write(d)
        lines.append(" ".join([str(layers)] + paths))
    manifest = tmp_path / "manifest.txt"
    manifest.write_text("\n".join(lines) + "\n")
    run = subprocess.run([exe, str(manifest)], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert run.stdout.startswith(f"compared {sum(4 * v[1] for v in variants)} plans of {len(variants)} files"), run.stdout
