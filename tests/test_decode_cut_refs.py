"""Files cut short, checked without a device: the conditions that make the cases of tests/cut_cases.py prove something; the
Tier-2 planner (decode_plan.cpp, as a stand-alone program under ASan + UBSan: tests/native/decode_cut_host.cpp) against the
oracle's block list of the same cut; the oracle against libopenjp2 where libopenjp2 decodes a cut (whole tile-parts and an
EOC); and the committed hashes of tests/golden/cut/cut.json for the files only libopenjp2 reads."""
import hashlib
import importlib.util
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN_DIR, ROOT

import cut_cases as cc

J2K_HIP_ERR_PARAM = 1


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.int32).tobytes()).hexdigest()


def _key(b):
    return (b["tile"], b["comp"], b["res"], b["orient"], b["rect"][0], b["rect"][1])


def _blocks(oracle, data):
    return {_key(b): b for b in oracle.file_blocks(data)["blocks"]}


def test_fixture_conditions(oracle):
    """The set cannot quietly prove nothing: what the cut files must exercise, counted from the oracle's block lists."""
    seen = dict(missing_tile=0, missing_component=0, included_no_passes=0, table_shortened=0, in_header=0, in_body=0, partial_packet=0)
    for tag in list(cc.ORACLE_FILES) + list(cc.REPACKS):
        data, cases = cc.load(tag), cc.cases(tag)
        w = cc.walk(data)
        refused = [c for c in cases if not cc.decodes(oracle, c)]
        assert len(refused) <= 0.2 * len(cases), (tag, [c["id"] for c in refused])
        for c in refused:  # only before the first SOD, or inside a later tile-part's header
            assert c["end"] < w["parts"][0]["sod"] or any(p["sot"] < c["end"] < p["sod"] for p in w["parts"][1:]), c["id"]
        for c in cases:
            if not cc.decodes(oracle, c):
                continue
            seen["missing_tile"] += bool(cc.missing_tiles(tag, c))
            if tag in cc.STYLED:
                for b in oracle.file_blocks(cc.reference_bytes(c))["blocks"]:
                    seen["table_shortened"] += len(cc.normalise(b["segs"], b["npasses"], len(b["data"]))) < len(b["segs"])
    # the SOP + EPH file shows where a cut fell: inside a packet's header or body, and what became of the packet's blocks
    data = cc.load("u8")
    packets = cc._packets(data, cc.walk(data)["parts"][0])
    for c in cc.cases("u8"):
        hit = [p for p in packets if p[0] <= c["end"] < p[3]]
        if c["kind"] == "a" or not hit:
            continue
        sop, hdr, body, end = hit[0]
        seen["in_header"] += hdr < c["end"] < body
        if not body < c["end"] < end:
            continue
        seen["in_body"] += 1
        before, whole, got = (_blocks(oracle, data[:e]) for e in (sop, end, c["end"]))
        passes = lambda d, k: d[k]["npasses"] if k in d else 0
        touched = [k for k in whole if passes(whole, k) > passes(before, k)]  # the packet's contributions, in the packet's order
        kept = [passes(got, k) == passes(whole, k) for k in touched]
        assert all(passes(got, k) in (passes(before, k), passes(whole, k)) for k in touched), c["id"]  # whole contributions only
        assert kept == sorted(kept, reverse=True), c["id"]  # the first ones are kept, every later one dropped
        seen["partial_packet"] += any(kept) and not all(kept)
        seen["included_no_passes"] += any(k not in got for k in touched)  # its header was read, nothing of it arrived
    for tag in ("d1", "d2"):  # one tile, one tile-part per component: a component missing while its tile is present
        w = cc.walk(cc.load(tag))
        seen["missing_component"] += sum(1 for c in cc.cases(tag) if w["ntiles"] == 1 and c["end"] < w["parts"][-1]["sot"])
    assert all(seen.values()), seen


def _host_listing(tmp_path, cases):
    csrc = os.path.join(ROOT, "j2k_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "native", "decode_cut_host.cpp")] + [os.path.join(csrc, f) for f in ("decode_plan.cpp", "geometry.cpp")]
    exe = str(tmp_path / "decode_cut_host")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I" + os.path.join(ROOT, "include"), *srcs, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    lines = []
    for c in cases:
        path = tmp_path / (c["tag"] + ".j2k")
        if not path.exists():
            path.write_bytes(cc.load(c["tag"]))
        lines.append(f"{c['id']} {path} {c['end']} {int(c['eoc'])}")
    manifest = tmp_path / "manifest.txt"
    manifest.write_text("\n".join(lines) + "\n")
    run = subprocess.run([exe, str(manifest)], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    out, cur = {}, None
    for ln in run.stdout.splitlines():
        f = ln.split(" ")
        if f[0] == "case":
            cur = out[(f[1], int(f[2]))] = dict(err=int(f[4]) if f[3] == "err" else 0, blocks=[])
        elif f[0] == "b":
            t, comp, res, orient, x, y, bw, bh, nb, npass = (int(v) for v in f[1:11])
            data = b"" if f[11] == "-" else bytes.fromhex(f[11])
            segs = [] if f[12] == "-" else [tuple(int(v) for v in s.split(":")) for s in f[12].split(",")]
            cur["blocks"].append(dict(key=(t, comp, res, orient, x, y), w=bw, h=bh, numbps=nb, npasses=npass, data=data, segs=segs))
    assert run.stdout.splitlines()[-1] == f"done {len(cases)}"
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_planner_equals_the_oracle_on_cut_files(tmp_path, oracle):
    """decode_plan.cpp under ASan + UBSan on every cut, reduce 0 and 1: it refuses (J2K_HIP_ERR_PARAM) exactly where the oracle
    does, and otherwise hands Tier-1 the oracle's blocks -- identity, bit-planes, coding passes, codeword bytes, and the
    codeword segment table once both are normalised (cut_cases.normalise)."""
    cases = [c for tag in list(cc.ORACLE_FILES) + list(cc.REPACKS) for c in cc.cases(tag)]
    got = _host_listing(tmp_path, cases)
    compared = blocks = 0
    for c in cases:
        ref = cc.reference_bytes(c)
        ok = cc.decodes(oracle, c)
        numres = oracle.decode_info(ref)["numres"] if ok else 0
        for red in (0, 1):
            g = got[(c["id"], red)]
            assert (g["err"] == 0) == ok and g["err"] in (0, J2K_HIP_ERR_PARAM), (c["id"], red, g["err"])
            if not ok:
                continue
            want = sorted((b for b in oracle.file_blocks(ref)["blocks"] if b["res"] <= numres - 1 - red), key=_key)
            have = sorted(g["blocks"], key=lambda b: b["key"])
            assert [b["key"] for b in have] == [_key(b) for b in want], (c["id"], red)
            for h, wnt in zip(have, want):
                at = (c["id"], red, h["key"])
                assert (h["w"], h["h"], h["numbps"], h["npasses"]) == (wnt["w"], wnt["h"], wnt["numbps"], wnt["npasses"]), at
                assert h["data"] == wnt["data"], at
                assert cc.normalise(h["segs"], h["npasses"], len(h["data"])) == cc.normalise(wnt["segs"], wnt["npasses"], len(wnt["data"])), at
            compared += 1
            blocks += len(have)
    assert compared > 2 * 0.8 * len(cases) and blocks > compared


def _boundary_eoc(tag):
    return [c for c in cc.cases(tag) if c["kind"] == "a" and c["eoc"]]


@pytest.mark.parametrize("tag", [t for t in cc.ORACLE_FILES if _boundary_eoc(t)])
def test_oracle_equals_libopenjp2_on_whole_tile_parts(oracle, opj, tag):
    """Whole tile-parts and an EOC: libopenjp2 decodes these, and the oracle equals it sample for sample, at full size and
    reduced.  The samples of a tile that never arrived are component value 0 (not the mid level an all-zero tile decodes to)."""
    w = cc.walk(cc.load(tag))
    for c in _boundary_eoc(tag):
        for red in (0, 1):
            dec = cc.expected(oracle, c, red)
            lib = opj.decode_comps(cc.cut_bytes(c), red)
            assert len(lib) == dec.shape[0]
            for k, comp in enumerate(lib):
                assert np.array_equal(comp["data"], dec[k]), (c["id"], red, k)
            for t in cc.missing_tiles(tag, c):
                x0, y0, x1, y1 = cc.tile_rect(w, t, red)
                assert x1 > x0 and y1 > y0 and not dec[:, y0:y1, x0:x1].any(), (c["id"], red, t)


def test_committed_hashes_cover_the_cases():
    """tests/golden/cut/cut.json holds, for the files the oracle does not read, one entry per case and reduce factor."""
    g = cc.golden()
    want = {c["id"] for tag in cc.OPJ_FILES for c in cc.cases(tag)}
    assert set(g["cases"]) == want and want
    for cid, e in g["cases"].items():
        assert set(e["decoded"]) == {"0", "1"} and all(len(h["sha256"]) == 64 for r in e["decoded"].values() for h in r), cid


def test_generator_reproduces_the_committed_hashes(opj):
    """With a live libopenjp2: the maker computes the committed index again (2.4.0 and 2.5.4 agree on these decodes)."""
    spec = importlib.util.spec_from_file_location("make_cut_golden", os.path.join(GOLDEN_DIR, "make_cut_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert json.loads(json.dumps(gen.generate(opj))) == cc.golden()
