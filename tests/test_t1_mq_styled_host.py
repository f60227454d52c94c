"""CPU: StyledCoder (j2k_amd/csrc/t1_mq_styled.h), the recurrence of the styled coder kernel, as a stand-alone host
program (tests/native/t1_mq_styled_host.cpp) built with the address and undefined-behaviour sanitizers and run as a child
process over the decision streams of the CPU oracle: every block of both families of t1_styled_families.py under each of
the 31 non-zero combinations of bypass, reset, termall, pterm and segsym -- the one place where all combinations meet the
long blocks.  Codeword bytes, length and the byte count at every segment end must be the oracle's.  The decisions are the
modeller's bytes, (context << 1) | bit, with the plain sign in raw passes: the oracle's trace has that format, and it does
not depend on the style beyond the bypass bit (asserted through pass_nsym).  What the GPU adds to this -- the LDS sink
and its drain, divergent lanes, the bypass modeller -- is test_t1_styled_blocks.py's.

The program also runs every case through a model of the kernel's byte stage, and through one whose drain keeps 0..15
bytes instead of 16..31.  test_the_drain_block_needs_the_kept_unit asserts that the blocks of DRAIN_CASES give another
codeword on the second model: the GPU comparison of those blocks is what holds the kernel's drain to its
16..31 bytes.  The sanitizers' runtimes are linked into the program; its environment is the test's own, unchanged."""
import os
import shutil
import struct
import subprocess

import pytest

import t1_styled_families as fam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "t1_mq_styled_host.cpp")
NOT_AN_END = 0xffffffff


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("t1_mq_styled_host") / "t1_mq_styled_host")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-Wall",
                           "-I", os.path.join(ROOT, "j2k_amd", "csrc"), "-o", exe, SRC])
    return exe


def _run(program, path):
    return subprocess.run([program, path], capture_output=True, text=True)


def _write_cases(path, oracle, family, styles, spoil=None):
    """The case file of a family (format: t1_mq_styled_host.cpp).  spoil(case dict) may falsify a case."""
    blocks = fam.scaled_blocks(oracle, family, True)
    streams, index = [], {}
    for b, (data, o) in enumerate(blocks):
        for bypass in (0, 1):
            r = oracle.t1_block(data, o, style=1 if bypass else 2, want_symbols=True)
            index[(b, bypass)] = (len(streams), r["pass_nsym"])
            streams.append(r["symbols"].tobytes())
    cases = []
    for style in styles:
        for b, r in enumerate(fam.refs(oracle, family, True, style)):
            si, pass_nsym = index[(b, style & 1)]
            assert r["pass_nsym"] == pass_nsym, (b, style)  # the decisions depend on the style through the bypass bit alone
            ends = [r["rates"][p] if r["seg_ends"][p] else NOT_AN_END for p in range(r["npasses"])]
            c = dict(block=b, style=style, stream=si, pass_nsym=pass_nsym, ends=ends, data=r["data"])
            if spoil:
                spoil(c)
            cases.append(c)
    with open(path, "wb") as f:
        f.write(b"T1SC" + struct.pack("<I", len(streams)))
        for s in streams:
            f.write(struct.pack("<I", len(s)) + s)
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            n = len(c["pass_nsym"])
            f.write(struct.pack(f"<4I{n}I{n}II", c["block"], c["style"], c["stream"], n, *c["pass_nsym"], *c["ends"], len(c["data"])))
            f.write(c["data"])
    return len(cases)


@pytest.mark.parametrize("family", ["mixed", "small"])
def test_styled_coder_on_the_host_matches_the_oracle(program, oracle, tmp_path, family):
    path = str(tmp_path / (family + ".cases"))
    n = _write_cases(path, oracle, family, fam.SMALL_STYLES)
    assert n == 31 * len(fam.FAMILIES[family]())
    r = _run(program, path)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith(f"{n} cases, 0 with a mismatch")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_the_drain_block_needs_the_kept_unit(program, oracle, tmp_path):
    """Each of DRAIN_CASES -- the steered block of the small family under bypass with and without TERMALL, and a block of
    the mixed family under bypass with PTERM -- codes right on the model of the kernel's stage and wrong on a stage that
    keeps 0..15 bytes: a kernel whose drain kept less than a unit fails the GPU comparison of these blocks."""
    for family in sorted({f for f, _, _ in fam.DRAIN_CASES}):
        path = str(tmp_path / (family + "_drain.cases"))
        _write_cases(path, oracle, family, sorted({s for f, _, s in fam.DRAIN_CASES if f == family}))
        r = _run(program, path)
        assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
        for f, block, style in fam.DRAIN_CASES:
            if f == family:
                assert f"block {block} style {style} tells the stages apart" in r.stdout, (f, block, style)


def test_the_program_reports_a_mismatch(program, oracle, tmp_path):
    """The comparison has teeth: one wrong codeword byte and one wrong segment end are each reported."""
    def spoil(c):
        if c["block"] == 0 and c["style"] == 4:
            c["data"] = c["data"][:3] + bytes([c["data"][3] ^ 1]) + c["data"][4:]
        if c["block"] == 1 and c["style"] == 5:
            c["ends"][-1] += 1
    path = str(tmp_path / "spoiled.cases")
    _write_cases(path, oracle, "small", [4, 5], spoil)
    r = _run(program, path)
    assert r.returncode == 1
    assert "block 0 style 4: codeword byte at 3" in r.stdout and "block 1 style 5: segment end of pass" in r.stdout
    assert r.stdout.strip().endswith("2 with a mismatch")
