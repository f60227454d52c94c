"""CPU: the lane-per-block Tier-1 decoder (j2k_amd/csrc/t1_dec_lane.h) under code-block styles, as a stand-alone host program
with one lane (tests/native/t1_lane_styled_host.cpp) built with the address and undefined-behaviour sanitizers and run as a
child process.  Every group of cases that test_t1_dec_styled_blocks.py sends to the GPU goes through it here: the families
of t1_styled_families.py under their styles, every last pass, codewords and segment tables cut short, damaged raw and
MQ-coded segments, every block of the styled files of libopenjp2 (the vertically causal ones among them), many bit-planes, and the
orders.  Expected samples are the oracle's styled block decoder's.  A second build without the ring's refill on the beat
(-DT1L_TEST_NO_REFILL) runs the long raw segments through the slow byte path.  The sanitizers' runtimes are linked into
the program; its environment is the test's own, unchanged."""
import os
import shutil
import subprocess

import pytest

import t1_dec_styled_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "t1_lane_styled_host.cpp")


def _build(tmp_path_factory, name, extra=()):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wno-unknown-pragmas", *extra, "-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return _build(tmp_path_factory, "t1_lane_styled_host")


@pytest.fixture(scope="module")
def program_no_refill(tmp_path_factory):
    return _build(tmp_path_factory, "t1_lane_styled_slow", ["-DT1L_TEST_NO_REFILL"])


def _run(program, path):
    return subprocess.run([program, path], capture_output=True, text=True)


def _check(program, oracle, tmp_path, batches):
    path = str(tmp_path / "blocks.cases")
    n, dec = tc.write_case_file(path, oracle, batches)
    assert n and dec
    r = _run(program, path)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith(f"{n} cases, {dec} decoded, 0 with a mismatch")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


@pytest.mark.parametrize("name", tc.GROUP_NAMES)
def test_lane_decoder_on_the_host_matches_the_styled_oracle(program, oracle, tmp_path, name):
    _check(program, oracle, tmp_path, tc.group(oracle, name))


@pytest.mark.parametrize("name", ["small-1", "small-5", "small-55", "lastpass-1", "cutshort-5", "spoiled-raw-1", "damaged-mq-4", "damaged-mq-5",
                                  "manyplanes"])
def test_slow_byte_path_reads_long_raw_segments_the_same(program_no_refill, oracle, tmp_path, name):
    batches = tc.group(oracle, name)
    assert any(n > 64 for _, s, cases in batches for c in cases for n, _ in c["segs"])  # a segment longer than the ring
    _check(program_no_refill, oracle, tmp_path, batches)


def test_the_program_reports_a_mismatch(program, oracle, tmp_path):
    """The comparison has teeth: one wrong expected sample is reported, with its case."""
    rev, style, cases = tc.group(oracle, "small-5")[0]
    path = str(tmp_path / "spoiled.cases")
    real = tc.expected_words

    def spoiled(oracle_, case, rev_, style_):
        e = real(oracle_, case, rev_, style_)
        if case is cases[3]:
            e = e.copy()
            e[0, 0] ^= 1
        return e
    tc.expected_words = spoiled
    try:
        tc.write_case_file(path, oracle, [(rev, style, cases)])
    finally:
        tc.expected_words = real
    r = _run(program, path)
    assert r.returncode == 1
    assert "case 3 (style 5" in r.stdout and "sample (y, x) = (0, 0)" in r.stdout
    assert r.stdout.strip().endswith("1 with a mismatch")
