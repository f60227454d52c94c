"""CPU: the MQ coder's code register as one wide number (j2k_amd/csrc/t1_mq_window.h), the recurrence of the plain two-wave
coder's consumer, as a stand-alone host program (tests/native/t1_mq_window_host.cpp) built with the address and
undefined-behaviour sanitizers and run as a child process.  The program holds the header -- groups of four decisions
accumulated without a test, bytes peeled afterwards, a reported group run again per decision through both state conversions
-- to a plain transcription of T.800 Figure C.3:

  2 000 generated streams of 4 000 decisions (half with Qe = 0x5601 alone, half walking Table C.2 in eight contexts), every
  sixteenth one once more with every group sent back;
  crafted groups, one per report of the header: a pending 0xFF with a late carry, a finished 0xFF that rolls over, four shifts
  of 15, a true 0x00 byte, the block's first byte.

Bytes and final state must be the reference's, each crafted group must be reported by the test it is named for, and at most
1 % of the generated groups may be sent back: a build in which everything falls back to the per-decision coder does not pass.
(The comparison sees the hazard: with the header's `rolled` report taken out, 13 of the first 600 streams differ in a byte.)
What the GPU adds -- lanes of unequal length, the LDS stage and its flush, the wave-wide vote -- is
test_t1_mq_window_blocks.py's.  The sanitizers' runtimes are linked into the program; its environment is the test's own."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "t1_mq_window_host.cpp")

CRAFTED = {  # name -> report (1 carry, 2 rolled, 4 wide)
    "pending 0xFF, late carry": 1,
    "pending 0xFE becomes 0xFF": 0,
    "finished 0xFF rolls": 2,
    "four shifts of 15": 4,
    "four shifts of 15, narrow start": 4,
    "true 0x00 byte": 2,
    "first byte": 0,
    "first byte, not yet out": 0,
}


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("t1_mq_window_host") / "t1_mq_window_host")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "j2k_amd", "csrc"), "-o", exe, SRC])
    return subprocess.run([exe, "2000", "4000", "1"], capture_output=True, text=True)


def test_bytes_and_final_state_are_the_references(report):
    assert report.returncode == 0, (report.stdout[-3000:], report.stderr[-3000:])
    assert "runtime error" not in report.stderr and "AddressSanitizer" not in report.stderr
    m = re.search(r"^(\d+) streams, (\d+) decisions, (\d+) groups", report.stdout, re.M)
    assert m and int(m.group(1)) >= 2000 and int(m.group(2)) >= 2000 * 4000 and int(m.group(3)) == int(m.group(2)) // 4
    assert report.stdout.strip().endswith(f"{len(CRAFTED)} of {len(CRAFTED)} crafted groups as named, 0 failures")


def test_every_crafted_group_is_reported_by_its_test(report):
    got = dict((name, int(r)) for name, r in re.findall(r"^crafted: (.*): report (\d+)$", report.stdout, re.M))
    assert got == CRAFTED


def test_few_groups_run_again(report):
    """At most 1 % of (lane, group) pairs; a CPU model of the construction measured 0.22 % at most."""
    m = re.search(r"^rerun share ([0-9.]+)$", report.stdout, re.M)
    assert m, report.stdout[-2000:]
    share = float(m.group(1))
    assert 0.0 < share <= 0.01, share
