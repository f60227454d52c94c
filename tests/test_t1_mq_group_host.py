"""CPU: the group form of the MQ coder's wide code register (j2k_amd/csrc/t1_mq_window.h) -- a group of four decisions summed
by the producer into {G, N}, taken by the consumer in one step, a zero byte reported only if a carry crossed its top boundary
-- as a stand-alone host program (tests/native/t1_mq_group_host.cpp) built with the address and undefined-behaviour
sanitizers and run as a child process.  The program holds that text to a plain transcription of T.800 Figure C.3:

  2 000 generated streams of 4 000 decisions, seed 1 (half with Qe = 0x5601 alone, half walking Table C.2 in eight contexts),
  every sixteenth one twice more: every group reported long, every group sent back;
  streams of every length from 1 to 23 and of 4 000 + 1, 2, 3 decisions, in all three ways;
  30 000 short streams from hard starts -- the pending byte 0xFD..0xFF above live bits of C that are nearly all ones: a 0xFF
  under a 0xFE with a carry behind both, which the generated streams seldom reach and the frames of a sequence do (a zero
  byte's boundary taken one bit too high behind a 0xFF passes the 8 M decisions above and fails 480 of these);
  crafted groups, each named for the report it must give;
  pack and unpack of the queue words for every shift 0..15 in every slot beside every Qe of Table C.2.

Bytes and final state must be the reference's.  At most 0.1 % of the generated (lane, group) pairs may be coded again -- a CPU
model of the construction gives 0.057 % on these streams, the conservative `rolled` test of mq_wide_peel 0.16 %: a build that
kept the old test, or sends everything back, does not pass -- and at most 0.01 % may be long (the model: 0.0005 %).
What the GPU adds -- 64 lanes voting, the LDS queue, the stage -- is test_t1_mq_group_blocks.py's.  The sanitizers' runtimes
are linked into the program; its environment is the test's own."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "t1_mq_group_host.cpp")

CRAFTED = {  # name -> report (1 carry, 2 rolled, 8 long)
    "finished 0xFF rolls": 2,
    "finished 0xFF rolls under a 0xFE": 2,
    "true 0x00 byte": 0,
    "0x00 byte, a carry crossed its top": 2,
    "pending 0xFF, late carry": 1,
    "pending 0xFE becomes 0xFF": 0,
    "N = 15, G at its bound": 0,
    "N = 15, G at its bound, widest start": 0,
    "N = 16": 8,
    "four shifts of 15": 8,
    "first byte": 0,
}


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("t1_mq_group_host") / "t1_mq_group_host")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "j2k_amd", "csrc"), "-o", exe, SRC])
    return subprocess.run([exe, "2000", "4000", "1"], capture_output=True, text=True)


def _share(report, name):
    m = re.search(rf"^{name} share ([0-9.]+)$", report.stdout, re.M)
    assert m, report.stdout[-2000:]
    return float(m.group(1))


def test_bytes_and_final_state_are_the_references(report):
    assert report.returncode == 0, (report.stdout[-3000:], report.stderr[-3000:])
    assert "runtime error" not in report.stderr and "AddressSanitizer" not in report.stderr
    m = re.search(r"^(\d+) streams, (\d+) decisions, (\d+) groups", report.stdout, re.M)
    assert m and int(m.group(1)) == 2000 and int(m.group(2)) == 2000 * 4000 and int(m.group(3)) == int(m.group(2)) // 4
    m = re.search(r"^(\d+) streams whose length is no multiple of four or below a chunk$", report.stdout, re.M)
    assert m and int(m.group(1)) == 2 * 23 + 3 * 8
    m = re.search(r"^(\d+) hard starts$", report.stdout, re.M)
    assert m and int(m.group(1)) == 30000
    assert report.stdout.strip().endswith(f"{len(CRAFTED)} of {len(CRAFTED)} crafted groups as named, 0 failures")


def test_every_crafted_group_gives_its_report(report):
    got = dict((name, int(r)) for name, r in re.findall(r"^crafted: (.*): report (\d+)$", report.stdout, re.M))
    assert got == CRAFTED


def test_queue_words_round_trip(report):
    m = re.search(r"^pack: (\d+) groups round trip$", report.stdout, re.M)
    assert m and int(m.group(1)) == 4 * 16 * 47 * 2, report.stdout[-2000:]
    assert "does not round trip" not in report.stdout and "unpacked as" not in report.stdout


def test_few_groups_are_coded_again(report):
    """Above 0 and at most 0.1 % of (lane, group) pairs: a true zero byte is not sent back."""
    share = _share(report, "rerun")
    print("rerun share", share, "zero share", _share(report, "zero"))
    assert 0.0 < share <= 0.001, share


def test_few_groups_are_long(report):
    """At most 0.01 % of (lane, group) pairs shift by more than 15 in all."""
    share = _share(report, "long")
    print("long share", share)
    assert share <= 0.0001, share
