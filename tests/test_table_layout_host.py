"""CPU: the layouts of the device tables an encode fills (j2k_amd/csrc/table_layout.h: T1Tables, GatherPlan) as a stand-alone
host program (tests/native/table_layout_host.cpp) that includes the header alone, built with the address and
undefined-behaviour sanitizers and run as a child process.  GatherPlan over blob_bytes in {0, 1, 8, 15, 16} and each of nh,
nbd, nseg in {0, 1, 3}: the tables in the documented order without overlap, 64-bit tables 8-byte and 32-bit tables 4-byte
aligned, the last one inside the reported total, a GatherArgs filled from a base equal to the typed pointers over it.
T1Tables over nb in {0, 1, 64, 65}: columns nb words apart, err at word 4 nb inside the meta size, row(i) in steps of the
passes per block.  The frame path and the stage hooks both go through these two types, so what holds here holds for both.
The sanitizers' runtimes are linked into the program; its environment is the test's own, unchanged."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "table_layout_host.cpp")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "this test needs g++"
    exe = str(tmp_path_factory.mktemp("table_layout_host") / "table_layout_host")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "j2k_amd", "csrc"), "-o", exe, SRC])
    return exe


def test_table_layouts_on_the_host(program):
    r = subprocess.run([program], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) > 1000
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
