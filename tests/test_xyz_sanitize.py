"""Host-side C++ of the cinema colour front end (the tables of xyz_tables.cpp, the threshold search that defines a code,
normalise's acceptance and refusals of rgb_to_xyz) as a stand-alone program under ASan + UBSan on the CPU: no device, nothing
loaded into python."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_xyz_host_logic_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "j2k_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "native", "xyz_sanitize.cpp")] + [os.path.join(csrc, f) for f in ("xyz_tables.cpp", "geometry.cpp")]
    exe = str(tmp_path / "xyz_sanitize")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I" + os.path.join(ROOT, "include"), *srcs, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert run.stdout.count("ok ") == 31  # 27 + 1 table sets, the argument checks, the accepted sets, the refusals
