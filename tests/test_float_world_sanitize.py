"""The host binding's float worlds (HipCodec and the test hook with FLOAT channels) as a stand-alone program under ASan + UBSan
on the CPU, against a stand-in for the C ABI that walks every channel view it is handed: no device, nothing loaded into
python."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_float_worlds_through_the_host_binding_under_sanitizers(tmp_path):
    host = os.path.join(ROOT, "j2k_amd", "host")
    srcs = [os.path.join(ROOT, "tests", "native", "float_world_sanitize.cpp"), os.path.join(host, "hip_codec.cpp"), os.path.join(host, "host_test_hook.cpp")]
    exe = str(tmp_path / "float_world_sanitize")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I" + os.path.join(ROOT, "include"), "-I" + host, *srcs, "-lpthread", "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert run.stdout.count("ok ") == 19
