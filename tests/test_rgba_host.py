"""CPU: the host side of the fused RGBA output stage under ASan + UBSan, as a stand-alone program (tests/native/
rgba_sanitize.cpp): the classifier over the committed files, and the function that fills the kernel's arguments -- the
packed form for every permutation of a record's four bases and for nothing else, every refusal."""
import os
import shutil
import subprocess

import pytest

import rgba_cases as rc
from conftest import GOLDEN_DIR, ROOT


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_classifier_and_argument_filler_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "j2k_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "native", "rgba_sanitize.cpp")] + [os.path.join(csrc, f) for f in ("rgba_plan.cpp", "decode_plan.cpp", "geometry.cpp")]
    exe = str(tmp_path / "rgba_sanitize")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I" + os.path.join(ROOT, "include"), *srcs, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    args = []
    for name, mode in sorted(rc.MODES.items()):
        if name == "pal":  # crafted at run time
            path = str(tmp_path / "pal.jp2")
            with open(path, "wb") as f:
                f.write(rc.load("pal"))
        else:
            path = os.path.join(GOLDEN_DIR, rc.FILES[name])
        args += [path, str(mode or 0)]
    run = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert run.stdout.startswith(f"classified {len(rc.MODES)} files, filled the arguments for 24 permutations")
