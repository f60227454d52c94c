"""CPU: j2k_hip_region_footprint -- which coefficients of a Mallat plane a window of the image needs -- against the
project's own inverse transforms (oracle.idwt53 / idwt97), with no device.

Sufficiency: every coefficient OUTSIDE the returned rectangles is overwritten with large random values; the window of the
oracle's transform must not change by a bit.  Not trivially everything: for a 24 x 24 window of a 256 x 256 plane the
top level's band rectangles stay within 24 samples a side (the exact need is 12 plus the filter's margin)."""
import numpy as np
import pytest

import region_cases as rc
from j2k_amd import api


def _idwt(oracle, a, levels, rev, x0, y0):
    return (oracle.idwt53 if rev else oracle.idwt97)(a, levels, x0, y0)


@pytest.mark.parametrize("case", rc.CASES, ids=rc.case_id)
def test_footprint_is_sufficient(oracle, case):
    w, h, x0, y0, levels, rev = case
    rng = np.random.default_rng(1000 * w + 10 * levels + x0 + int(rev))
    a = rc.plane(rng, w, h, rev)
    want = _idwt(oracle, a, levels, rev, x0, y0)
    for win in rc.windows(w, h, seed=w + levels):
        rects = api.region_footprint(w, h, levels, rev, win, x0, y0)
        assert len(rects) == 3 * levels + 1
        mask = rc.footprint_mask(rects, w, h)
        got = _idwt(oracle, rc.poison(a, mask, rev, rng, hard=False), levels, rev, x0, y0)
        x, y, ww, wh = win
        assert np.array_equal(got[y:y + wh, x:x + ww].view(np.int32), want[y:y + wh, x:x + ww].view(np.int32)), (win, rects)


@pytest.mark.parametrize("rev", [True, False], ids=["53", "97"])
def test_footprint_is_not_everything(rev):
    rects = api.region_footprint(256, 256, 3, rev, (100, 100, 24, 24))
    for (x, y, w, h) in rects[7:10]:  # HL, LH, HH of the top level
        assert 12 <= w <= 24 and 12 <= h <= 24, rects
    for (x, y, w, h) in rects[:7]:    # and the levels below shrink further
        assert 1 <= w <= 24 and 1 <= h <= 24, rects
    # the rectangles lie in their bands: LL of 32 x 32, then bands of 32, 64, 128 behind the lower resolution
    assert rects[0][0] + rects[0][2] <= 32 and rects[0][1] + rects[0][3] <= 32
    for lvl, size in ((0, 32), (1, 64), (2, 128)):
        hl, lh, hh = rects[1 + 3 * lvl:4 + 3 * lvl]
        assert size <= hl[0] and hl[0] + hl[2] <= 2 * size and hl[1] + hl[3] <= size
        assert lh[0] + lh[2] <= size and size <= lh[1] and lh[1] + lh[3] <= 2 * size
        assert size <= hh[0] and hh[0] + hh[2] <= 2 * size and size <= hh[1] and hh[1] + hh[3] <= 2 * size


def test_whole_plane_window_needs_every_coefficient():
    for rev in (True, False):
        rects = api.region_footprint(37, 29, 3, rev, (0, 0, 37, 29), 3, 5)
        assert rc.footprint_mask(rects, 37, 29).all()


def test_footprint_parameter_checks():
    for win in ((30, 0, 8, 8), (0, 25, 4, 5), (0, 0, 0, 4), (0, 0, 4, 0), (37, 0, 1, 1)):
        with pytest.raises(api.J2kHipError) as ei:
            api.region_footprint(37, 29, 2, True, win)
        assert ei.value.code == 1  # J2K_HIP_ERR_PARAM
    with pytest.raises(api.J2kHipError) as ei:
        api.region_footprint(37, 29, 2, True, (0, 0, 4, 4), nrects=6)
    assert ei.value.code == 1
    with pytest.raises(api.J2kHipError):
        api.region_footprint(0, 29, 2, True, (0, 0, 1, 1))


@pytest.mark.skipif(__import__("shutil").which("g++") is None, reason="g++ not available")
def test_window_planner_under_sanitizers(tmp_path):
    """plan_decode with a window on every committed file at reduce 0 .. 2 (tests/native/region_sanitize.cpp, ASan + UBSan): no
    more blocks than the whole image, all of them for the whole-image window, every footprint inside its resolution and its
    bands -- the windowed inverse DWT indexes the planes with them -- and windows outside the image refused."""
    import glob
    import os
    import subprocess
    from conftest import ROOT
    csrc = os.path.join(ROOT, "j2k_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "native", "region_sanitize.cpp")] + [os.path.join(csrc, f) for f in ("decode_plan.cpp", "geometry.cpp")]
    exe = str(tmp_path / "region_sanitize")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I" + os.path.join(ROOT, "include"), *srcs, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    files = sorted(p for pat in ("*.j2k", "*.jp2", os.path.join("ext", "*.j2k")) for p in glob.glob(os.path.join(ROOT, "tests", "golden", pat))
                   if os.path.getsize(p) < (1 << 20))
    assert len(files) >= 20
    run = subprocess.run([exe] + files, capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert run.stdout.startswith("planned ")
