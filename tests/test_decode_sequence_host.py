"""CPU: the host side of the sequence decode (include/j2k_hip.h: j2k_hip_decode_sequence*).  Which frames may share a call
(j2k_hip_decode_sequence_check: headers only, no device), and the merge of the frames' plans into one set of tables
(j2k_amd/csrc/decode_seq.cpp) as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer."""
import glob
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN_DIR, ROOT
from j2k_amd import api
from test_read_fallback import _marker, _seg, _with_coc

J2K_HIP_ERR_PARAM, J2K_HIP_ERR_UNSUPPORTED = 1, 6


def load(name):
    return open(os.path.join(GOLDEN_DIR, name + ".j2k"), "rb").read()


def with_comment(data: bytes, text: bytes) -> bytes:
    """`data` with one more COM segment (Rcom = 1: Latin text) behind its QCD."""
    pos, q = _marker(data, 0xFF5C)
    end = pos + 4 + len(q)
    return data[:end] + _seg(0xFF64, b"\x00\x01" + text) + data[end:]


def with_qcd_exponent(data: bytes, by: int) -> bytes:
    """`data` with the first exponent of its QCD raised by `by` (reversible: a byte per band, exponent << 3)."""
    pos, q = _marker(data, 0xFF5C)
    assert q[0] & 31 == 0
    out = bytearray(data)
    out[pos + 5] = ((q[1] >> 3) + by) << 3
    return bytes(out)


def with_style(data: bytes, style: int) -> bytes:
    pos, cod = _marker(data, 0xFF52)
    out = bytearray(data)
    assert out[pos + 4 + 8] == cod[8]
    out[pos + 4 + 8] = style
    return bytes(out)


def refused(files):
    with pytest.raises(api.J2kHipError) as ei:
        api.sequence_check(files)
    return ei.value


def test_sequence_check_accepts_frames_of_one_geometry():
    g3 = load("g3_300x200_rgb8_53_rct")
    other = with_comment(g3, b"another comment, of another length")
    assert api.read_info(other)["width"] == 300 and len(other) != len(g3)
    api.sequence_check([g3, other, g3[:len(g3) * 7 // 10]])
    api.sequence_check([g3])


def test_sequence_check_refuses_frames_that_differ():
    g3, g4 = load("g3_300x200_rgb8_53_rct"), load("g4_300x200_rgb16_53_rct_tile128")
    e = refused([g3, g4])
    assert e.code == J2K_HIP_ERR_PARAM and e.frame == 1 and "frame 1: " in str(e)
    e = refused([g3, g3, with_qcd_exponent(g3, 1), g3])
    assert e.code == J2K_HIP_ERR_PARAM and e.frame == 2 and "frame 2: " in str(e) and "QCD" in str(e)
    e = refused([g3, with_style(g3, 0x02)])
    assert e.code == J2K_HIP_ERR_PARAM and e.frame == 1 and "frame 1: " in str(e) and "style" in str(e)
    e = refused([])
    assert e.code == J2K_HIP_ERR_PARAM and e.frame == 0 and "frame 0: " in str(e)
    e = refused([g3, b""])
    assert e.code == J2K_HIP_ERR_PARAM and e.frame == 1 and "frame 1: " in str(e)
    e = refused([g3, g3[:40]])  # a main header cut short: malformed, not unsupported
    assert e.code == J2K_HIP_ERR_PARAM and e.frame == 1


def test_sequence_check_reports_an_unsupported_frame():
    g6 = load("g6_300x200_rgb16_97_ict")
    bad = _with_coc(g6, (1,), -1)  # a COC that changes a component's levels (tests/test_read_fallback.py)
    with pytest.raises(api.J2kHipError) as ei:
        api.read_info(bad)
    assert ei.value.code == J2K_HIP_ERR_UNSUPPORTED
    e = refused([g6, g6, bad])
    assert e.code == J2K_HIP_ERR_UNSUPPORTED and e.frame == 2 and "frame 2: " in str(e) and "COC" in str(e)
    e = refused([bad, g6])
    assert e.code == J2K_HIP_ERR_UNSUPPORTED and e.frame == 0 and "frame 0: " in str(e)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_plan_merge_under_sanitizers(tmp_path):
    """decode_seq.cpp's merge on every golden file taken three times (whole, cut at 70 %, cut at 35 %), the styled and ext/
    files included: a stand-alone program, nothing is loaded into Python."""
    csrc = os.path.join(ROOT, "j2k_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "native", "decode_seq_sanitize.cpp")] + \
           [os.path.join(csrc, f) for f in ("decode_plan.cpp", "geometry.cpp", "decode_seq.cpp")]
    exe = str(tmp_path / "decode_seq_sanitize")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I" + os.path.join(ROOT, "include"), *srcs, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    files = sorted(glob.glob(os.path.join(GOLDEN_DIR, "*.j2k")) + glob.glob(os.path.join(GOLDEN_DIR, "*.jp2")) +
                   glob.glob(os.path.join(GOLDEN_DIR, "ext", "*.j2k")) + glob.glob(os.path.join(GOLDEN_DIR, "styles", "*.j2k")) +
                   glob.glob(os.path.join(GOLDEN_DIR, "styles_dec", "*.j2k")) + glob.glob(os.path.join(GOLDEN_DIR, "rgba", "*.jp2")))
    assert len(files) > 60
    run = subprocess.run([exe] + files, capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert run.stdout.startswith("merged ")
    assert int(run.stdout.split()[1]) >= len(files) - 2  # (the files this reader leaves to the fallback do not plan: CMYK is read, a differing COC is not)
