"""CPU: the guard-bits parameter of the write side (j2k_hip_params.guard_bits) as far as it goes without a
device.  What is refused and with which text; the main header and the block table under a fixed count; the rule
j2k_hip_guard_bits_needed against the classifier of tests/guard_cases.py (the oracle's Tier-1); host Tier-2 alone on the oracle's
block results -- strict counts refuse an `over` frame with the text they always had, three guard bits and J2K_HIP_GUARD_AUTO
plan it, auto reporting 3, and a frame in range is planned at 2 to the oracle file's length; and the plan, excess, re-plan
path as a stand-alone program under the address and undefined-behaviour sanitizers (tests/native/guard_replan_host.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import guard_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD_TEXT = "code-block has more bit-planes than its sub-band signals (guard bits exceeded)"
J2K_HIP_ERR_PARAM, J2K_HIP_ERR_OVERFLOW = 1, 4


@pytest.fixture(scope="module")
def api():
    from j2k_amd import api
    return api


def _ids(c):
    return c.name


def _with(api, c, g):
    p = gc.api_params(api, c)
    p.guard_bits = g
    return p


def _results(oracle, c):
    rows = gc.classify(oracle, c)
    return ([b["numbps"] for b in rows], [b["t1"]["included"] for b in rows], [b["t1"]["length"] for b in rows])


def _refused(api, call, code, *words):
    with pytest.raises(api.J2kHipError) as ei:
        call()
    assert ei.value.code == code and all(w in str(ei.value) for w in words), str(ei.value)


# ---------------------------------------------------------------------------------------------------------------------- parameters
def test_values_that_are_refused_name_the_field(api):
    AUTO = api.GUARD_AUTO
    assert AUTO == 0x100
    for g in (8, 9, 0xff, AUTO | 8, 0x200, 0x300 | 2, 0x80000000, 0xffffffff):
        _refused(api, lambda: api.main_header(api.make_params(64, 64, 3, 8, guard_bits=g)), J2K_HIP_ERR_PARAM, "guard_bits")
        _refused(api, lambda: api.frame_blocks(api.make_params(64, 64, 3, 8, guard_bits=g)), J2K_HIP_ERR_PARAM, "guard_bits")
    for g in range(0, 8):  # every count is taken, and every floor by the calls that plan a frame
        api.main_header(api.make_params(64, 64, 3, 8, guard_bits=g))
        api.frame_blocks(api.make_params(64, 64, 3, 8, guard_bits=AUTO | g))


def test_a_count_beyond_the_readers_bit_planes_is_refused(api):
    """decode_plan.cpp takes at most 30 bit-planes in a code-block: a count whose bands would signal more is not written.  The
    block table holds every band's Mb; the largest at two guard bits decides which counts pass, and a floor is held alike."""
    mb = api.BLOCK_COLUMNS.index("Mb")
    refused = 0
    for kw in (dict(reversible=False, num_resolutions=6), dict(reversible=True, num_resolutions=6), dict(reversible=False, num_resolutions=9)):
        w = 256 if kw["num_resolutions"] == 9 else 64
        top = int(api.frame_blocks(api.make_params(w, w, 3, 16, ycc=True, **kw))[:, mb].max())
        assert top <= 30
        for g in range(1, 8):
            p = api.make_params(w, w, 3, 16, ycc=True, guard_bits=g, **kw)
            pa = api.make_params(w, w, 3, 16, ycc=True, guard_bits=api.GUARD_AUTO | g, **kw)
            if top + g - 2 > 30:
                refused += 1
                _refused(api, lambda: api.main_header(p), J2K_HIP_ERR_PARAM, "guard_bits", "30 bit-planes")
                _refused(api, lambda: api.frame_blocks(pa), J2K_HIP_ERR_PARAM, "guard_bits", "30 bit-planes")
            else:
                assert int(api.frame_blocks(p)[:, mb].max()) == top + g - 2 == int(api.frame_blocks(pa)[:, mb].max())
    assert refused  # (16-bit 9/7 frames reach the limit below seven guard bits)


def test_cinema_profiles_take_no_guard_bits(api):
    for g in (1, 2, 3, api.GUARD_AUTO, api.GUARD_AUTO | 3):
        _refused(api, lambda: api.main_header(api.make_params(512, 270, 3, 12, reversible=False, ycc=True, dci_profile=3, guard_bits=g)),
                 J2K_HIP_ERR_PARAM, "guard_bits", "dci_profile")
    api.main_header(api.make_params(512, 270, 3, 12, reversible=False, ycc=True, dci_profile=3))


def test_auto_needs_a_frame(api):
    """A header made without a frame cannot say how many guard bits the frame needs; a fixed count is fine."""
    for floor in (0, 2, 3):
        _refused(api, lambda: api.main_header(api.make_params(64, 64, 3, 8, guard_bits=api.GUARD_AUTO | floor)), J2K_HIP_ERR_PARAM, "guard_bits", "J2K_HIP_GUARD_AUTO")
    assert api.main_header(api.make_params(64, 64, 3, 8, guard_bits=3))


def test_struct_size_of_the_older_layout_still_passes(api):
    """A caller built before the field: its struct ends behind rgb_to_xyz, and what lies beyond is not read."""
    old = api.Params.guard_bits.offset
    assert old < C.sizeof(api.Params)
    want = api.main_header(api.make_params(64, 64, 3, 8))
    p = api.make_params(64, 64, 3, 8)
    p.struct_size, p.guard_bits = old, 0xdeadbeef
    assert api.main_header(p) == want
    assert np.array_equal(api.frame_blocks(p), api.frame_blocks(api.make_params(64, 64, 3, 8)))
    for bad in (old - 4, old + 4, C.sizeof(api.Params) + 8, 12):
        p.struct_size = bad
        _refused(api, lambda: api.main_header(p), J2K_HIP_ERR_PARAM, "struct_size")


# ---------------------------------------------------------------------------------------------------------------------- headers
def _qcd(header: bytes):
    """(offset of the Sqcd byte, Sqcd) of a main header."""
    q = 2
    while header[q:q + 2] != b"\xff\x5c":
        q += 2 + int.from_bytes(header[q + 2:q + 4], "big")
    return q + 4, header[q + 4]


@pytest.mark.parametrize("kw", [dict(reversible=True, ycc=True, num_resolutions=3), dict(reversible=False, ycc=True, num_resolutions=4),
                                dict(reversible=True, num_resolutions=1), dict(reversible=False, num_resolutions=6, tile_size=64, jp2=True)],
                         ids=["53_r3", "97_r4", "53_r1", "97_r6_tiles"])
def test_main_header_differs_in_the_sqcd_byte_alone(api, kw):
    prec = 8 if kw["reversible"] else 12
    nc = 3 if kw.get("ycc") else 1
    h0 = api.main_header(api.make_params(97, 131, nc, prec, **kw))
    at, s0 = _qcd(h0)
    style = 0 if kw["reversible"] else 2
    assert s0 == style | 2 << 5
    for g in range(1, 8):
        hg = api.main_header(api.make_params(97, 131, nc, prec, guard_bits=g, **kw))
        assert len(hg) == len(h0) and hg[at] == style | g << 5
        assert [i for i in range(len(h0)) if hg[i] != h0[i]] == ([] if g == 2 else [at])
    assert api.main_header(api.make_params(97, 131, nc, prec, guard_bits=2, **kw)) == h0


@pytest.mark.parametrize("c", [gc.BY_NAME[n] for n in ("over_8_k4_r3", "limit_16_k2_r2", "over_tiles_8_k2_r2", "over_8_rand7_r6")], ids=_ids)
def test_block_table_moves_in_the_mb_column_alone(api, c):
    t0 = api.frame_blocks(gc.api_params(api, c)).astype(np.int64)
    mb = api.BLOCK_COLUMNS.index("Mb")
    for g in range(1, 8):
        for gb in (g, api.GUARD_AUTO | g):  # (a floor is where the plan starts)
            tg = api.frame_blocks(_with(api, c, gb)).astype(np.int64)
            assert np.array_equal(np.delete(tg, mb, 1), np.delete(t0, mb, 1)) and np.array_equal(tg[:, mb], t0[:, mb] + g - 2)
    assert np.array_equal(api.frame_blocks(_with(api, c, api.GUARD_AUTO)), t0)


# ---------------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("c", gc.CASES, ids=_ids)
def test_guard_bits_needed_on_the_classifiers_blocks(oracle, api, c):
    rows = gc.classify(oracle, c)
    nb, mb = np.array([b["numbps"] for b in rows]), np.array([b["Mb"] for b in rows])
    for gb in (0, 2, api.GUARD_AUTO, api.GUARD_AUTO | 2, 1, api.GUARD_AUTO | 1):
        got = api.guard_bits_needed(_with(api, c, gb), nb)
        assert got == (3 if c.expect == "over" else 2), gb
    if c.expect == "at_limit":
        assert api.guard_bits_needed(gc.api_params(api, c), nb) == int((nb - mb + 2).max()) == 2
    else:
        assert int((nb - mb + 2).max()) == 3
    # a floor above what the blocks need stands; a block deeper still takes more; beyond seven nothing holds it
    assert api.guard_bits_needed(_with(api, c, api.GUARD_AUTO | 5), nb) == 5 and api.guard_bits_needed(_with(api, c, 4), nb) == 4
    deep = nb.copy()
    k = int(np.argmax(nb - mb))
    deep[k] = mb[k] + 3
    assert api.guard_bits_needed(gc.api_params(api, c), deep) == 5
    deep[k] = mb[k] + 6
    _refused(api, lambda: api.guard_bits_needed(gc.api_params(api, c), deep), J2K_HIP_ERR_OVERFLOW, GUARD_TEXT)
    _refused(api, lambda: api.guard_bits_needed(gc.api_params(api, c), nb[:-1]), J2K_HIP_ERR_PARAM, "code-blocks")


# ---------------------------------------------------------------------------------------------------------------------- host Tier-2
@pytest.mark.parametrize("pricer", [False, True], ids=["packet_writer", "tile_pricer"])
@pytest.mark.parametrize("c", gc.OVER, ids=_ids)
def test_host_tier2_strict_counts_refuse_over_frames(oracle, api, c, pricer):
    for g in (0, 2, 1):
        _refused(api, lambda: api.host_tier2(_with(api, c, g), *_results(oracle, c), pricer=pricer), J2K_HIP_ERR_OVERFLOW, GUARD_TEXT)
        _refused(api, lambda: api.host_tier2(_with(api, c, g), *_results(oracle, c), pricer=pricer, with_guard=True), J2K_HIP_ERR_OVERFLOW, GUARD_TEXT)


@pytest.mark.parametrize("c", gc.OVER, ids=_ids)
def test_host_tier2_plans_over_frames_at_three_and_at_auto(oracle, api, c):
    r = _results(oracle, c)
    fixed = api.host_tier2(_with(api, c, 3), *r)
    assert fixed > 0
    assert api.host_tier2(_with(api, c, 3), *r, with_guard=True) == (fixed, 3)
    for auto in (api.GUARD_AUTO, api.GUARD_AUTO | 2, api.GUARD_AUTO | 1, api.GUARD_AUTO | 3):
        assert api.host_tier2(_with(api, c, auto), *r, with_guard=True) == (fixed, 3), auto
        assert api.host_tier2(_with(api, c, auto), *r) == fixed
        assert api.host_tier2(_with(api, c, auto), *r, pricer=True, with_guard=True) == (0, 3)
    assert api.host_tier2(_with(api, c, 3), *r, pricer=True) == 0
    # a floor above what the blocks need stands
    assert api.host_tier2(_with(api, c, api.GUARD_AUTO | 4), *r, with_guard=True) == (api.host_tier2(_with(api, c, 4), *r), 4)


@pytest.mark.parametrize("c", gc.AT_LIMIT, ids=_ids)
def test_host_tier2_at_limit_frames(oracle, api, c):
    r = _results(oracle, c)
    want = len(gc.oracle_file(oracle, c))
    for gb in (api.GUARD_AUTO, api.GUARD_AUTO | 2, api.GUARD_AUTO | 1):
        assert api.host_tier2(_with(api, c, gb), *r, with_guard=True) == (want, 2), gb
        assert api.host_tier2(_with(api, c, gb), *r, pricer=True, with_guard=True) == (0, 2)
    assert api.host_tier2(_with(api, c, 2), *r, with_guard=True) == (want, 2) and api.host_tier2(_with(api, c, 0), *r) == want
    for pricer in (False, True):
        _refused(api, lambda: api.host_tier2(_with(api, c, 1), *r, pricer=pricer), J2K_HIP_ERR_OVERFLOW, GUARD_TEXT)


# ---------------------------------------------------------------------------------------------------------------------- sanitizers
def test_replan_path_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "this test needs g++"
    csrc = os.path.join(ROOT, "j2k_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "native", "guard_replan_host.cpp")] + \
           [os.path.join(csrc, f) for f in ("geometry.cpp", "tier2.cpp", "jp2.cpp", "rate_control.cpp", "workers.cpp")]
    exe = str(tmp_path / "guard_replan_host")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                            "-I" + os.path.join(ROOT, "include"), *srcs, "-lpthread", "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert run.stdout.splitlines() == ["ok plain frame", "ok plain frame under a byte budget", "ok two tiles, one exceeds",
                                       "ok two tiles, one exceeds under a byte budget"]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
