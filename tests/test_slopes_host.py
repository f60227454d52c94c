"""CPU: layers at given slope thresholds (j2k_hip_params.layer_slopes) as far as they go without a device.

  * the parameter: what is refused and with which text, what is accepted, the older struct sizes, the main header;
  * tests/native/slopes_host.cpp as a stand-alone program under the address and undefined-behaviour sanitizers: the slopes
    allocation laid out at the thresholds the plain procedure reports is the plain procedure's allocation (read-back and replay,
    one tile and several);
  * the multi-layer model (tests/slopes_model.py, over rate_model.makelayer_plain) against the same program's per-block routine
    on the families of tests/rate_cases.py, pass counts and bytes, at thresholds that are negative, 0, 1e-300, just below and at
    DBL_EPSILON, equal to a run's slope and one ulp either side, and 1e300.
"""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import rate_cases as rc
import slopes_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
J2K_HIP_ERR_PARAM = 1


@pytest.fixture(scope="module")
def api():
    from j2k_amd import api
    return api


def _refused(api, call, *words):
    with pytest.raises(api.J2kHipError) as ei:
        call()
    assert ei.value.code == J2K_HIP_ERR_PARAM and all(w in str(ei.value) for w in words), str(ei.value)


# ---------------------------------------------------------------------------------------------------------------------- parameters
def test_values_that_are_refused_name_the_field(api):
    for bad in (math.nan, math.inf, -math.inf):
        for sl in ([bad], [1.0, bad, 0.5], [0.5, 0.25, bad]):
            _refused(api, lambda: api.main_header(api.make_params(64, 64, 1, 8, slopes=sl)), "layer_slopes", "finite")
            _refused(api, lambda: api.frame_blocks(api.make_params(64, 64, 1, 8, slopes=sl)), "layer_slopes")
    _refused(api, lambda: api.main_header(api.make_params(64, 64, 1, 8, slopes=[1.0] * 101)), "layer_slopes", "100 layers")


def test_the_other_allocations_and_styles_are_excluded(api):
    _refused(api, lambda: api.main_header(api.make_params(64, 64, 1, 8, slopes=[1.0], rates=[20])), "layer_rates and layer_slopes exclude each other")
    _refused(api, lambda: api.main_header(api.make_params(64, 64, 1, 8, slopes=[1.0], psnr=[30])), "layer_psnr and layer_slopes exclude each other")
    _refused(api, lambda: api.main_header(api.make_params(64, 64, 1, 8, slopes=[1.0], cblk_style=1)), "cblk_style cannot be combined with layer_slopes")
    _refused(api, lambda: api.main_header(api.make_params(512, 270, 3, 12, reversible=False, ycc=True, dci_profile=3, slopes=[1.0])),
             "layer_slopes cannot be combined with dci_profile")


def test_negative_and_unordered_entries_are_accepted(api):
    for sl in ([-1.0], [-1.0, -1.0, -1.0], [0.0], [1e-300, 1e300], [0.5, 2.0, 1.0], [3.0, -1.0, 1.0], [-0.0, 5e-324], [1.0] * 100):
        assert api.main_header(api.make_params(64, 64, 1, 8, slopes=sl))


def test_what_layer_rates_combines_with_is_accepted(api):
    for kw in (dict(tile_size=32), dict(precincts=[(32, 32), (16, 16)]), dict(progression=4), dict(sub=[(1, 1), (2, 2), (2, 2)], rgb_to_sycc=True),
               dict(guard_bits=3), dict(rgb_to_xyz=1, reversible=False)):
        p = api.make_params(64, 64, 3, 8, slopes=[2.0, 0.5], **kw)
        assert api.main_header(p) == api.main_header(api.make_params(64, 64, 3, 8, rates=[20, 10], **kw))


def test_the_header_is_that_of_rates_with_the_same_layer_count(api):
    """COD carries only the layer count."""
    for layers in (1, 3, 100):
        want = api.main_header(api.make_params(200, 150, 3, 10, reversible=False, ycc=True, rates=[float(1000 - 9 * i) for i in range(layers)]))
        assert api.main_header(api.make_params(200, 150, 3, 10, reversible=False, ycc=True, slopes=[float(i) for i in range(layers)])) == want
        assert api.main_header(api.make_params(200, 150, 3, 10, reversible=False, ycc=True, layers=layers)) == want


def test_older_struct_sizes_read_as_no_slopes(api):
    """Accepted: this header's size, the size before layer_slopes (guard_bits and the padding behind it) and the size before
    guard_bits; what lies beyond the caller's size is not read -- a garbage pointer there is never followed."""
    before_slopes, before_guard = api.Params.layer_slopes.offset, api.Params.guard_bits.offset
    assert before_guard < before_slopes < C.sizeof(api.Params) and before_slopes % C.sizeof(C.c_void_p) == 0
    want = api.main_header(api.make_params(64, 64, 3, 8, layers=2))
    want3 = api.main_header(api.make_params(64, 64, 3, 8, layers=2, guard_bits=3))
    for size in (before_slopes, before_guard):
        p = api.make_params(64, 64, 3, 8, layers=2, guard_bits=3)
        p.struct_size = size
        p.layer_slopes = C.cast(C.c_void_p(0xdead0008), C.POINTER(C.c_double))
        assert api.main_header(p) == (want3 if size == before_slopes else want)
        assert np.array_equal(api.frame_blocks(p), api.frame_blocks(api.make_params(64, 64, 3, 8, layers=2, guard_bits=3 if size == before_slopes else 0)))
    p = api.make_params(64, 64, 3, 8, layers=2)
    for bad in (before_guard - 4, before_guard + 4, before_slopes + 4, C.sizeof(api.Params) + 8, 12, 0):
        p.struct_size = bad
        _refused(api, lambda: api.main_header(p), "struct_size")


# ---------------------------------------------------------------------------------------------------------------------- the program
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    csrc = os.path.join(ROOT, "j2k_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "native", "slopes_host.cpp")] + \
           [os.path.join(csrc, f) for f in ("geometry.cpp", "tier2.cpp", "jp2.cpp", "rate_control.cpp", "workers.cpp")]
    exe = str(tmp_path_factory.mktemp("slopes_host") / "slopes_host")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I" + os.path.join(ROOT, "include"), *srcs, "-lpthread", "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    return exe


def _run(program, *args):
    r = subprocess.run([program, *args], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return r.stdout


def test_read_back_and_replay_under_sanitizers(program):
    out = _run(program)
    lines = [ln for ln in out.splitlines() if ln.startswith("ok replay")]
    assert len(lines) == 16
    assert any("layers100" in ln for ln in lines) and any(" in 1 tiles" in ln for ln in lines) and any("psnr" in ln for ln in lines)
    assert sum(" in 1 tiles" not in ln for ln in lines) >= 4 and any("spoiled" in ln for ln in lines)


@pytest.fixture(scope="module")
def all_calls(oracle):
    return rc.calls(oracle)


@pytest.mark.parametrize("name", rc.CALL_NAMES)
def test_model_equals_the_host_path(program, all_calls, tmp_path, name):
    call = all_calls[name]
    n = len(call["npasses"])
    want = sm.model(call)
    lists = [sl for sl, _, _ in want]
    assert sorted(set(len(sl) for sl in lists)) == list(sm.LAYER_COUNTS)
    flat = [v for sl in lists for v in sl]
    assert any(v < 0 for v in flat) and 0.0 in flat and 1e-300 in flat and sm.EPS in flat and 1e300 in flat
    path = str(tmp_path / f"{name}.case")
    sm.write_case(path, call, lists)
    got = sm.read_output(_run(program, path), n, lists)
    for k, (sl, passes, nbytes) in enumerate(want):
        assert np.array_equal(got[k][0], passes), (name, k, sl[:8])
        assert np.array_equal(got[k][1], nbytes), (name, k, sl[:8])
        assert (passes <= np.asarray(call["npasses"])[:, None]).all() and (np.diff(passes.astype(int), axis=1) >= 0).all()
        neg = [l for l, v in enumerate(sl) if v < 0]
        if neg:  # a negative threshold takes everything that is left
            assert (passes[:, neg[0]:] == np.asarray(call["npasses"], dtype=np.uint8)[:, None]).all()


def test_the_epsilon_edge_by_hand(program, tmp_path):
    """Block 0: weight 64, one bit-plane, one pass of 4 bytes with nmsedec 16: w = 64, distortion 64 * (64 * 16 / 8192) = 8, slope
    2.  A threshold equal to the slope takes the pass (0 < DBL_EPSILON); one ulp above does not (an ulp of 2 is 4.4e-16, more
    than DBL_EPSILON); one ulp below does; a threshold just below DBL_EPSILON takes every pass with bytes whatever its slope.
    Block 1: two bit-planes, pass 0 in plane 1 (w = 128: 128 * (128 * 16 / 8192) = 32 over 4 bytes, slope 8), pass 1 with 6
    bytes and no distortion (slope 0): taken just below DBL_EPSILON, not at it."""
    call = rc._pack("edge", [(64.0, 0, 1, [4], [16]), (64.0, 0, 2, [4, 10], [16, 0])], True)
    tb = rc.tables(call)
    s = tb.disto[0][0] / 4
    assert tb.disto[0] == [8.0] and s == 2.0 and tb.disto[1] == [32.0, 32.0]
    up, down = float(np.nextafter(s, np.inf)), float(np.nextafter(s, -np.inf))
    below_eps = float(np.nextafter(sm.EPS, 0.0))
    lists = [[s], [up], [down], [below_eps], [sm.EPS], [1e300, up, s]]
    path = str(tmp_path / "edge.case")
    sm.write_case(path, call, lists)
    got = sm.read_output(_run(program, path), 2, lists)
    assert [int(got[k][0][0, 0]) for k in range(5)] == [1, 0, 1, 1, 1]
    assert [int(got[k][0][1, 0]) for k in range(5)] == [1, 1, 1, 2, 1]
    assert got[5][0][0].tolist() == [0, 0, 1] and got[5][1][0].tolist() == [0, 0, 4]
    for k, sl in enumerate(lists):
        for b in range(2):
            assert got[k][0][b].tolist() == sm.layers_plain(tb.rate[b], tb.disto[b], sl)[0]
