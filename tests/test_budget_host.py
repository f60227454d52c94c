"""CPU: a sequence to a byte budget (j2k_hip_encode_sequence_budget_device) without a device.

  * the grid: j2k_hip_slope_grid is ldexp over the sixteen constants typed in here, strictly increasing over the whole range,
    an exact power of two at every sixteenth index, -1 for J2K_HIP_SLOPE_ALL, refused outside the range;
  * j2k_hip_encode_sequence_budget_check: every refusal by its text, and the same parameters accepted under limits of 0/0,
    N/0, 0/M and N/M;
  * nothing moves in the older ABI: the size of j2k_hip_params, the main header of three goldens;
  * tests/native/budget_host.cpp under the address and undefined-behaviour sanitizers: the search class of rate_budget.h over a
    CPU curve (rate_block.h) of the synthetic families of rate_cases.py -- monotone and spoiled tables of 1, 63, 65, 255 and
    1000 blocks read as 1, 3 and 5 frames (as many blocks as divide evenly) -- and three exact pricers: the estimate, the
    estimate plus a constant per frame, the estimate plus a wobble of 0..80 bytes keyed by (frame, index), which makes the
    length non-monotone in the index.  The limits come from the pricer's own tables.  Every cap and shared index returned is a
    member of the brute-force set of budget_model over all 4097 candidates, a second run returns the same, overflow is reported
    exactly when the set is empty, and the program's curve equals the model's (rate_model.makelayer_plain) where sampled.
    exact_plans -- whole-frame plans beyond one per frame -- is at most 3 per frame under the first two pricers, where the
    estimate is exact up to a constant, in every setting.  Under the wobble the search only has to end; its counts are printed
    (the most seen: 17 per frame, a walk across a flat stretch of the table where the wobble alone decides).
"""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import budget_model as bm
import rate_cases as rc
import rate_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
J2K_HIP_ERR_PARAM = 1

LITERALS = """0x1.0000000000000p+0 0x1.0b5586cf9890fp+0 0x1.172b83c7d517bp+0 0x1.2387a6e756238p+0
              0x1.306fe0a31b715p+0 0x1.3dea64c123422p+0 0x1.4bfdad5362a27p+0 0x1.5ab07dd485429p+0
              0x1.6a09e667f3bcdp+0 0x1.7a11473eb0187p+0 0x1.8ace5422aa0dbp+0 0x1.9c49182a3f090p+0
              0x1.ae89f995ad3adp+0 0x1.c199bdd85529cp+0 0x1.d5818dcfba487p+0 0x1.ea4afa2a490dap+0""".split()


@pytest.fixture(scope="module")
def api():
    from j2k_amd import api
    return api


# ---------------------------------------------------------------------------------------------------------------------- the grid
def test_grid_is_ldexp_over_the_sixteen_constants(api):
    m = [float.fromhex(h) for h in LITERALS]
    assert len(m) == 16 and m == [2.0 ** (j / 16) for j in range(16)]
    assert (api.SLOPE_K_MIN, api.SLOPE_K_MAX, api.SLOPE_ALL) == (-2048, 2047, -2049)
    prev = 0.0
    for k in range(api.SLOPE_K_MIN, api.SLOPE_K_MAX + 1):
        t = api.slope_grid(k)
        assert t == math.ldexp(m[k % 16], k // 16) == bm.grid(k), k
        assert t > prev and math.isfinite(t), k
        prev = t
        if k % 16 == 0:
            assert math.frexp(t)[0] == 0.5 and t == 2.0 ** (k // 16), k
    assert api.slope_grid(api.SLOPE_ALL) == -1.0
    assert 1.1e7 < api.slope_grid(377) < 1.3e7


def test_grid_is_refused_outside_the_range(api):
    for k in (api.SLOPE_ALL - 1, api.SLOPE_K_MAX + 1, 1 << 20, -(1 << 31), (1 << 31) - 1):
        with pytest.raises(api.J2kHipError) as x:
            api.slope_grid(k)
        assert x.value.code == J2K_HIP_ERR_PARAM


# ---------------------------------------------------------------------------------------------------------------------- the check
def _refused(api, p, nframes, budget, *words):
    with pytest.raises(api.J2kHipError) as x:
        api.sequence_budget_check(p, nframes, budget)
    assert x.value.code == J2K_HIP_ERR_PARAM and all(w in str(x.value) for w in words), str(x.value)


LIMITS = [(0, 0), (100000, 0), (0, 30000), (100000, 30000)]


def test_check_refuses_by_field(api):
    mk = lambda **kw: api.make_params(200, 150, 3, 10, reversible=False, ycc=True, num_resolutions=5, **kw)
    for total, frame_max in LIMITS:
        b = api.make_budget(total, frame_max)
        api.sequence_budget_check(mk(), 4, b)
        api.sequence_budget_check(mk(layers=1), 1, b)
        _refused(api, mk(layers=2), 4, b, "layers")
        _refused(api, mk(rates=[20.0]), 4, b, "layer_rates")
        _refused(api, mk(psnr=[40.0]), 4, b, "layer_psnr")
        _refused(api, mk(slopes=[1.0]), 4, b, "layer_slopes")
        _refused(api, mk(slopes=[-1.0]), 4, b, "layer_slopes")
        _refused(api, mk(cblk_style=1), 4, b, "cblk_style")
        _refused(api, mk(guard_bits=0x100), 4, b, "guard_bits", "J2K_HIP_GUARD_AUTO")
        _refused(api, mk(guard_bits=0x103), 4, b, "guard_bits", "J2K_HIP_GUARD_AUTO")
        _refused(api, api.make_params(512, 270, 3, 12, reversible=False, ycc=True, dci_profile=3), 4, b, "dci_profile")
        _refused(api, mk(), 0, b, "nframes")
        for size in (C.sizeof(api.Budget) - 8, C.sizeof(api.Budget) + 8, 0):
            bad = api.make_budget(total, frame_max)
            bad.struct_size = size
            _refused(api, mk(), 4, bad, "j2k_hip_budget", "struct_size")
        flagged = api.make_budget(total, frame_max)
        flagged.flags = 1
        _refused(api, mk(), 4, flagged, "flags")


def test_check_accepts_what_layer_slopes_combines_with(api):
    for kw in (dict(tile_size=32), dict(precincts=[(32, 32), (16, 16)]), dict(progression=4), dict(sub=[(1, 1), (2, 2), (2, 2)], rgb_to_sycc=True),
               dict(guard_bits=3), dict(rgb_to_xyz=1, reversible=False), dict(jp2=True)):
        for total, frame_max in LIMITS:
            api.sequence_budget_check(api.make_params(64, 64, 3, 8, **kw), 3, api.make_budget(total, frame_max))


def test_check_passes_on_what_the_parameters_are_refused_for(api):
    p = api.make_params(64, 64, 1, 8)
    p.struct_size += 4
    _refused(api, p, 2, api.make_budget(), "struct_size")
    _refused(api, api.make_params(64, 64, 1, 8, guard_bits=9), 2, api.make_budget(), "guard_bits")


# ---------------------------------------------------------------------------------------------------------------------- the old ABI
def test_nothing_moves_in_the_old_abi(api, golden):
    assert C.sizeof(api.Params) == 464
    assert api.load_library().j2k_hip_abi_version() == 9
    assert (C.sizeof(api.Budget), C.sizeof(api.BudgetResult)) == (24, 32)
    for name in ("g8_c1", "g8_c3", "g8_c5"):
        g = golden[name]
        kw = g["params"]
        p = api.make_params(g["width"], g["height"], g["ncomp"], g["prec"], reversible=kw.get("reversible", True), ycc=kw.get("mct", False),
                            tile_size=kw.get("tile", 0), num_resolutions=kw.get("numres", 6))
        assert api.main_header(p).hex() == g["main_header_hex"]


# ---------------------------------------------------------------------------------------------------------------------- the program
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    srcs = [os.path.join(ROOT, "tests", "native", "budget_host.cpp"), os.path.join(ROOT, "j2k_amd", "csrc", "rate_budget.cpp")]
    exe = str(tmp_path_factory.mktemp("budget_host") / "budget_host")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I" + os.path.join(ROOT, "include"), *srcs, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    return exe


def _run(program, *args):
    r = subprocess.run([program, *args], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return r.stdout


SIZES = (1, 63, 65, 255, 1000)
FAMILIES = [(kind, n) for kind in ("mono", "spoiled") for n in SIZES]


def family(kind, n, nframes):
    """The synthetic family (rate_cases.synthetic_call needs no oracle), cut to a whole number of frames."""
    call = rc.synthetic_call(f"{kind}_{n}_budget", n, 40 + n, spoil=kind == "spoiled")
    keep = n - n % nframes
    return {k: (v[:keep] if isinstance(v, np.ndarray) else v) for k, v in call.items()}


def settings_from(tables, nframes):
    """The limits of a case, every one from the pricer's own tables: the exact sum at three interior indices and that sum
    less one; a cap that binds one frame only and a cap that binds every frame (no total: every frame is then at its cap);
    limits of 0; a limit below the coarsest length, as total and as cap; a cap and a total together."""
    t = [np.asarray(tables[f], dtype=np.int64) for f in range(nframes)]
    at = lambda k: int(sum(x[k - bm.ALL] for x in t))
    interior = [k for k in (-200, 120, 500) ]
    out = []
    for k in interior:
        out += [(at(k), 0), (max(at(k) - 1, 1), 0)]
    whole = sorted(int(x[0]) for x in t)
    one = whole[-1] - 1 if nframes == 1 or whole[-1] - 1 >= whole[-2] else 0  # below the largest frame's whole length alone
    if one > 0:
        out.append((0, one))
    out.append((0, max(min(int(x[120 - bm.ALL]) for x in t), 1)))  # (what the smallest frame takes at an interior index: binds all that are larger)
    out.append((0, 0))
    coarsest = [int(x[-1]) for x in t]
    out.append((max(sum(coarsest) - 1, 1), 0))
    out.append((0, max(max(coarsest) - 1, 1)))
    both = (at(300), max(int(max(x[300 - bm.ALL] for x in t)) - 1, 1))
    out.append(both)
    return out, len(out) - 1  # (the last one has both limits)


@pytest.mark.parametrize("kind,n", FAMILIES)
def test_search_ends_in_the_brute_force_sets(program, tmp_path, kind, n):
    worst = {}
    for nframes in (1, 3, 5):
        if n < nframes:
            continue
        call = family(kind, n, nframes)
        for pricer in (0, 1, 2):
            path = str(tmp_path / f"{kind}_{n}_{nframes}_{pricer}.bin")
            bm.write_case(path, call, nframes, pricer, [])
            tables, samples, _ = bm.read_output(_run(program, path, "tables"))
            assert sorted(tables) == list(range(nframes)) and all(len(v) == bm.NCAND for v in tables.values())
            if pricer == 0 and n <= 255:  # the program's curve is the model's
                tb = rm.Tables(call["weight"], call["comp"], call["numbps"], call["npasses"], call["pass_rate"], call["pass_dist"])
                curve = bm.Curve(tb)
                nb1 = tb.n // nframes
                assert len(samples) == nframes * len(range(0, bm.NCAND, 64))
                for f, k, body, bits in samples[::3]:
                    assert (body, bits) == curve.frame(f, nb1, k), (kind, n, nframes, f, k)
            settings, both = settings_from(tables, nframes)
            bm.write_case(path, call, nframes, pricer, settings)
            _, _, results = bm.read_output(_run(program, path))
            assert len(results) == 2 * len(settings)
            tabs = [tables[f] for f in range(nframes)]
            for r in results:
                total, frame_max = settings[r["setting"]]
                assert (r["total_limit"], r["frame_limit"]) == (total, frame_max)
                first = results[2 * r["setting"]]
                assert {k: v for k, v in r.items() if k != "run"} == {k: v for k, v in first.items() if k != "run"}  # the same on a second run
                cap_sets = [bm.valid_caps(tabs[f], frame_max) for f in range(nframes)]
                # A set is empty exactly when no index fits at all (from one that fits, walking finer ends at a boundary), so an
                # empty set must be reported as overflow.  The other way round the call goes by the coarsest candidate (the
                # contract: "if even K_MAX does not fit"); where lengths fall with the index -- the first two pricers -- that
                # is the same thing, under the wobble an interior index may fit while K_MAX does not.
                if r["status"] == 2 or any(not s for s in cap_sets):
                    assert r["status"] == 2, (kind, n, nframes, pricer, r)
                    over = [f for f in range(nframes) if tabs[f][-1] > frame_max]
                    assert over and r["smallest"] in [tabs[f][-1] for f in over]
                    if pricer < 2:
                        assert any(not s for s in cap_sets), (kind, n, nframes, pricer, r)
                    continue
                if r["status"] == 1 or not bm.valid_shared(tabs, r["cap"], total):
                    assert r["status"] == 1 and all(r["cap"][f] in cap_sets[f] for f in range(nframes)), (kind, n, nframes, pricer, r)
                    assert r["smallest"] == sum(tabs[f][-1] for f in range(nframes)) > total
                    if pricer < 2:
                        assert not bm.valid_shared(tabs, r["cap"], total), (kind, n, nframes, pricer, r)
                    continue
                assert r["status"] == 0, (kind, n, nframes, pricer, r)
                assert all(r["cap"][f] in cap_sets[f] for f in range(nframes)), (kind, n, nframes, pricer, r)
                shared = bm.valid_shared(tabs, r["cap"], total)
                assert r["shared"] in shared, (kind, n, nframes, pricer, r, sorted(shared)[:8])
                assert r["index"] == [max(r["shared"], c) for c in r["cap"]]
                lens = [tabs[f][r["index"][f] - bm.ALL] for f in range(nframes)]
                assert (not total or sum(lens) <= total) and (not frame_max or max(lens) <= frame_max)
                key = (pricer, r["setting"] == both)
                worst[key] = max(worst.get(key, 0.0), r["plans"] / nframes)
                if pricer < 2:
                    assert r["plans"] <= 3 * nframes, (kind, n, nframes, pricer, r)
                print(f"{kind}_{n} frames {nframes} pricer {pricer} limits {total}/{frame_max}: status {r['status']} shared {r['shared']} "
                      f"curve_launches {r['launches']} exact_plans {r['plans']}")
    print("most exact_plans per frame, by (pricer, both limits):", {k: round(v, 2) for k, v in sorted(worst.items())})
