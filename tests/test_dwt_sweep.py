"""GPU parity tests of the forward transform at the edges of its launch shapes (run with -m gpu on an MI355X), bit-exact
through the int32 view (-0.0 is not 0.0) against oracle.dwt53 / dwt97.  test_dwt_sweep_refs.py checks the references and
what the case tables reach, on any machine.

  test_dwt_sweep                          18 widths x 15 heights x 5 origins as the 1350 regions of one plane, every
                                          (plane, region) a job of one dwt_level_kernel launch per level through
                                          Encoder.stage_dwt_regions: jobs smaller than the grid, offsets off the 16-byte
                                          grid, widths and heights 1 .. 13 against both lifting parities and the chunk length
  test_dwt_strip_and_fast_boundaries      one strip / two strips, the thresholds of the wave-uniform fast test, rh = 15 / 16
                                          / 17 at casy = 1, fast-eligible widths at misaligned offsets
  test_dwt_small_lines_one_job_per_launch the same small lines as the only job of their launches (stage_dwt)
  test_fused_edge_tiles_sweep             edge tiles 1 .. 13 wide and high, even and odd origins, through the fused level-1
                                          kernel (stage_transform), which no region hook reaches
The whole plane is compared: a word written between the regions fails the test.
"""
import numpy as np
import pytest

import dwt_sweep_cases as S
import dwt_variant_cases as V
from dwt_variant_cases import check

pytestmark = pytest.mark.gpu

TRANSFORMS = [True, False]


@pytest.fixture(scope="module")
def enc():
    from j2k_amd import api
    e = api.Encoder(0)
    yield e
    e.close()
    S.release()  # (the cached references: a hundred megabytes no later module needs)


@pytest.mark.parametrize("kn", S.KNOBS, ids=V.kid)
@pytest.mark.parametrize("levels", S.SWEEP_LEVELS)
@pytest.mark.parametrize("rev", TRANSFORMS, ids=["53", "97"])
def test_dwt_sweep(enc, oracle, rev, levels, kn):
    """Every (w, h, origin) of the sweep as a region of one plane; every input class a plane of the same call."""
    S.check_regions(oracle, enc, "sweep", rev, levels, kn)


@pytest.mark.parametrize("kn", S.BOUNDARY_KNOBS, ids=V.kid)
@pytest.mark.parametrize("levels", S.BOUNDARY_LEVELS)
@pytest.mark.parametrize("rev", TRANSFORMS, ids=["53", "97"])
def test_dwt_strip_and_fast_boundaries(enc, oracle, rev, levels, kn):
    """dwt_sweep_cases.boundary_regions: what it reaches is asserted by test_boundary_list_reaches_what_it_claims."""
    S.check_regions(oracle, enc, "boundary", rev, levels, kn)


def _small_line_inputs(rng, rev, w, h):
    """One plane per call, so the shape is the only job of its launches: random, then zeros / tiny (9/7) or the
    checkerboard at +-2^17 (5/3)."""
    if rev:
        return [rng.integers(-S.TOP + 1, S.TOP + 1, size=(1, h, w)).astype(np.int32), S.pattern(1, w, h).astype(np.int32)[None]]
    return [S.idwt_input(rng, (1, h, w), False), S.idwt_input(rng, (1, h, w), False, tiny=True)]


@pytest.mark.parametrize("rev", TRANSFORMS, ids=["53", "97"])
def test_dwt_small_lines_one_job_per_launch(enc, oracle, rev):
    """The lengths where the three warm-up row pairs of a chunk reflect more than once and reflect() is periodic, each as
    the only job of its launches (max_rw / max_rh its own)."""
    rng = np.random.default_rng(78)
    f = oracle.dwt53 if rev else oracle.dwt97
    for n in range(1, 14):
        for (x0, y0) in ((0, 0), (1, 1)):
            for (w, h) in ((n, 9), (9, n), (n, n)):
                for k, a in enumerate(_small_line_inputs(rng, rev, w, h)):
                    got, _ = enc.stage_dwt(a, 2, rev, x0, y0)
                    ref = f(a[0], 2, x0, y0)[None]
                    case = V.Case(f"stage_dwt {w}x{h} origin ({x0},{y0}) {'53' if rev else '97'} L2 input {k}", w, h, 1, rev, False, 0, 0, False, 0, 2, 0, "planes")
                    msg = V.difference(case, {}, got, ref, origin=(x0, y0))
                    if msg:
                        pytest.fail(msg, pytrace=False)


@pytest.mark.parametrize("rev", TRANSFORMS, ids=["53", "97"])
def test_region_hook_equals_plain_hook(enc, oracle, rev):
    """One region that covers the plane: the words of stage_dwt (and the oracle's)."""
    w, h, x0, y0, levels = 301, 199, 33, 7, 3
    rng = np.random.default_rng(301199)
    a = np.stack([rng.integers(-S.TOP + 1, S.TOP + 1, size=(h, w)).astype(np.int32) if rev else S.idwt_input(rng, (h, w), False) for _ in range(3)])
    plain, _ = enc.stage_dwt(a, levels, rev, x0, y0)
    got = enc.stage_dwt_regions(a, levels, rev, [(0, 0, w, h, x0, y0)])
    assert np.array_equal(got.view(np.int32), plain.view(np.int32))
    ref = np.stack([(oracle.dwt53 if rev else oracle.dwt97)(p, levels, x0, y0) for p in a])
    assert np.array_equal(got.view(np.int32), ref.view(np.int32))
    assert np.array_equal(enc.stage_dwt_regions(a, 0, rev, [(0, 0, w, h, x0, y0)]).view(np.int32), a.view(np.int32))  # no level: the input


def test_dwt_stage_rejects_bad_regions(enc):
    from j2k_amd import api, synth
    a = np.zeros((1, 32, 32), dtype=np.int32)
    ok = [(0, 0, 8, 8, 0, 0)]
    for bad, levels in (([(0, 0, 8, 0, 0, 0)], 1), ([(0, 0, 0, 8, 0, 0)], 1),                 # empty
                        ([(0, 0, 33, 8, 0, 0)], 1), ([(30, 0, 3, 8, 0, 0)], 1), ([(0, 25, 8, 8, 0, 0)], 1),  # outside the plane
                        ([(0, 0, 8, 8, 0, 0), (7, 7, 8, 8, 0, 0)], 1),                      # overlapping
                        (ok, 33),                                                            # levels > 32
                        ([], 1)):                                                            # no region
        with pytest.raises(api.J2kHipError) as ei:
            enc.stage_dwt_regions(a, levels, True, bad)
        assert ei.value.code == 1, (bad, levels)  # J2K_HIP_ERR_PARAM
    assert np.array_equal(enc.stage_dwt_regions(a, 32, True, ok), a)
    # an encode pending on the handle: refused.  A borrowed frame on its way is not disturbed (the refusal comes before the
    # handle is touched); a refusal between encode_begin and encode_end drops the pending encode, like every failed call
    pl = synth.planes(64, 48, 3, 8, 5)
    frame, lay = synth.ae_frame(pl, 8)
    p = api.make_params(64, 48, 3, 8, reversible=True, ycc=True, num_resolutions=3)
    want = enc.encode_host(frame, lay, p)
    enc.encode_begin_borrowed(frame, lay, p)
    try:
        with pytest.raises(api.J2kHipError) as ei:
            enc.stage_dwt_regions(a, 1, True, ok)
        assert ei.value.code == 1
    finally:
        cs = enc.encode_end()
    assert cs == want
    enc.encode_begin_host(frame, lay, p)
    with pytest.raises(api.J2kHipError, match="has not been finished") as ei:
        enc.stage_dwt_regions(a, 1, True, ok)
    assert ei.value.code == 1
    # and the hook leaves the handle fit for the next encode
    enc.stage_dwt_regions(a, 1, True, ok)
    assert enc.encode_host(frame, lay, p) == want


# ------------------------------------------------------------------------------------------------ the fused level-1 kernel
@pytest.mark.parametrize("levels", [1, 3])
@pytest.mark.parametrize("rev", TRANSFORMS, ids=["53", "97"])
@pytest.mark.parametrize("fmt", list(S.EDGE_FORMATS), ids=list(S.EDGE_FORMATS))
def test_fused_edge_tiles_sweep(enc, oracle, fmt, rev, levels):
    """Frames of (t + n) x (t + m) in tiles of t: edge tiles n wide, m high and n x m, n = 1 .. 13, at even (t = 16) and odd
    (t = 17) origins, one and four waves per workgroup, in the four sample conversions of the fused kernel."""
    for case in S.edge_tile_cases(fmt, rev, levels):
        for wpb in (1, 4):
            check(oracle, enc, case, dict(fused_wpb=wpb))
