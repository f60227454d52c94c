"""GPU parity tests of the forward transform at coefficient level (run with -m gpu on an MI355X): the fused level-1 kernel in
every instantiation, real job tables (tiles, edge tiles, odd origins, strided planes), the launch knobs that "never change
a byte", and launches over row-pair ranges -- all bit-exact (np.array_equal on the int32 view, so -0.0 is not 0.0) against
dwt_variant_cases.reference, through Encoder.stage_transform (the encoder's own front end and DWT launches) and stage_dwt.
test_dwt_variant_refs.py checks the reference and what the cases reach, on any machine.

Which case reaches which template instantiation (test_every_fused_instantiation_has_a_case and
test_level_kernel_cases_... assert this table from the launch model):

  dwt_fused_kernel<REV, NCOMP, GEN, SPEC, WPB>          test_fused_level1_matches_reference[...]
    REV true / false                                     ids 53-... / 97-...
    NCOMP 1 / 3 / 4                                      ids ...-c1-, -c3- / -c3m-, -c4- / -c4m-  (m: with the colour transform)
    generic (GEN false, SPEC 0)                          -16to10, -16to12 (right shift); -8to8-generic, -16to16-generic
                                                         (fused_generic = 1); every -c1- case without Promote / up-shift
    GEN true                                             -8to10, -8to12, -8to16 (up-shift); -16to16p, -16to12p (Promote)
    SPEC 1 (ARGB64), SPEC 2 (ARGB32), NCOMP 3 / 4        -16to16, -8to8
    WPB 1 / 4                                            [..., fused_wpb=1 / 4, ...]
    fast and edge strips, both in one workgroup          frames 1016 x 40 (no fast strip with padded rows: +pad4, +pad8)
  dwt_level_kernel<REV, PAIRS>, fast / edge strips       test_level_kernel_knobs_stage_dwt[53 / 97, dwt_pairs=1 / 2, ...]:
                                                         1000 x 37 and 748 x 33 have fast strips under PAIRS 2, none under 1;
                                                         test_level_kernel_knobs_tiled_hook: 1100 x 70 in tiles of 512
  frontend_kernel with dst_x0 / dst_y0, strided planes   test_tiles_match_reference[..., no_fuse] and [...-planar8,16to...]

An untiled frame narrower or lower than 2^levels is refused by the encoder, as by the reference: 1 x 40, 40 x 1 and
their like run as the edge tiles of small tiled frames (dwt_variant_cases.fused_shapes), at even and at odd origins.
"""
import numpy as np
import pytest

import dwt_variant_cases as V
from conftest import golden_case
from dwt_variant_cases import check, knobs, run_hook  # (shared with test_dwt_sweep.py)
from j2k_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def enc():
    from j2k_amd import api
    e = api.Encoder(0)
    yield e
    e.close()


def _api():
    from j2k_amd import api
    return api


# ------------------------------------------------------------------------------------------------ the fused level-1 kernel
@pytest.mark.parametrize("fmt,kn", [pytest.param(f, kn, id=f"{V.fmt_id(f)}-{V.kid(kn)}") for f in V.FUSED_FORMATS for kn in V.FUSED_KNOBS])
def test_fused_level1_matches_reference(enc, oracle, fmt, kn):
    """One sample format x one launch shape on every frame of fused_shapes, at one and at three levels."""
    for case in V.fused_cases(fmt):
        check(oracle, enc, case, V.fused_knobs(fmt, kn))


# ------------------------------------------------------------------------------------------------ tiles
@pytest.mark.parametrize("mode", list(V.TILE_MODES))
@pytest.mark.parametrize("case", V.tile_cases(True) + V.tile_cases(False), ids=lambda c: c.name)
def test_tiles_match_reference(enc, oracle, case, mode):
    """One job per tile(-component): edge tiles smaller than the grid, odd tile origins (tiles of 75), z_off per tile, planes
    of stride 320 / 1152 -- fused, unfused (no_fuse = 1) and from planar channel views of unequal sample size."""
    check(oracle, enc, case, V.TILE_MODES[mode])


# ------------------------------------------------------------------------------------------------ the level kernel's knobs
_dwt_refs = {}


def _dwt_ref(oracle, shape, rev):
    """(input, reference) of a stage_dwt shape: computed once, shared by every knob set, never written."""
    if (shape, rev) not in _dwt_refs:
        w, h, levels, x0, y0 = shape
        rng = np.random.default_rng(w * 1000 + h)
        if rev:
            a = rng.integers(-40000, 40000, size=(V.DWT_PLANES, h, w), dtype=np.int32)
            ref = np.stack([oracle.dwt53(a[i], levels, x0, y0) for i in range(V.DWT_PLANES)])
        else:
            a = (rng.standard_normal((V.DWT_PLANES, h, w)) * 3000).astype(np.float32)
            ref = np.stack([oracle.dwt97(a[i], levels, x0, y0) for i in range(V.DWT_PLANES)])
        a.setflags(write=False)
        ref.setflags(write=False)
        _dwt_refs[(shape, rev)] = (a, ref)
    return _dwt_refs[(shape, rev)]


def _check_stage_dwt(enc, oracle, shape, rev, kn):
    w, h, levels, x0, y0 = shape
    a, ref = _dwt_ref(oracle, shape, rev)
    with knobs(kn):
        got, _ = enc.stage_dwt(a, levels, rev, x0, y0)
    case = V.Case(f"stage_dwt {w}x{h} origin ({x0},{y0}) {'53' if rev else '97'} L{levels}", w, h, V.DWT_PLANES, rev, False, 0, 0, False, 0, levels, 0, "planes")
    msg = V.difference(case, kn, got, ref, origin=(x0, y0))
    if msg:
        pytest.fail(msg, pytrace=False)


@pytest.mark.parametrize("kn", V.LEVEL_KNOBS, ids=V.kid)
@pytest.mark.parametrize("rev", [True, False], ids=["53", "97"])
def test_level_kernel_knobs_stage_dwt(enc, oracle, rev, kn):
    for shape in V.DWT_SHAPES:
        _check_stage_dwt(enc, oracle, shape, rev, kn)


@pytest.mark.parametrize("kn", V.LADDER_KNOBS, ids=V.kid)
@pytest.mark.parametrize("rev", [True, False], ids=["53", "97"])
def test_level_kernel_chunk_ladder(enc, oracle, rev, kn):
    """dwt_min_waves between the wave counts of neighbouring steps: chunks of 128, 64, 32, 16, 8 and 4 row pairs on 513 x 515."""
    _check_stage_dwt(enc, oracle, (513, 515, 6, 0, 0), rev, kn)


@pytest.mark.parametrize("kn", V.LEVEL_KNOBS, ids=V.kid)
@pytest.mark.parametrize("case", V.LEVEL_HOOK_CASES, ids=lambda c: c.name)
def test_level_kernel_knobs_tiled_hook(enc, oracle, case, kn):
    """The same knobs on the encoder's own job tables: every level through dwt_level_kernel on strided planes."""
    check(oracle, enc, case, kn if case.views == "planar" else dict(kn, no_fuse=1))


# ------------------------------------------------------------------------------------------------ partitions
@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
@pytest.mark.parametrize("cutset", ["every", "first", "last", "2,3,17", "per-level"])
@pytest.mark.parametrize("fuse", ["fused", "no_fuse"])
@pytest.mark.parametrize("rev", [True, False], ids=["53", "97"])
@pytest.mark.parametrize("frame", V.PARTITION_FRAMES, ids=lambda f: f"{f[0]}x{f[1]}/t{f[2]}")
def test_any_partition_gives_the_same_coefficients(enc, oracle, frame, rev, fuse, cutset, descending):
    """DwtLevelArgs::pair0 / pair1: a level launched in pieces, in either order, equals the reference -- and so the uncut launch."""
    case = V.partition_case(frame, rev)
    check(oracle, enc, case, V.TILE_MODES[fuse], V.cut_sets(case)[cutset], descending)


def test_bad_cut_points_are_parameter_errors(enc):
    api = _api()
    case = V.partition_case(V.PARTITION_FRAMES[0], True)
    n0 = V.level_pairs(case, 0)
    for cuts in ([[n0]], [[0]], [[3, 3]], [[5, 2]], [[1], [1], [1], [1]], [[], [V.level_pairs(case, 1)]]):
        with pytest.raises(api.J2kHipError) as ei:
            run_hook(enc, case, {}, cuts)
        assert ei.value.code == 1, cuts  # J2K_HIP_ERR_PARAM


# ------------------------------------------------------------------------------------------------ the handle afterwards
def test_hook_does_not_poison_the_handle(enc, oracle, golden):
    """stage_transform of another geometry, then a normal encode on the same handle: the golden's bytes."""
    api = _api()
    g, pl, _, cs = golden_case(golden, "g3_300x200_rgb8_53_rct")
    frame, lay = synth.ae_frame(pl, g["prec"], row_pad_bytes=8)
    kw = g["params"]
    p = api.make_params(g["width"], g["height"], g["ncomp"], g["prec"], reversible=kw.get("reversible", True), ycc=kw.get("mct", False),
                        layers=kw.get("layers", 1), tile_size=kw.get("tile", 0), num_resolutions=kw.get("numres", 6),
                        cblk=tuple(kw.get("cblk", (64, 64))), comment="")
    assert enc.encode_host(frame, lay, p) == cs
    for case in (V.ae_case(301, 199, 3, False, True, 8, 8, False, 0, 3, 75), V.ae_case(300, 200, 3, True, True, 8, 8, False, 0, kw.get("numres", 6) - 1, kw.get("tile", 0))):
        check(oracle, enc, case, {})
        assert enc.encode_host(frame, lay, p) == cs, case.name
        d = enc.upload(frame)
        try:
            assert enc.encode_device(d, lay, p)[2] == cs, case.name
        finally:
            enc.free(d)
