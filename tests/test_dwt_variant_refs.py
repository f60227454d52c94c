"""CPU: the reference and the case table of test_dwt_variants.py checked on their own.

1. The composition is right: for every reversible case the oracle's inverse transform of every tile rectangle, the inverse
   RCT and the DC shift give back the samples as numpy computes them from the frame (no oracle in that); for the 9/7
   cases the untiled reference equals oracle.dwt97 of the whole plane.
2. The table reaches what it claims: the launch model of dwt_variant_cases.py (the wave-uniform predicates of
   dwt_level_kernel, dwt_fused_kernel and level_grid in Python) is asked for every claim -- fast and edge strips, both
   in one workgroup of four, the 1-D grid with a partly invalid last group, a shorter last chunk, jobs smaller than the
   grid -- and for the set of template instantiations the GPU cases launch.
"""
import numpy as np
import pytest

import dwt_variant_cases as V


def _all_hook_cases():
    seen, out = set(), []
    lists = [c for f in V.FUSED_FORMATS for c in V.fused_cases(f)] + V.tile_cases(True) + V.tile_cases(False) + V.LEVEL_HOOK_CASES + \
            [V.partition_case(fr, rev) for fr in V.PARTITION_FRAMES for rev in (True, False)]
    for c in lists:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


ALL = _all_hook_cases()


def _inverse(oracle, case, ref):
    out = np.empty_like(ref)
    for (x0, y0, x1, y1) in V.tiles(case):
        for c in range(case.nc):
            out[c, y0:y1, x0:x1] = oracle.idwt53(ref[c, y0:y1, x0:x1], case.levels, x0, y0)
    out = out.astype(np.int64)
    if case.mct:
        y, cb, cr = out[0].copy(), out[1].copy(), out[2].copy()
        g = y - ((cb + cr) >> 2)
        out[0], out[1], out[2] = cr + g, g, cb + g
    return out + (1 << (case.prec - 1))


@pytest.mark.parametrize("fmt", [f for f in V.FUSED_FORMATS if f.rev and not f.generic], ids=V.fmt_id)
def test_reversible_reference_inverts_to_the_input_fused_shapes(oracle, fmt):
    for case in V.fused_cases(fmt):
        assert np.array_equal(_inverse(oracle, case, V.reference(oracle, case)), V.make_input(case).samples), case.name


@pytest.mark.parametrize("case", [c for c in ALL if c.rev and (c.tile and c.w > 50 or c.w == 1016 and c.h == 70)], ids=lambda c: c.name)
def test_reversible_reference_inverts_to_the_input_tiles(oracle, case):
    assert np.array_equal(_inverse(oracle, case, V.reference(oracle, case)), V.make_input(case).samples)


@pytest.mark.parametrize("case", [c for c in ALL if not c.rev and not c.tile], ids=lambda c: c.name)
def test_untiled_97_reference_is_the_transform_of_the_whole_plane(oracle, case):
    fe = V.frontend_reference(oracle, case).view(np.float32)
    ref = V.reference(oracle, case)
    for c in range(case.nc):
        assert np.array_equal(ref[c].view(np.int32), oracle.dwt97(fe[c], case.levels).view(np.int32))


def test_97_frontend_words_are_the_floats_of_the_shifted_samples(oracle):
    """Without the colour transform the 9/7 front end is (float)(sample - dc): the reference's words are float patterns."""
    case = V.ae_case(301, 37, 4, False, False, 16, 12, False, 0, 1, 0)
    fe = V.frontend_reference(oracle, case).view(np.float32)
    assert np.array_equal(fe, (V.make_input(case).samples - (1 << 11)).astype(np.float32))


# ------------------------------------------------------------------------------------------------ the table's claims
def _gpu_items():
    """Every (case, knobs) the hook tests of test_dwt_variants.py run."""
    items = set()
    for f in V.FUSED_FORMATS:
        for kn in V.FUSED_KNOBS:
            for c in V.fused_cases(f):
                items.add((c, V.kid(V.fused_knobs(f, kn))))
    for rev in (True, False):
        for c in V.tile_cases(rev):
            for kn in V.TILE_MODES.values():
                items.add((c, V.kid(kn)))
    return items


@pytest.mark.parametrize("item", V.claimed(), ids=lambda it: f"{it[0].name}[{V.kid(it[1])}]")
def test_case_reaches_what_it_claims(item):
    case, kn, claims = item
    assert (case, V.kid(kn)) in _ITEMS, "the claim is about a launch no GPU test runs"
    facts = V.claim_facts(case, kn)
    assert claims <= facts, (sorted(claims - facts), [dict(m, strips=None) for m in V.hook_launches(case, kn)])


_ITEMS = _gpu_items()


def test_small_frames_get_the_same_fused_launch_whatever_the_occupancy():
    """launch_fused sizes its chunks by the kernels' register counts as built; for the frames of these tests every
    occupancy 1..8 gives the launch the model assumes, so the claims do not hang on a compiler version."""
    for f in V.FUSED_FORMATS[::7]:
        for case in V.fused_cases(f):
            if not V.is_fused(case, {}):
                continue
            for kn in V.FUSED_KNOBS:
                base = V.fused_launch(case, kn)
                for occ in range(1, 9):
                    m = V.fused_launch(case, kn, occ)
                    assert (m["ppc"], m["wpb"], m["chunks"]) == (base["ppc"], base["wpb"], base["chunks"]), (case.name, kn, occ)


def test_fused_ppc_values_give_the_chunk_lengths_they_name():
    case = V.ae_case(1016, 40, 3, True, True, 8, 8, False, 0, 1, 0)
    assert [V.fused_launch(case, kn)["ppc"] for kn in V.FUSED_KNOBS[:5]] == [4, 1, 3, 8, 20]
    # (the grid is sized by (max_rh + 2) / 2 = 21 row pairs, the job has 20: where 20 is a multiple, a last chunk leaves at once)
    assert [V.fused_launch(case, kn)["chunks"] for kn in V.FUSED_KNOBS[:5]] == [6, 21, 7, 3, 2]


def test_every_fused_instantiation_has_a_case():
    """{5/3, 9/7} x {1, 3, 4 components} x {generic, GEN, SPEC1, SPEC2 where they exist} x {1, 4 waves}."""
    want = {(rev, nc, v, wpb) for rev in (True, False) for nc in (1, 3, 4) for wpb in (1, 4)
            for v in (("generic", "GEN") if nc == 1 else ("generic", "GEN", "SPEC1", "SPEC2"))}
    got = set()
    for f in V.FUSED_FORMATS:
        for kn in V.FUSED_KNOBS:
            k = V.fused_knobs(f, kn)
            for case in V.fused_cases(f):
                if V.is_fused(case, k):
                    m = V.fused_launch(case, k)
                    got.add((f.rev, f.nc, m["variant"], m["wpb"]))
    assert got == want, (sorted(want - got), sorted(got - want))


def test_level_kernel_cases_meet_fast_and_edge_strips_and_lose_the_fast_ones_with_one_pair_per_lane():
    """{5/3, 9/7} x {PAIRS 1, 2} x {fast, edge} (PAIRS 1 has no fast path), through stage_dwt and through the tiled hook."""
    for (w, h, levels, x0, y0) in [(1000, 37, 5, 0, 0), (748, 33, 2, 0, 0)]:
        jobs = V.stage_dwt_jobs(w, h, 0, x0, y0, V.DWT_PLANES)
        m2, m1 = V.level_launch(jobs, dict(dwt_pairs=2), w), V.level_launch(jobs, dict(dwt_pairs=1), w)
        assert m2["fast"] and m2["edge"] and not m1["fast"] and m1["edge"]
        assert [sum(r) for r in m2["strips"]] == [3 if w == 1000 else 2] * V.DWT_PLANES
    assert any(kn["dwt_pairs"] == 1 for kn in V.LEVEL_KNOBS) and any(kn["dwt_pairs"] == 2 for kn in V.LEVEL_KNOBS)
    for case in V.LEVEL_HOOK_CASES:
        kn = {} if case.views == "planar" else dict(no_fuse=1)
        assert not V.is_fused(case, kn)
        if case.w == 1100:
            assert any(m["fast"] for m in V.hook_launches(case, kn)) and not any(m["fast"] for m in V.hook_launches(case, dict(kn, dwt_pairs=1)))


def test_level_knobs_walk_the_chunk_ladder_and_both_grids():
    jobs = V.stage_dwt_jobs(513, 515, 0, 0, 0, V.DWT_PLANES)
    assert [V.level_launch(jobs, kn, 513)["ppc"] for kn in V.LADDER_KNOBS] == [128, 64, 32, 16, 8, 4]
    ppcs, forms, partial, short = set(), set(), False, False
    for kn in V.LEVEL_KNOBS:
        for (w, h, levels, x0, y0) in V.DWT_SHAPES:
            for l in range(levels):
                jobs = V.stage_dwt_jobs(w, h, l, x0, y0, V.DWT_PLANES)
                if jobs:
                    m = V.level_launch(jobs, kn, w)
                    ppcs.add(m["ppc"]); forms.add(m["xcd_form"]); partial |= m["xcd_partial"]; short |= m["short_last_chunk"]
    assert ppcs >= {1, 3, 4, 7, 128} and forms == {False, True} and partial and short
    # the long chunks of the stand-alone 9/7 level kernel (above 16 row pairs) with more than one of them
    m = V.level_launch(V.stage_dwt_jobs(513, 515, 0, 0, 0, V.DWT_PLANES), dict(dwt_min_waves=1), 513)
    assert m["ppc"] == 128 and m["chunks"] == 3 and m["short_last_chunk"]


def test_cut_sets_lie_inside_their_levels():
    for fr in V.PARTITION_FRAMES:
        case = V.partition_case(fr, True)
        n = [V.level_pairs(case, l) for l in range(case.levels)]
        assert n[0] == (35 if fr[2] == 0 else 50)
        for name, cuts in V.cut_sets(case).items():
            for l, c in enumerate(cuts):
                assert c == sorted(set(c)) and c[0] >= 1 and c[-1] < n[l], (name, l)
