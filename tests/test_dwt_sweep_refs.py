"""CPU: the references and the case tables of test_dwt_sweep.py checked on their own.

1. The oracle's forward transforms are pinned to libopenjp2 through whole files only; the sweep feeds them regions no file
   holds (lines of 1 .. 13 samples at either parity, flat and alternating fields at the top of the 18-bit range).  Two
   restatements written from T.800 F.4.8 without the oracle anchor them there: int64 for 5/3 (equal word for word, and no
   magnitude leaves int32, where the oracle computes), float64 for 9/7 (a measured bound).
2. The tables reach what they claim: the launch model of dwt_variant_cases.py, given the region hook's job tables
   (dwt_sweep_cases.region_jobs), is asked for every claim about the sweep launch and about the boundary list.
"""
import numpy as np
import pytest

import dwt_sweep_cases as S


# ------------------------------------------------------------------------------------------------ restatements
@pytest.mark.parametrize("levels", S.SWEEP_LEVELS)
def test_dwt53_int64_restatement_equals_the_oracle_inside_int32(oracle, levels):
    """Both 5/3 input planes of the sweep, every region: dwt53_int64 == oracle.dwt53, and the largest magnitude at any
    level, the sums inside the lifting steps included, stays below 2^31 (measured: 2^20 + 2, a sum inside a lifting step; the largest coefficient is 2^19)."""
    _, regions = S.region_list("sweep")
    a = S.inputs("sweep", True)
    peak = [0]
    for p in range(a.shape[0]):
        for i, (x, y, w, h, x0, y0) in enumerate(regions):
            r = a[p, y:y + h, x:x + w]
            want = S.dwt53_int64(r, levels, x0, y0, peak)
            assert np.array_equal(oracle.dwt53(r, levels, x0, y0), want), (S.INPUT_CLASSES[True][p], i, w, h, x0, y0, levels)
    print(f"dwt53 L{levels}: largest magnitude {peak[0]}")
    assert peak[0] < 1 << 31


def test_structured_plane_holds_every_pattern_at_the_top_of_the_range():
    _, regions = S.region_list("sweep")
    s = S.inputs("sweep", True)[1]
    for k in range(6):
        x, y, w, h, _, _ = regions[600 + k]  # (12 .. 13 wide)
        r = s[y:y + h, x:x + w]
        assert np.array_equal(r, S.pattern(k + 600, w, h)) and (np.abs(r).max() == S.TOP) == (k % 6 != 5), (k, w, h)
    f = S.inputs("sweep", False)
    assert f.shape[0] == 3 and np.array_equal(f[2][y:y + h, x:x + w], S.pattern(605, w, h).astype(np.float32))
    assert (f[1] == 0).mean() > 0.2 and 0 < np.abs(f[1]).max() < 2.0 ** -110


def test_dwt97_matches_float64_restatement(oracle):
    """oracle.dwt97 against dwt_sweep_cases.dwt97_float64 over the sweep (every region at 1, 2, 3 and 5 levels) on the
    standard_normal x 3000 plane.

    The error is measured against the float64 result, in units of 2^-24 of the region's largest magnitude (of the float64
    result).  Measured over the 5400 cases of the sweep: worst 10.53 units (w = 1, h = 8, origin (1, 1), 1 level).
    Bound: four times that, 42.12 units; the margin covers other seeds."""
    bound = 4 * 10.53
    worst, at = 0.0, None
    _, regions = S.region_list("sweep")
    a = S.inputs("sweep", False)[0]
    for levels in S.SWEEP_LEVELS:
        for (x, y, w, h, x0, y0) in regions:
            r = a[y:y + h, x:x + w]
            ref = S.dwt97_float64(r, levels, x0, y0)
            got = oracle.dwt97(r, levels, x0, y0).astype(np.float64)
            err = np.abs(got - ref).max() / np.abs(ref).max() * 2.0 ** 24
            if err > worst:
                worst, at = err, (w, h, x0, y0, levels)
    print(f"dwt97 against float64: worst error {worst:.2f} x 2^-24 of the region's largest magnitude at {at}")
    assert worst <= bound, (worst, at)


# ------------------------------------------------------------------------------------------------ the sweep launch
def test_region_jobs_are_the_plain_hooks_for_one_region_that_covers_the_plane():
    import dwt_variant_cases as V
    for l in range(4):
        assert S.region_jobs([(0, 0, 301, 199, 33, 7)], l, 301, 199, 3) == V.stage_dwt_jobs(301, 199, l, 33, 7, 3)
    assert S.region_jobs([(5, 6, 1, 1, 1, 1)], 1, 64, 64, 2) == []  # a single odd-phase sample: nothing is left of it


@pytest.mark.parametrize("rev", [True, False], ids=["53", "97"])
def test_sweep_launch_reaches_what_it_claims(rev):
    """Under every knob set of test_dwt_sweep: jobs smaller than the grid in both directions; the 1-D grid with a partly
    invalid last group of eight under dwt_xcd = 1 and the plain grid under dwt_xcd = 0; more than one chunk at dwt_ppc 1
    and 3, and a shorter last chunk at 3 (a chunk of one row pair cannot be short)."""
    height, regions = S.region_list("sweep")
    assert len(regions) == 1350 and height <= 1100
    for kn in S.KNOBS:
        jobs, m = S.region_launch("sweep", rev, 0, kn)
        assert len(jobs) == 1350 * len(S.INPUT_CLASSES[rev])
        assert m["small_job"], kn
        assert any(j.src_off % 4 for j in jobs) and any(j.src_off % 2 for j in jobs)  # offsets off the 16-byte grid
        if kn["dwt_xcd"]:
            assert m["xcd_form"] and m["xcd_partial"], kn
        else:
            assert not m["xcd_form"], kn
        if kn["dwt_ppc"]:
            assert m["ppc"] == kn["dwt_ppc"] and m["chunks"] > 1, kn
            assert m["short_last_chunk"] == (kn["dwt_ppc"] == 3), kn


# ------------------------------------------------------------------------------------------------ the boundary list
def _boundary(kn, level=0, rev=True):
    _, regions, twins = S.boundary_regions()
    jobs, m = S.region_launch("boundary", rev, level, kn)
    return regions, twins, jobs[:len(regions)], m["strips"][:len(regions)], m  # (plane 0: at level 0 one job per region)


def test_boundary_list_holds_every_shape_and_the_twins():
    height, regions, twins = S.boundary_regions()
    assert height <= 1300 and all(x + w < S.PLANE_W and y + h < height for (x, y, w, h, _, _) in regions)
    shapes = {(w, h, x0, y0) for (x, y, w, h, x0, y0) in regions if x % 4 == 0}
    assert shapes == {(w, h, x0, y0) for w in S.BOUNDARY_W for h in S.BOUNDARY_H for (x0, y0) in S.BOUNDARY_ORIGINS}
    assert sorted(twins) == [500, 504, 748, 752]
    for w, ids in twins.items():
        assert [regions[i][0] % 4 for i in ids] == [0, 2, 1] and all(regions[i][2:] == (w, 16, 0, 1) for i in ids)
    S._label_map("boundary")  # (asserts that no two regions overlap)


def test_boundary_list_reaches_what_it_claims():
    regions, twins, jobs, strips, m = _boundary(dict(dwt_pairs=2))
    # a fast strip with rh == 16 and casy == 1; fast and edge strips in one launch
    assert any(any(s) and j.rh == 16 and j.casy == 1 for j, s in zip(jobs, strips))
    assert {j.rh for j, s in zip(jobs, strips) if any(s)} == {16, 17} and m["fast"] and m["edge"]
    assert {len(s) for s in strips} == {1, 2, 3, 4}  # the early exit `k0 >= npx`: the grid has more strips than most jobs
    shape = {(r[2], r[3], r[4], r[5]): s for r, s in zip(regions, strips) if r[0] % 4 == 0}
    assert shape[(500, 16, 0, 1)] == [False, True, False]
    assert shape[(748, 16, 0, 1)] == [False, True, True, False]
    assert not any(shape[(500, 15, 0, 1)]) and not any(shape[(502, 16, 0, 1)]) and not any(shape[(496, 16, 0, 1)])
    # strip counts 1 and 2 on either side of 248 / 249
    for h in S.BOUNDARY_H:
        for (x0, y0) in ((0, 0), (0, 1), (2, 1)):
            assert [len(shape[(w, h, x0, y0)]) for w in (247, 248, 249, 250)] == [1, 1, 2, 2]
        assert [len(shape[(w, h, 1, 0)]) for w in (247, 248, 249)] == [1, 2, 2]  # (odd origin: one column pair more)
    # the two misaligned twins lose the fast path their aligned sibling takes
    for w, (i0, i2, i1) in twins.items():
        assert any(strips[i0]) and not any(strips[i2]) and not any(strips[i1]), w
        assert jobs[i2].src_off % 4 == 2 and jobs[i1].ll_off % 2 == 1 and jobs[i1].z_off % 2 == 1
    # one pair per lane: 120 / 121, and nothing is fast
    regions, twins, jobs, strips, m1 = _boundary(dict(dwt_pairs=1))
    shape = {(r[2], r[3], r[4], r[5]): s for r, s in zip(regions, strips) if r[0] % 4 == 0}
    for h in S.BOUNDARY_H:
        assert [len(shape[(w, h, 0, 1)]) for w in (119, 120, 121, 122)] == [1, 1, 2, 2]
    assert not m1["fast"]
    for kn in S.BOUNDARY_KNOBS:
        for rev in (True, False):
            for level in range(2):
                assert S.region_launch("boundary", rev, level, kn)[1]["fast"] == (kn["dwt_pairs"] == 2 and level == 0), (kn, level)


# ------------------------------------------------------------------------------------------------ the fused edge tiles
def test_edge_tile_formats_take_the_four_conversions_of_the_fused_kernel():
    import dwt_variant_cases as V
    frames = S.edge_tile_frames()
    assert len(frames) == 50 and {t for (_, _, t) in frames} == {16, 17}
    assert {(w - t, h - t) for (w, h, t) in frames} == {(n, m) for n in range(1, 14) for m in (n, 14 - n)}
    for fmt, variant in S.EDGE_VARIANTS.items():
        for rev in (True, False):
            for levels in (1, 3):
                for case in S.edge_tile_cases(fmt, rev, levels):
                    for wpb in (1, 4):
                        kn = dict(fused_wpb=wpb)
                        m = V.fused_launch(case, kn)
                        assert V.is_fused(case, kn) and m["variant"] == variant and m["wpb"] == wpb and m["small_job"], (case.name, kn)
                        jobs = V.hook_jobs(case, 0, True)[0]
                        assert len(jobs) == 4 and {(j.casx, j.casy) for j in jobs} == {(0, 0), (case.tile & 1, 0), (0, case.tile & 1), (case.tile & 1, case.tile & 1)}
