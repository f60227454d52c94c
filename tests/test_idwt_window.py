"""The windowed inverse DWT of a region decode in isolation (run with -m gpu): idwt_win_h_kernel + idwt_win_v_kernel through
j2k_hip_stage_idwt_window against oracle.idwt53 / idwt97, word for word.

The input is poisoned OUTSIDE the rectangles of j2k_hip_region_footprint -- ints near 2^30 for 5/3, NaN patterns for 9/7 --
and the window of the result must equal the window of the oracle's transform of the UNPOISONED plane: one comparison
shows that the kernels compute the right values and that they read nothing they were not promised.  A guard row before
and behind the planes, in the same allocation, must keep its fill.  Shapes and windows: region_cases.py."""
import numpy as np
import pytest

import region_cases as rc
from j2k_amd import api

pytestmark = pytest.mark.gpu

GUARD = 0x5ca1ab1e


@pytest.fixture(scope="module")
def enc():
    e = api.Encoder(0)
    yield e
    e.close()


@pytest.mark.parametrize("case", rc.CASES, ids=rc.case_id)
def test_window_matches_oracle_and_reads_only_its_footprint(enc, oracle, case):
    w, h, x0, y0, levels, rev = case
    rng = np.random.default_rng(2000 * w + 10 * levels + x0 + int(rev))
    a = np.stack([rc.plane(rng, w, h, rev), rc.plane(rng, w, h, rev)])
    f = oracle.idwt53 if rev else oracle.idwt97
    want = np.stack([f(p, levels, x0, y0) for p in a]).view(np.int32)
    for win in rc.windows(w, h, seed=w + levels):
        mask = rc.footprint_mask(api.region_footprint(w, h, levels, rev, win, x0, y0), w, h)
        bad = np.stack([rc.poison(p, mask, rev, rng, hard=True) for p in a])
        got, before, behind = enc.stage_idwt_window(bad, levels, rev, win, x0, y0, guard=GUARD)
        x, y, ww, wh = win
        assert np.array_equal(got.view(np.int32)[:, y:y + wh, x:x + ww], want[:, y:y + wh, x:x + ww]), win
        assert (before == GUARD).all() and (behind == GUARD).all(), win


@pytest.mark.parametrize("rev", [True, False], ids=["53", "97"])
def test_window_of_a_larger_plane(enc, oracle, rev):
    """More than one workgroup per launch, lines of ten samples and more (reflect_idx's other regime), 5 levels."""
    w, h, x0, y0, levels = 700, 333, 1, 2, 5
    rng = np.random.default_rng(31 + int(rev))
    a = np.stack([rc.plane(rng, w, h, rev), rc.plane(rng, w, h, rev)])
    f = oracle.idwt53 if rev else oracle.idwt97
    want = np.stack([f(p, levels, x0, y0) for p in a]).view(np.int32)
    for win in ((0, 0, w, h), (0, 0, 1, 1), (w - 1, h - 1, 1, 1), (123, 45, 401, 257), (333, 100, 64, 200), (5, 300, 690, 33)):
        mask = rc.footprint_mask(api.region_footprint(w, h, levels, rev, win, x0, y0), w, h)
        bad = np.stack([rc.poison(p, mask, rev, rng, hard=True) for p in a])
        got, before, behind = enc.stage_idwt_window(bad, levels, rev, win, x0, y0, guard=GUARD)
        x, y, ww, wh = win
        assert np.array_equal(got.view(np.int32)[:, y:y + wh, x:x + ww], want[:, y:y + wh, x:x + ww]), win
        assert (before == GUARD).all() and (behind == GUARD).all(), win


def test_window_stage_rejects_bad_windows(enc):
    a = np.zeros((1, 32, 32), dtype=np.int32)
    for bad in ((0, 0, 33, 8), (0, 0, 8, 0), (32, 0, 1, 1), (30, 30, 3, 3)):
        with pytest.raises(api.J2kHipError) as ei:
            enc.stage_idwt_window(a, 2, True, bad)
        assert ei.value.code == 1
