"""Tier-1 modeller, sample-wise writing of sparse significance / cleanup passes (run with -m gpu).

The modelling kernel writes a 32-row half of a significance-propagation pass (or of a cleanup pass without run-length
columns) either stripe by stripe or -- when few samples are visited -- sample by sample; the knob t1_sparse picks the
path (0: by the counts, -1: never sample-wise, 1: sample-wise whenever the half fits the LDS stage).  No byte may
depend on it.  Coded bytes, bit-plane and pass counts, and with want_passes the per-pass rates and distortion sums are
compared with the CPU oracle under all three settings, reversible and 9/7, with and without the distortion sums, all
four orientations:
  (a) the block families of test_t1_emission.py: every width 1..64, odd heights, 32-row blocks, lanes at the 10-byte
      maximum of a stripe column, long streams;
  (b) blocks for the sparse regime: 64 x 64 Gaussian / Laplacian magnitudes at scales 2^4 .. 2^12 (low planes with a
      few to a thousand insignificant samples), isolated significant samples and single significant rows / columns at
      block edges and stripe boundaries (rows 3|4, 31|32, 63; columns 0 and 63: "left column new, right column old, row
      below old across the stripe boundary"), and a sweep of the fraction of non-zero samples (0.1 % .. 30 %) that puts
      halves on both sides of the path choice and of the 640-byte limit of the stage.
"""
import numpy as np
import pytest

from t1_families import emission_families as _emission_families, layout as _layout, sparse_families as _sparse_families

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def enc():
    from j2k_amd import api
    e = api.Encoder(0)
    before = api.get_tune("t1_sparse")
    yield e
    api.tune("t1_sparse", before)
    e.close()


_REF = {}


def _reference(oracle, family, rev):
    """The family's plane, rectangles, orientations and the oracle's results (with passes), once per (family, rev)."""
    key = (family, rev)
    if key not in _REF:
        rng = np.random.default_rng(4321 + 7 * int(rev) + (0 if family == "emission" else 100))
        cases = _emission_families(rng) if family == "emission" else _sparse_families(rng)
        coef, rects, orients = _layout(cases)
        step = 1.0 if rev else 0.37
        plane = coef.astype(np.int32) if rev else (coef * 0.61).astype(np.float32)
        refs = []
        for (x, y, w, h), o in zip(rects, orients):
            blk = plane[y:y + h, x:x + w]
            if rev:
                data = (blk.astype(np.int64) << 6).astype(np.int32)
            else:
                data = np.array([[oracle.L.j2ko_quant97(float(v), step) for v in row] for row in blk], dtype=np.int32)
            refs.append(oracle.t1_block(data, o))
        _REF[key] = (plane, rects, orients, step, refs)
    return _REF[key]


@pytest.mark.parametrize("sparse", [-1, 0, 1], ids=["never", "auto", "always"])
@pytest.mark.parametrize("passes", [False, True], ids=["plain", "dist"])
@pytest.mark.parametrize("rev", [True, False], ids=["rev", "irr"])
@pytest.mark.parametrize("family", ["emission", "sparse"])
def test_t1_sparse_pass_matches_oracle(enc, oracle, family, rev, passes, sparse):
    from j2k_amd import api
    plane, rects, orients, step, refs = _reference(oracle, family, rev)
    api.tune("t1_sparse", sparse)
    try:
        got = enc.stage_t1(plane.copy(), rects, orients, [step] * len(rects), rev, want_passes=passes)
    finally:
        api.tune("t1_sparse", 0)
    for r, o, g, ref in zip(rects, orients, got, refs):
        assert g["numbps"] == ref["numbps"], (r, o)
        assert g["npasses"] == ref["npasses"], (r, o)
        assert g["data"] == ref["data"], (r, o)
        if passes:
            assert g["rates"] == ref["rates"], (r, o)
            assert g["nmsedec"] == ref["nmsedec"], (r, o)
        else:
            assert g["length"] == len(ref["data"]), (r, o)
