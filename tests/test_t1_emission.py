"""Tier-1 decision emission on the GPU (run with -m gpu): blocks built to hit the edges of how the modelling kernel
packs a stripe column's decision bytes in registers and ORs them into its LDS stage as words -- lanes at the 10-byte
maximum (run-length prefix with the first 1 in each row of the stripe, then zero coding + sign on every row below),
every block width 1..64, heights that are not multiples of 4 and 32-row blocks, all four orientations, streams long
enough to cross the 1 KiB flush of the stage many times at varying offsets, reversible and 9/7, with and without
the distortion sums of rate control.  Coded bytes, bit-plane and pass counts, per-pass rates and distortion sums
are compared with the CPU oracle."""
import numpy as np
import pytest

from t1_families import max_stripes as _max_stripes, random_block as _random_block

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def enc():
    from j2k_amd import api
    e = api.Encoder(0)
    yield e
    e.close()


def _cases(seed):
    rng = np.random.default_rng(seed)
    blocks = []
    heights = [1, 2, 3, 5, 6, 7, 13, 31, 32, 33, 37, 61, 62, 63, 64]
    for w in range(1, 65):  # every width, heights cycling through the awkward ones
        blocks.append(_random_block(rng, w, heights[w % len(heights)], w % 4))
    for h in (64, 32, 63, 30):
        for w in (64, 63, 33, 17):
            blocks.append(_max_stripes(rng, w, h, 10 + (w % 3)))
    for i in range(16):  # full blocks with long streams: many flushes of the stage at varying offsets
        blocks.append(_random_block(rng, 64, 64 if i % 4 else 32, i % 4))
    # one 64 x 64 cell per block in a plane of 16 cells per row (the kernel rewrites each block in place)
    ncol = 16
    nrow = (len(blocks) + ncol - 1) // ncol
    coef = np.zeros((64 * nrow, 64 * ncol), dtype=np.int64)
    rects, orients = [], []
    for i, b in enumerate(blocks):
        h, w = b.shape
        x, y = 64 * (i % ncol), 64 * (i // ncol)
        coef[y:y + h, x:x + w] = b
        rects.append((x, y, w, h))
        orients.append(i % 4)
    return coef, rects, orients


@pytest.mark.parametrize("rev", [True, False], ids=["rev", "irr"])
@pytest.mark.parametrize("passes", [False, True], ids=["plain", "dist"])
def test_t1_emission_edges_match_oracle(enc, oracle, rev, passes):
    coef, rects, orients = _cases(1234 + 2 * int(rev) + int(passes))
    step = 1.0 if rev else 0.37
    plane = coef.astype(np.int32) if rev else (coef * 0.61).astype(np.float32)
    got = enc.stage_t1(plane, rects, orients, [step] * len(rects), rev, want_passes=passes)
    for r, o, g in zip(rects, orients, got):
        x, y, w, h = r
        blk = plane[y:y + h, x:x + w]
        if rev:
            data = (blk.astype(np.int64) << 6).astype(np.int32)
        else:
            data = np.array([[oracle.L.j2ko_quant97(float(v), step) for v in row] for row in blk], dtype=np.int32)
        ref = oracle.t1_block(data, o)
        assert g["numbps"] == ref["numbps"], (r, o)
        assert g["npasses"] == ref["npasses"], (r, o)
        assert g["data"] == ref["data"], (r, o)
        if passes:
            assert g["rates"] == ref["rates"], (r, o)
            assert g["nmsedec"] == ref["nmsedec"], (r, o)
        else:
            assert g["length"] == len(ref["data"]), (r, o)
