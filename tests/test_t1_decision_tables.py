"""Tier-1 modeller: decision bytes by table.

The modelling kernel takes the decision bytes of a stripe column two bit-planes at a time from a 256-entry table
(entry a | b << 4 = spread4(a) | spread4(b) << 1, a and b the two planes' row nibbles of the stripe) instead of spreading every
nibble with a multiply: the zero-coding bytes of a dense stripe (the planes' index bytes formed once per 32-row half), its sign
bytes, and the refinement pass's bytes (a stripe pair per round: an even and an odd stripe of the half).  No decision byte may
change.

Without the gpu mark: a numpy copy of the three table expressions against the multiply expressions over all inputs, and the
oracle alone on every block below.  With it (run with -m gpu): coded bytes, bit-plane and pass counts -- and with want_passes the
per-pass rates and distortion sums -- against the CPU oracle: reversible and 9/7, with and without the distortion sums, four
orientations, on
  * 48 blocks of 64 x 64 whose bit-planes are random at densities 1/2, 1/8 and 1/32 (3, 5, 7, 9 planes): halves that stay dense;
  * blocks of 32 x 32, 64 x 13, 13 x 64, 5 x 7 and 17 x 64: one half only, an odd last stripe, lanes beyond the width;
  * the pattern and pair-count blocks of t1_fill_refine_families.py: every refinement pattern in both stripes of a pair, in
    both halves;
and on the dense family once more with the knob t1_sparse forced to -1 (never sample-wise) and 1 (always): the same bytes.
"""
import numpy as np
import pytest

import t1_fill_refine_families as fam
from t1_families import layout as _layout

MAX_PASSES = 96  # kDevMaxPasses (kernels.h)


# ---- the table and the three expressions, in numpy
def spread4(x):
    return (np.asarray(x, dtype=np.uint32) * np.uint32(0x00204081)) & np.uint32(0x01010101)


def pair_table():
    t = np.zeros(256, dtype=np.uint32)
    for e in range(256):
        for r in range(4):
            t[e] |= np.uint32((((e >> r) & 1) | (((e >> (4 + r)) & 1) << 1)) << (8 * r))
    return t


def _grid(n):
    return np.meshgrid(*([np.arange(16, dtype=np.uint32)] * n), indexing="ij")


def test_table_is_two_spreads():
    T = pair_table()
    a, b = _grid(2)
    assert (T[a | (b << 4)] == (spread4(a) | (spread4(b) << 1))).all()


def test_zero_coding_bytes_all_inputs():
    T = pair_table()
    bits, zb0, zb1, zb2, zb3 = _grid(5)  # 16^5
    old = (spread4(zb0) << 1) | (spread4(zb1) << 2) | (spread4(zb2) << 3) | (spread4(zb3) << 4) | spread4(bits)
    new = T[bits | (zb0 << 4)] | (T[zb1 | (zb2 << 4)] << 2) | (spread4(zb3) << 4)
    assert (old == new).all()


def test_sign_bytes_all_inputs():
    T = pair_table()
    sd, sb0, sb1, sb2 = _grid(4)  # 16^4
    base = np.uint32(0x12121212)
    old = base + (spread4(sb0) << 1) + (spread4(sb1) << 2) + (spread4(sb2) << 3) + spread4(sd)
    new = base + T[sd | (sb0 << 4)] + (T[sb1 | (sb2 << 4)] << 2)
    assert (old == new).all()


def test_refinement_bytes_all_inputs():
    T = pair_table()
    bits, nb, mu = _grid(3)  # 16^3
    base = np.uint32(0x1c1c1c1c)
    nbm = nb & ~mu & np.uint32(0xf)  # the kernel's neighbour flags are cleared where a sample was refined before
    old = base + (spread4(nbm) << 1) + (spread4(mu) << 2) + spread4(bits)
    new = base + T[bits | (nbm << 4)] + (T[mu] << 2)
    assert (old == new).all()


def test_index_bytes_of_a_half():
    """The index words of a 32-row half for a plane pair (x, y): byte k of `even` is the entry number of stripe 2 k, of `odd`
    that of stripe 2 k + 1; a stripe's byte is picked by parity and sl / 8 (sl = 4 x stripe)."""
    rng = np.random.default_rng(11)
    M = np.uint32(0x0f0f0f0f)
    for _ in range(200):
        x, y = (np.uint32(v) for v in rng.integers(0, 1 << 32, size=2, dtype=np.uint64))
        even = (x & M) | ((y << np.uint32(4)) & ~M)
        odd = ((x >> np.uint32(4)) & M) | (y & ~M)
        for st in range(8):
            word = odd if st & 1 else even
            got = (int(word) >> (8 * (st >> 1))) & 0xff
            assert got == ((int(x) >> (4 * st)) & 0xf) | (((int(y) >> (4 * st)) & 0xf) << 4)


# ---- the blocks
def dense_block(rng, density, planes, w=64, h=64):
    """Every bit-plane random at `density`: about that share of the samples becomes significant per plane."""
    m = np.zeros((h, w), dtype=np.int64)
    for p in range(planes):
        m |= (rng.random((h, w)) < density).astype(np.int64) << p
    return m * np.where(rng.random((h, w)) < 0.5, -1, 1)


def _cases(family):
    rng = np.random.default_rng({"dense": 2024, "shapes": 2025, "refine": 2026}[family])
    cases = []
    if family == "dense":
        for density in (1 / 2, 1 / 8, 1 / 32):
            for planes in (3, 5, 7, 9):
                for o in range(4):
                    cases.append((dense_block(rng, density, planes), o))
    elif family == "shapes":
        for w, h in ((32, 32), (64, 13), (13, 64), (5, 7), (17, 64)):
            for o in range(4):
                cases.append((dense_block(rng, (1 / 2, 1 / 8)[o & 1], 7, w, h), o))
    else:
        for shift in range(8):
            cases.append((fam.pattern_block(shift), shift % 4))
        low = rng.integers(0, 1 << 9, size=(64, 64))
        for shift in range(4):
            cases.append((fam.pattern_block(shift + 1, 9, 64, 64, low) * np.where(rng.random((64, 64)) < 0.5, -1, 1), shift))
        for order in (0, 1):
            for rot in range(4):
                counts = fam.PAIR_COUNTS[rot:] + fam.PAIR_COUNTS[:rot]
                cases.append((fam.pair_count_block(counts, 8, order), (order + rot) % 4))
    return cases


FAMILIES = ["dense", "shapes", "refine"]
_REF = {}


def _reference(oracle, family, rev):
    """The family's plane, rectangles, orientations and the oracle's results, once per (family, rev)."""
    key = (family, rev)
    if key not in _REF:
        coef, rects, orients = _layout(_cases(family))
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


@pytest.mark.parametrize("rev", [True, False], ids=["rev", "irr"])
@pytest.mark.parametrize("family", FAMILIES)
def test_oracle_accepts_every_block(oracle, family, rev):
    _, rects, _, _, refs = _reference(oracle, family, rev)  # (t1_block raises on "t1 overflow")
    assert len(refs) == len(rects) > 0
    assert len(_cases("dense")) == 48
    assert all(0 < ref["npasses"] <= MAX_PASSES for ref in refs)
    assert all(ref["numbps"] > 0 for ref in refs)


def test_refinement_families_reach_both_stripes_of_a_pair_in_both_halves(oracle):
    """The first refinement pass of the pattern blocks codes every 4-row pattern in the even and in the odd stripe of a pair;
    the patterns repeat down the block, so both 32-row halves hold them."""
    seen = set()
    for shift in range(8):
        block = fam.pattern_block(shift)
        assert (block[:32] != 0).any() and (block[32:] != 0).any()
        ref = oracle.t1_block((block.astype(np.int64) << 6).astype(np.int32), shift % 4, want_symbols=True)
        seen |= {(k, p) for k, p, _ in fam.pattern_coverage(shift, ref["pass_nsym"][1])}
    assert seen == {(k, p) for k in range(2) for p in range(16)}


# ---- the kernel (GPU)
@pytest.fixture(scope="module")
def enc():
    from j2k_amd import api
    e = api.Encoder(0)
    before = api.get_tune("t1_sparse")
    yield e
    api.tune("t1_sparse", before)
    e.close()


def _compare(got, rects, orients, refs, passes):
    assert len(got) == len(refs)
    for r, o, g, ref in zip(rects, orients, got, refs):
        assert g["numbps"] == ref["numbps"], (r, o)
        assert g["npasses"] == ref["npasses"], (r, o)
        assert g["data"] == ref["data"], (r, o)
        assert g["length"] == len(ref["data"]), (r, o)
        if passes:
            assert g["rates"] == ref["rates"], (r, o)
            assert g["nmsedec"] == ref["nmsedec"], (r, o)


@pytest.mark.gpu
@pytest.mark.parametrize("passes", [False, True], ids=["plain", "dist"])
@pytest.mark.parametrize("rev", [True, False], ids=["rev", "irr"])
@pytest.mark.parametrize("family", FAMILIES)
def test_t1_decision_tables_match_oracle(enc, oracle, family, rev, passes):
    plane, rects, orients, step, refs = _reference(oracle, family, rev)
    got = enc.stage_t1(plane.copy(), rects, orients, [step] * len(rects), rev, want_passes=passes)
    _compare(got, rects, orients, refs, passes)


@pytest.mark.gpu
@pytest.mark.parametrize("sparse", [-1, 1], ids=["never", "always"])
@pytest.mark.parametrize("passes", [False, True], ids=["plain", "dist"])
@pytest.mark.parametrize("rev", [True, False], ids=["rev", "irr"])
def test_t1_decision_tables_under_either_path_choice(enc, oracle, rev, passes, sparse):
    from j2k_amd import api
    plane, rects, orients, step, refs = _reference(oracle, "dense", rev)
    before = api.get_tune("t1_sparse")
    api.tune("t1_sparse", sparse)
    try:
        got = enc.stage_t1(plane.copy(), rects, orients, [step] * len(rects), rev, want_passes=passes)
    finally:
        api.tune("t1_sparse", before)
    _compare(got, rects, orients, refs, passes)
