"""Tier-1 modeller: run-length fills of the cleanup pass and the register-packed refinement pass.

The modelling kernel writes a cleanup stripe in which every column of the block is in run-length mode and holds no 1 as
w identical bytes (and skips the context planes of a 32-row half that consists of such stripes), and it compacts the
refinement pass's decision bytes of a stripe column with one byte permute and ORs them into its LDS stage as words.
Neither may change a byte.  Coded bytes, bit-plane and pass counts, and with want_passes the per-pass rates and distortion
sums are compared with the CPU oracle -- reversible and 9/7, with and without the distortion sums, four orientations --
on the blocks of t1_fill_refine_families.py (run with -m gpu).

The tests without the gpu mark run the oracle alone: it accepts every input (no overflow, no more passes than the device
tables hold), and its decision streams show that the blocks reach what they were built for -- fills that cross the 1 KiB
flush of the stage at every offset mod 4, every 4-row refinement pattern in either stripe of a pair at every byte
alignment, stripe pairs with 0, 1, 63, 64, 447, 448, 511 and 512 refined samples.
"""
import numpy as np
import pytest

import t1_fill_refine_families as fam
from t1_families import layout as _layout

MAX_PASSES = 96  # kDevMaxPasses (kernels.h)
RL_ZERO = 17 << 1  # the run-length context's decision "no 1 in this stripe column"


@pytest.fixture(scope="module")
def enc():
    from j2k_amd import api
    e = api.Encoder(0)
    yield e
    e.close()


def _cases(family):
    rng = np.random.default_rng({"fill": 777, "refine": 888}[family])
    if family == "fill":
        return fam.fill_families(rng) + fam.flush_crossing_blocks()
    return fam.refine_families(rng)


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


@pytest.mark.gpu
@pytest.mark.parametrize("passes", [False, True], ids=["plain", "dist"])
@pytest.mark.parametrize("rev", [True, False], ids=["rev", "irr"])
@pytest.mark.parametrize("family", ["fill", "refine"])
def test_t1_fill_refine_matches_oracle(enc, oracle, family, rev, passes):
    plane, rects, orients, step, refs = _reference(oracle, family, rev)
    got = enc.stage_t1(plane.copy(), rects, orients, [step] * len(rects), rev, want_passes=passes)
    assert len(got) == len(refs)
    for r, o, g, ref in zip(rects, orients, got, refs):
        assert g["numbps"] == ref["numbps"], (r, o)
        assert g["npasses"] == ref["npasses"], (r, o)
        assert g["data"] == ref["data"], (r, o)
        if passes:
            assert g["rates"] == ref["rates"], (r, o)
            assert g["nmsedec"] == ref["nmsedec"], (r, o)
        else:
            assert g["length"] == len(ref["data"]), (r, o)


# ---- the oracle alone (no GPU)
@pytest.mark.parametrize("rev", [True, False], ids=["rev", "irr"])
@pytest.mark.parametrize("family", ["fill", "refine"])
def test_oracle_accepts_every_block(oracle, family, rev):
    _, rects, _, _, refs = _reference(oracle, family, rev)  # (t1_block raises on "t1 overflow")
    assert len(refs) == len(rects) > 0
    assert all(0 < ref["npasses"] <= MAX_PASSES for ref in refs)
    assert all(ref["numbps"] > 0 for ref in refs)


def _symbols(oracle, block, orient):
    return oracle.t1_block((block.astype(np.int64) << 6).astype(np.int32), orient, want_symbols=True)


def test_fills_cross_the_flush_at_every_offset(oracle):
    offsets, crossings = set(), 0
    for block, orient in fam.flush_crossing_blocks():
        ref = _symbols(oracle, block, orient)
        for pos, n in fam.fill_positions(block, ref["pass_nsym"]):
            assert (ref["symbols"][pos:pos + n] == RL_ZERO).all(), (block.shape, pos)  # the fills are where the builder says
            if fam.crosses_flush(pos, n):
                offsets.add(pos % 4)
                crossings += 1
    assert offsets == {0, 1, 2, 3}, offsets
    assert crossings >= 32


def test_fill_blocks_hold_whole_fill_halves_and_mixed_ones(oracle):
    """In a 64-wide block a run of 64 k decisions "run-length, no 1" covers at least k - 1 whole stripes: runs of 9 x 64 cover a
    whole half, shorter ones of 2 x 64 and more lie between stripes that code something."""
    rng = np.random.default_rng(777)
    whole, between = 0, 0
    for block, orient in fam.fill_families(rng):
        if block.shape != (64, 64):
            continue
        sym = _symbols(oracle, block, orient)["symbols"]
        edges = np.flatnonzero(np.diff(np.concatenate(([0], (sym == RL_ZERO).astype(np.int8), [0]))))
        runs = edges[1::2] - edges[0::2]
        whole += int((runs >= 9 * 64).sum())
        between += int(((runs >= 2 * 64) & (runs < 9 * 64)).sum())
    assert whole >= 50 and between >= 50, (whole, between)


def test_refinement_patterns_at_every_alignment(oracle):
    seen = set()
    for shift in range(8):
        block = fam.pattern_block(shift)
        ref = _symbols(oracle, block, shift % 4)
        # passes: cleanup of the top plane, then significance propagation and refinement of the next one
        start, end = ref["pass_nsym"][1], ref["pass_nsym"][2]
        assert end - start == int((block != 0).sum())  # the refinement pass codes exactly the pattern
        seen |= fam.pattern_coverage(shift, start)
    assert seen == {(k, p, al) for k in range(2) for p in range(16) for al in range(4)}


def test_refinement_pairs_by_refined_samples(oracle):
    block = fam.pair_count_block()
    ref = _symbols(oracle, block, 0)
    assert ref["pass_nsym"][2] - ref["pass_nsym"][1] == sum(fam.PAIR_COUNTS)
    per_pair = [int((block[8 * j:8 * j + 8] != 0).sum()) for j in range(8)]
    assert per_pair == list(fam.PAIR_COUNTS)
