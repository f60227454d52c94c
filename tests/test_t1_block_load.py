"""Tier-1 modeller: the block load -- scaling to sign-magnitude and the bit-plane transposition in one sweep.

A block of 64 or 32 rows is read 32 rows at a time into registers, scaled there (9/7: divided by the step size and rounded
to 1/64 steps; 5/3: shifted), transposed to one word per bit-plane, and the plane words are written over the block's own
rows; the magnitudes are never stored.  Blocks of any other height scale their samples in place and read every bit-plane
from there.  Neither may change a byte: bit-plane and pass counts, coded bytes, and with want_passes the per-pass rates and
distortion sums of every block of t1_block_load_families.py are compared with the CPU oracle -- reversible and 9/7, with
and without the distortion sums (run with -m gpu).

The kernel's branch for "more bit-planes than the pass tables hold" is not among the cases: a 32-bit word with 6 fractional
bits holds at most 26 bit-planes = 76 passes, and the tables hold 96 (test_pass_tables_hold_every_word states the
arithmetic); the blocks of the most planes a word holds without its top bit (25) are there instead.

The tests without the gpu mark run the oracle alone: it accepts every block, and the families reach what they claim --
every block shape of either path, neighbours on all sides at a stride that is no multiple of 64, every number of
bit-planes with all (row, plane) pairs distinguishable, the quantiser's ties, its dead-zone edge and its largest values.
"""
import numpy as np
import pytest

import t1_block_load_families as fam

MAX_PASSES = 96  # kDevMaxPasses (kernels.h)
GROUPS = ["shapes", "neighbours", "walking", "values"]
_REF = {}


@pytest.fixture(scope="module")
def enc():
    from j2k_amd import api
    e = api.Encoder(0)
    yield e
    e.close()


def _irr_plane(name, g):
    """The 9/7 plane of a group and its step sizes (the integer families scaled by a constant; the walking blocks as they
    are, cut to the 24 bits a float holds, at step size 1 so that every fractional bit below is zero)."""
    nb = len(g["rects"])
    if g["steps"] is not None:
        return g["plane"], g["steps"]
    if name == "walking":
        c = g["plane"]
        c = np.where(np.abs(c) >= 1 << 24, np.sign(c) * (np.abs(c) & ~1), c)
        plane = c.astype(np.float32)
        assert (plane.astype(np.int64) == c).all()
        return plane, [1.0] * nb
    return (g["plane"] * 0.61).astype(np.float32), [float(np.float32(0.37))] * nb


def _reference(oracle, name, rev):
    """The group's plane, rectangles, orientations, step sizes, the scaled blocks and the oracle's results, once."""
    key = (name, rev)
    if key not in _REF:
        g = fam.group(name)
        nb = len(g["rects"])
        if rev:
            plane, steps = g["plane"].astype(np.int32), [1.0] * nb
        else:
            plane, steps = _irr_plane(name, g)
        datas, refs = [], []
        for (x, y, w, h), o, step in zip(g["rects"], g["orients"], steps):
            blk = plane[y:y + h, x:x + w]
            if rev:
                data = (blk.astype(np.int64) << 6).astype(np.int32)
            else:
                data = np.array([[oracle.L.j2ko_quant97(float(v), step) for v in row] for row in blk], dtype=np.int32)
            datas.append(data)
            refs.append(oracle.t1_block(data, o))
        plane.setflags(write=False)
        _REF[key] = (plane, g["rects"], g["orients"], steps, datas, refs)
    return _REF[key]


def _cases():
    return [(n, r) for n in GROUPS for r in (True, False) if not (n == "values" and r)]


@pytest.mark.gpu
@pytest.mark.parametrize("passes", [False, True], ids=["plain", "dist"])
@pytest.mark.parametrize("name,rev", _cases(), ids=[f"{n}-{'rev' if r else 'irr'}" for n, r in _cases()])
def test_t1_block_load_matches_oracle(enc, oracle, name, rev, passes):
    plane, rects, orients, steps, _, refs = _reference(oracle, name, rev)
    got = enc.stage_t1(plane.copy(), rects, orients, steps, rev, want_passes=passes)
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
@pytest.mark.parametrize("name,rev", _cases(), ids=[f"{n}-{'rev' if r else 'irr'}" for n, r in _cases()])
def test_oracle_accepts_every_block(oracle, name, rev):
    _, rects, _, _, datas, refs = _reference(oracle, name, rev)  # (t1_block raises on "t1 overflow")
    assert len(refs) == len(rects) > 0
    for data, ref in zip(datas, refs):
        assert ref["npasses"] <= MAX_PASSES
        top = int(np.abs(data.astype(np.int64)).max())
        assert top < 1 << 31
        assert ref["numbps"] == max(0, top.bit_length() - fam.FRAC)
        assert ref["npasses"] == (3 * ref["numbps"] - 2 if ref["numbps"] else 0)


def test_pass_tables_hold_every_word():
    # a magnitude word of 32 bits with 6 fractional ones: at most 26 bit-planes, 3 * 26 - 2 passes
    assert 3 * (32 - fam.FRAC) - 2 <= MAX_PASSES
    assert 3 * fam.MAX_PLANES - 2 <= MAX_PASSES


def test_shapes_cover_both_paths():
    g = fam.group("shapes")
    shapes = {(w, h) for _, _, w, h in g["rects"]}
    assert set(fam.PLANE_SHAPES) <= shapes
    assert {h for _, h in shapes if h not in (32, 64)} == set(fam.INPLACE_HEIGHTS)
    for w, h in shapes:  # every shape under all four orientations' worth of content
        assert sum(1 for r in g["rects"] if r[2:] == (w, h)) == 4


def test_neighbours_tile_the_plane():
    g = fam.group("neighbours")
    H, W = g["plane"].shape
    assert W % 64 != 0 and W == sum(fam.NEIGHBOUR_WIDTHS)
    cover = np.zeros((H, W), dtype=np.int32)
    for x, y, w, h in g["rects"]:
        cover[y:y + h, x:x + w] += 1
    assert (cover == 1).all()  # no gap: whatever a block writes outside itself lands in another block
    heights = {h for _, _, _, h in g["rects"]}
    assert {64, 32} <= heights and heights - {64, 32}
    # a block of plane words (h 64 / 32) narrower than the wave has a neighbour to its right, and one below it
    assert any(h in (64, 32) and w < 64 and x + w < W and y + h < H for x, y, w, h in g["rects"])


@pytest.mark.parametrize("rev", [True, False], ids=["rev", "irr"])
def test_walking_blocks_reach_every_plane_count(oracle, rev):
    _, rects, _, _, datas, refs = _reference(oracle, "walking", rev)
    assert [ref["numbps"] for ref in refs[:fam.MAX_PLANES]] == list(range(1, fam.MAX_PLANES + 1))
    assert refs[fam.MAX_PLANES]["numbps"] == 0 and refs[fam.MAX_PLANES]["npasses"] == 0  # the all-zero block
    assert refs[fam.MAX_PLANES + 1]["numbps"] == fam.MAX_PLANES and refs[fam.MAX_PLANES + 2]["numbps"] == fam.MAX_PLANES
    for n, data in enumerate(datas[:fam.MAX_PLANES], start=1):
        vec, signs = fam.row_plane_vectors(data.astype(np.int64))
        coded = {k: v for k, v in vec.items() if k[1] >= fam.FRAC and k[1] >= fam.FRAC + n - 24}  # (a float holds 24 of them)
        assert len({r for r, _ in coded}) == 64 and len({p for _, p in coded}) == min(n, 24)
        assert len(set(coded.values())) == len(coded), n  # every (row, plane) pair differs from every other
        assert len(set(signs)) == 64 and all(0 < s < (1 << 64) - 1 for s in signs), n  # mixed signs, no two rows alike


def test_values_hold_the_quantiser_edges(oracle):
    plane, rects, _, steps, datas, _ = _reference(oracle, "values", False)
    assert {np.float32(s) for s in steps} == {np.float32(s) for s in fam.STEPS}
    q = oracle.L.j2ko_quant97
    for step in {float(np.float32(s)) for s in steps}:
        m = np.frexp(np.float64(step))[0] * 4096
        assert m == int(m)  # 11 mantissa bits below the leading one: a step size the codestream can signal
        t = fam.ties(step, 64)
        x = t.astype(np.float64) / np.float64(step) * 64  # exact: (2 k + 1) / 2
        assert (np.abs(x) % 1 == 0.5).all()
        got = np.array([q(float(v), step) for v in t])
        assert (got % 2 == 0).all() and (np.abs(got - x) == 0.5).all()  # ties go to the even neighbour
        assert len(set(np.abs(got) // 2 % 2)) == 2  # from odd and from even quotients
        dz = [q(float(v), step) for v in fam.dead_zone(step)]
        assert dz == [0, 0, 1, 0, 0, -1]
        assert [q(float(v), step) for v in fam.tiny()] == [0] * 6 or step < 2.0 ** -100
        big = [abs(q(float(v), step)) for v in fam.largest(step)]
        assert all((1 << 30) <= b < (1 << 31) for b in big)
    # and the blocks carry them: per step size one block with 25 bit-planes and one without, in three shapes
    tops = {}
    for (x, y, w, h), step, data in zip(rects, steps, datas):
        tops.setdefault((step, w, h), set()).add(int(np.abs(data.astype(np.int64)).max()).bit_length() - fam.FRAC)
        blk = plane[y:y + h, x:x + w]
        assert (blk[0] == fam.ties(step, 64)[:w]).all() or w == 17
        assert np.signbit(blk[blk == 0]).any()  # a -0.0
    assert all(len(v) == 2 and max(v) == fam.MAX_PLANES for v in tops.values())
    assert {(w, h) for _, w, h in tops} == {(64, 64), (32, 32), (17, 64)}
