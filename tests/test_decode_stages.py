"""Decode kernels in isolation (run with -m gpu): the Tier-1 decoders -- a wavefront per block (t1_decode_kernel +
t1_assemble_kernel) and a lane per block (t1_decode_lanes_kernel + t1_assemble_lanes_kernel) -- through
j2k_hip_stage_t1_decode, and the inverse DWT (idwt_h_kernel + idwt_v_kernel) through j2k_hip_stage_idwt, against the
oracle's block decoder and inverse transforms.  Every comparison is word for word: no tolerance anywhere in this file.

Tier-1: the expected plane is the oracle's block decoder used as its tile decoder uses it (reversible v / 2 toward zero,
irreversible float32(v) x float32(0.5 step)); words outside every block's rectangle must keep what they held.  Both
kernels, both transforms:
  * the block families of the encode-side tests (t1_families.py), all four orientations, every pass;
  * every possible last pass, and codewords cut short (half, one byte, none) with the passes kept: past the end a decoder is
    fed 1-bits (T.800 C.3.4), while the bytes behind a block in the arena are zeros here;
  * blocks of one pass; blocks that hold nothing (no pass, no bit-plane: left alone) and a block that claims more passes
    than 3 numbps - 2 (decoded like the clamped count): the rules of a file decode (decode_plan.h: t1dec_passes);
  * a 9 KB stream, whole and cut at 256, 512 and 4096 bytes (the refill granules of the wave kernel's byte window);
  * 25 bit-planes (73 passes); region-of-interest shifts; and for the lane kernel a wave of 64 unlike blocks.
Inverse DWT: lengths 1 .. 13 (where reflect_idx changes regime and the vertical kernel's groups of four row pairs are
partial) by both parities on either axis, many regions of different sizes in one launch, the shapes of the forward
transform's test, exact zeros and denormal intermediates.
"""
import numpy as np
import pytest

import decode_stage_cases as dc
from t1_families import emission_families, random_block, sparse_families

pytestmark = pytest.mark.gpu

KERNELS = ["wave", "lanes"]
TRANSFORMS = [True, False]
both = lambda f: pytest.mark.parametrize("kernel", KERNELS)(pytest.mark.parametrize("rev", TRANSFORMS, ids=["rev", "irr"])(f))


@pytest.fixture(scope="module")
def enc():
    from j2k_amd import api
    e = api.Encoder(0)
    yield e
    e.close()


_CASES = {}


def _cached(key, make):
    if key not in _CASES:
        _CASES[key] = make()
    return _CASES[key]


def _check(enc, oracle, cases, rev, kernel):
    got, want, rects = dc.decode_and_expect(enc, oracle, cases, rev, kernel)
    dc.assert_planes_equal(got, want, rects, cases)


def _family_cases(oracle, family, rev):
    def make():
        rng = np.random.default_rng(8642 + 7 * int(rev) + (0 if family == "emission" else 100))
        fam = emission_families(rng) if family == "emission" else sparse_families(rng)
        if family == "emission":  # (the family fixes one orientation per block: here each block under all four)
            fam = [(b, o) for b, _ in fam for o in range(4)]
        return [dc.code_block(oracle, b, o, rev) for b, o in fam]
    return _cached(("family", family, rev), make)


def _subset(oracle, rev):
    return _cached(("subset", rev), lambda: [dc.code_block(oracle, b, o, rev) for _, b, o in dc.subset_blocks(np.random.default_rng(1357 + int(rev)))])


# ------------------------------------------------------------------------------------------------ Tier-1
@both
@pytest.mark.parametrize("family", ["emission", "sparse"])
def test_t1_decode_families(enc, oracle, family, rev, kernel):
    cases = _family_cases(oracle, family, rev)
    assert all(c["npasses"] == dc.kernel_passes(c["numbps"], c["npasses"]) for c in cases)
    _check(enc, oracle, cases, rev, kernel)


@both
def test_t1_decode_every_last_pass(enc, oracle, rev, kernel):
    """Blocks cut after each of their passes, with the bytes a rate allocation would keep (the coder's rate of that pass)."""
    cases = []
    for c in _subset(oracle, rev):
        assert c["npasses"] >= 4
        cases += [dc.variant(c, npasses=p, data=c["data"][:c["rates"][p - 1]]) for p in range(1, c["npasses"])]
        cases += [dc.variant(c, npasses=p) for p in range(1, c["npasses"], 5)]  # ... and with all bytes behind the cut
    _check(enc, oracle, cases, rev, kernel)


@both
def test_t1_decode_short_codewords(enc, oracle, rev, kernel):
    """Passes kept, bytes gone: the decoder runs on into 1-bits."""
    cases = []
    for c in _subset(oracle, rev):
        n = len(c["data"])
        assert n >= 2
        cases += [dc.variant(c, data=c["data"][:k]) for k in (n // 2, 1, 0)]
    _check(enc, oracle, cases, rev, kernel)


@both
def test_t1_decode_single_pass(enc, oracle, rev, kernel):
    """npasses == 1: the cleanup pass of the top bit-plane alone."""
    rng = np.random.default_rng(2468)
    shapes = [(64, 64, 0), (64, 64, 1), (1, 1, 0), (1, 64, 0), (64, 1, 3), (3, 5, 2), (37, 13, 0), (64, 4, 2), (5, 63, 3), (63, 33, 1)]
    cases = []
    for i, (w, h, kind) in enumerate(shapes):
        c = dc.code_block(oracle, random_block(rng, w, h, kind), i % 4, rev)
        cases.append(dc.variant(c, npasses=1, data=c["data"][:c["rates"][0]]))
        cases.append(dc.variant(c, npasses=1))
    _check(enc, oracle, cases, rev, kernel)


@both
def test_t1_decode_blocks_that_hold_nothing_and_pass_clamp(enc, oracle, rev, kernel):
    rng = np.random.default_rng(1122)
    full = [dc.code_block(oracle, random_block(rng, w, h, 0), o, rev) for (w, h, o) in ((64, 64, 0), (17, 9, 1), (5, 64, 3))]
    cases = []
    for c in full:
        cases.append(dc.variant(c, npasses=0))                 # bit-planes, no pass: left alone
        cases.append(dc.variant(c, numbps=0, npasses=1))       # no bit-plane: left alone
        cases.append(dc.variant(c, numbps=0, npasses=0, data=b""))
        over = dc.variant(c, npasses=c["npasses"] + 5)         # more passes than the bit-planes allow: the clamped count
        assert c["npasses"] == 3 * c["numbps"] - 2
        assert np.array_equal(dc.expected_words(oracle, over, rev), dc.expected_words(oracle, c, rev))
        cases.append(over)
        cases.append(c)
    assert sum(dc.expected_words(oracle, c, rev) is None for c in cases) == 9
    _check(enc, oracle, cases, rev, kernel)


@both
def test_t1_decode_long_stream(enc, oracle, rev, kernel):
    c = dc.code_scaled(oracle, dc.long_stream_block(np.random.default_rng(4242)), 0)
    assert c["numbps"] == 16 and c["npasses"] == 46 and len(c["data"]) > 8192
    cases = [c] + [dc.variant(c, data=c["data"][:k], orient=o) for k, o in ((256, 0), (512, 1), (4096, 3), (255, 0), (257, 2))]
    cases += [dc.variant(dc.code_scaled(oracle, dc.long_stream_block(np.random.default_rng(4243)), 1), orient=1)]
    _check(enc, oracle, cases, rev, kernel)


@both
def test_t1_decode_top_bit_planes(enc, oracle, rev, kernel):
    rng = np.random.default_rng(4242)
    cases = []
    for o in range(4):
        c = dc.code_scaled(oracle, dc.top_planes_block(rng), o)
        assert c["numbps"] == 25 and c["npasses"] == 73
        cases += [c, dc.variant(c, npasses=72), dc.variant(c, npasses=71)]
    _check(enc, oracle, cases, rev, kernel)


@both
@pytest.mark.parametrize("shift", [0, 3, 7])
def test_t1_decode_roi_shift(enc, oracle, rev, kernel, shift):
    rng = np.random.default_rng(3300 + shift)
    cases = [dc.code_block(oracle, random_block(rng, w, h, kind), o, rev, roishift=shift)
             for (w, h, kind, o) in ((64, 64, 0, 0), (64, 64, 3, 1), (33, 7, 0, 2), (1, 64, 1, 3))]
    cases.append(dc.variant(cases[0], npasses=cases[0]["npasses"] - 3))
    if shift:  # the shift moves some samples and leaves others
        v = oracle.t1_decode_block(cases[0]["data"], 64, 64, 0, cases[0]["numbps"], cases[0]["npasses"])
        assert (np.abs(v) >= (1 << shift)).any() and ((np.abs(v) < (1 << shift)) & (v != 0)).any()
    _check(enc, oracle, cases, rev, kernel)


def _unlike_group(oracle, rev):
    """87 blocks, a full wave of 64 and a partial one: every width 1 .. 64 and heights 1 .. 64 mixed, pass counts from 1 to
    each block's maximum side by side, one stream empty, one block cut to a byte."""
    def make():
        rng = np.random.default_rng(6060 + int(rev))
        cases = []
        for i in range(87):
            w, h = 1 + (i * 37) % 64, 1 + (i * 23 + 5) % 64
            c = dc.code_block(oracle, random_block(rng, w, h, i % 4), i % 4, rev)
            full = c["npasses"]
            if full == 0:  # (a small block of zeros: nothing coded, it stays in the list and out of the wave)
                cases.append(c)
                continue
            np_ = full if i % 5 == 0 else (1 if i % 16 == 1 else 1 + (i * 7) % full)
            cases.append(dc.variant(c, npasses=np_, data=c["data"] if i % 3 else c["data"][:c["rates"][np_ - 1]]))
        cases[11] = dc.variant(cases[11], data=b"")
        cases[70] = dc.variant(cases[70], data=cases[70]["data"][:1])
        return cases
    return _cached(("unlike", rev), make)


@pytest.mark.parametrize("rev", TRANSFORMS, ids=["rev", "irr"])
def test_t1_decode_lanes_unlike_blocks_in_one_wave(enc, oracle, rev):
    cases = _unlike_group(oracle, rev)
    assert {c["w"] for c in cases[:64]} == set(range(1, 65)) and len({c["h"] for c in cases}) == 64
    assert 1 in {c["npasses"] for c in cases[:64]} and max(c["npasses"] for c in cases[:64]) >= 25
    _check(enc, oracle, cases, rev, "lanes")
    _check(enc, oracle, cases[::-1], rev, "lanes")  # other neighbours, other group maxima, the same blocks
    _check(enc, oracle, cases, rev, "wave")


def test_t1_decode_stage_rejects_bad_rectangles(enc):
    from j2k_amd import api
    blk = dict(rect=(0, 0, 8, 8), orient=0, numbps=3, npasses=1, data=b"\x12\x34")
    plane = np.zeros((64, 128), dtype=np.int32)
    for bad in ([dict(blk, rect=(0, 0, 65, 8))], [dict(blk, rect=(0, 0, 8, 0))], [dict(blk, rect=(124, 0, 8, 8))],
                [blk, dict(blk, rect=(7, 7, 8, 8))]):
        with pytest.raises(api.J2kHipError):
            enc.stage_t1_decode(plane, bad, True, "wave")


# ------------------------------------------------------------------------------------------------ inverse DWT
def _idwt_ref(oracle, a, levels, rev, x0, y0):
    f = oracle.idwt53 if rev else oracle.idwt97
    return np.stack([f(p, levels, x0, y0) for p in a])


@pytest.mark.parametrize("levels", dc.SWEEP_LEVELS)
@pytest.mark.parametrize("rev", TRANSFORMS, ids=["53", "97"])
def test_idwt_sweep(enc, oracle, rev, levels):
    """Every (w, h, origin) of the sweep as a region of one plane: 1350 jobs of different sizes and parities per launch.
    Two planes; the second 9/7 plane holds exact zeros and values near 2^-120 (denormal lifting products)."""
    rng = np.random.default_rng(7000 + levels + 10 * int(rev))
    height, regions = dc.pack_regions(dc.sweep_shapes())
    a = np.stack([dc.idwt_input(rng, (height, 1024), rev), dc.idwt_input(rng, (height, 1024), rev, tiny=True)])
    got = enc.stage_idwt(a, levels, rev, regions=regions)
    for p in range(2):
        want = dc.idwt_regions_reference(oracle, a[p], regions, levels, rev)
        g = got[p].view(np.int32)
        if np.array_equal(g, want.view(np.int32)):
            continue
        for (x, y, w, h, x0, y0) in regions:
            assert np.array_equal(g[y:y + h, x:x + w], want[y:y + h, x:x + w].view(np.int32)), \
                f"plane {p}: region {w} x {h} at origin ({x0}, {y0}), {levels} levels"
        raise AssertionError(f"plane {p}: words between the regions were written")


@pytest.mark.parametrize("case", dc.IDWT_SHAPES, ids=str)
@pytest.mark.parametrize("rev", TRANSFORMS, ids=["53", "97"])
def test_idwt_matches_oracle_bit_exact(enc, oracle, case, rev):
    w, h, levels, x0, y0 = case
    rng = np.random.default_rng(w * 1000 + h)
    a = np.stack([dc.idwt_input(rng, (h, w), rev), dc.idwt_input(rng, (h, w), rev, tiny=True)])
    got = enc.stage_idwt(a, levels, rev, x0, y0)
    assert np.array_equal(got.view(np.int32), _idwt_ref(oracle, a, levels, rev, x0, y0).view(np.int32))


@pytest.mark.parametrize("rev", TRANSFORMS, ids=["53", "97"])
def test_idwt_small_lines_one_job_per_launch(enc, oracle, rev):
    """The lengths where reflect_idx changes regime, each as the only job of its launches (max_rw / max_rh its own)."""
    rng = np.random.default_rng(77)
    for n in range(1, 14):
        for (x0, y0) in ((0, 0), (1, 1)):
            for (w, h) in ((n, 9), (9, n), (n, n)):
                a = dc.idwt_input(rng, (1, h, w), rev)
                got = enc.stage_idwt(a, 2, rev, x0, y0)
                assert np.array_equal(got.view(np.int32), _idwt_ref(oracle, a, 2, rev, x0, y0).view(np.int32)), (w, h, x0, y0)


@pytest.mark.parametrize("rev", TRANSFORMS, ids=["53", "97"])
def test_idwt_regions_of_different_sizes_in_one_launch(enc, oracle, rev):
    """Eight tiles of one component, sizes and origin parities all different: max_rw / max_rh exceed most jobs' own."""
    regions = [(1, 1, 300, 200, 0, 0), (310, 3, 1, 77, 5, 0), (320, 2, 77, 1, 0, 3), (400, 5, 3, 4, 1, 1), (410, 1, 12, 11, 3, 2),
               (2, 210, 129, 65, 64, 33), (140, 215, 10, 9, 1, 0), (160, 205, 513, 97, 511, 7), (700, 3, 2, 2, 1, 1)]
    rng = np.random.default_rng(99)
    a = np.stack([dc.idwt_input(rng, (310, 720), rev), dc.idwt_input(rng, (310, 720), rev, tiny=True)])
    for levels in (1, 3, 5):
        got = enc.stage_idwt(a, levels, rev, regions=regions)
        for p in range(2):
            want = dc.idwt_regions_reference(oracle, a[p], regions, levels, rev)
            for (x, y, w, h, x0, y0) in regions:
                assert np.array_equal(got[p].view(np.int32)[y:y + h, x:x + w], want.view(np.int32)[y:y + h, x:x + w]), (p, levels, w, h, x0, y0)
            assert np.array_equal(got[p].view(np.int32), want.view(np.int32)), "words between the regions were written"


def test_idwt_stage_rejects_bad_regions(enc):
    from j2k_amd import api
    a = np.zeros((1, 32, 32), dtype=np.int32)
    for bad in ([(0, 0, 33, 8, 0, 0)], [(0, 0, 8, 0, 0, 0)], [(0, 0, 8, 8, 0, 0), (7, 7, 8, 8, 0, 0)]):
        with pytest.raises(api.J2kHipError):
            enc.stage_idwt(a, 1, True, regions=bad)
