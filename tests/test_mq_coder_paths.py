"""The two-wave MQ coder's lane stage and table look-ups on the GPU (run with -m gpu): 134 blocks of 64 x 64, that is two
full coder workgroups (one lane per block) and one with 6 live lanes, mixed so that the lanes of a workgroup differ as much
as they can: full-amplitude noise (about 7 KB of codeword) beside blocks of a few bytes, all-zero blocks and everything
between, the longest block in the first lane and the shortest in the last.  The flush of the codeword stage runs for all
lanes at once, triggered by one lane while the others hold anything from nothing to several 16-byte units; after it every
lane moves its remainder to the front of its stage, and the byte count is derived from the lane's store pointer at every
pass end (the per-pass rates read it) and at the end.  Coded bytes, bit-plane and pass counts, lengths and per-pass rates
are compared with the CPU oracle, reversible and 9/7.

What the mix is meant to hit is asserted on the oracle's outputs first: codeword lengths in every residue mod 16, a spread
of at least 8 between the longest and the shortest non-empty codeword of every workgroup, a block shorter than 16 bytes,
and a coded 0xFF with its stuffed successor."""
import numpy as np
import pytest

from t1_families import layout as _layout, random_block as _random_block, signs as _signs

pytestmark = pytest.mark.gpu

NBLOCKS = 134  # 64 + 64 + 6
SEED = 20


def _noise(rng, bits):
    return rng.integers(-(1 << bits) + 1, 1 << bits, size=(64, 64))


def _few(rng, n, top):
    b = np.zeros((64, 64), dtype=np.int64)
    ys, xs = rng.integers(0, 64, size=n), rng.integers(0, 64, size=n)
    b[ys, xs] = rng.integers(1, 1 << top, size=n) * _signs(rng, n)
    return b


def _workgroup(rng, lanes):
    """The blocks of one coder workgroup: lane 0 the longest, the last lane the shortest that is not empty."""
    blocks = []
    for lane in range(lanes):
        k = lane % 8
        if lane == 0:
            b = _noise(rng, 16)  # the longest: noise over the whole 16-bit range
        elif lane == lanes - 1:
            b = np.zeros((64, 64), dtype=np.int64)
            b[int(rng.integers(0, 64)), int(rng.integers(0, 64))] = 2  # the shortest: one sample, one bit-plane
        elif k in (1, 5):
            b = _noise(rng, 13 + lane % 3)  # long streams
        elif k == 2:
            b = _few(rng, 1 + lane % 5, 3 + lane % 4)  # a few bytes
        elif k == 3:
            b = np.zeros((64, 64), dtype=np.int64)  # nothing at all
        elif k == 4:
            b = np.where(rng.random((64, 64)) < 0.002 * (1 + lane % 7), rng.integers(1, 1 << (4 + lane % 9), size=(64, 64)), 0) * _signs(rng, (64, 64))
        elif k == 6:
            b = _random_block(rng, 64, 64, lane % 4)
        else:
            b = np.rint(rng.laplace(0, 1 << (lane % 11), size=(64, 64))).astype(np.int64)
        blocks.append(np.asarray(b, dtype=np.int64))
    return blocks


def _blocks(seed):
    rng = np.random.default_rng(seed)
    blocks = _workgroup(rng, 64) + _workgroup(rng, 64) + _workgroup(rng, NBLOCKS - 128)
    return [(b, i % 4) for i, b in enumerate(blocks)]


def _plane_and_refs(oracle, rev):
    """The plane handed to the encoder, its rectangles and orientations, and the oracle's result per block."""
    coef, rects, orients = _layout(_blocks(SEED))
    step = 1.0 if rev else 0.37
    plane = coef.astype(np.int32) if rev else (coef * 0.61).astype(np.float32)
    quant = oracle.L.j2ko_quant97
    refs = []
    for (x, y, w, h), o in zip(rects, orients):
        blk = plane[y:y + h, x:x + w]
        if rev:
            data = (blk.astype(np.int64) << 6).astype(np.int32)
        elif not blk.any():
            data = np.zeros((h, w), dtype=np.int32)
        else:
            data = np.array([[quant(float(v), step) if v else 0 for v in row] for row in blk], dtype=np.int32)
        refs.append(oracle.t1_block(data, o))
    return plane, rects, orients, step, refs


@pytest.fixture(scope="module", params=[True, False], ids=["rev", "irr"])
def case(request, oracle):
    return (request.param,) + _plane_and_refs(oracle, request.param)


@pytest.fixture(scope="module")
def enc():
    from j2k_amd import api
    e = api.Encoder(0)
    yield e
    e.close()


def check_mix(refs):
    """The four conditions on the oracle's codewords, and where the longest and the shortest block sit."""
    assert len(refs) == NBLOCKS
    lens = [len(r["data"]) for r in refs]
    live = [n for n in lens if n]
    assert {n % 16 for n in live} == set(range(16)), sorted({n % 16 for n in live})
    for g in range(0, NBLOCKS, 64):
        grp = lens[g:g + 64]
        some = [n for n in grp if n]
        assert max(some) >= 8 * min(some), (g, max(some), min(some))
        assert grp[0] == max(grp) and grp[-1] == min(some), (g, grp[0], grp[-1], max(grp), min(some))
        assert 0 in grp, g
    assert any(0 < n < 16 for n in lens)
    assert max(lens) > 6500  # the long streams: hundreds of flushes of the stage
    assert any(b"\xff" in r["data"][:-1] for r in refs)  # (a 0xFF inside a codeword is always followed by a stuffed byte)


def test_mix_meets_its_conditions(case):
    check_mix(case[5])


@pytest.mark.parametrize("passes", [False, True], ids=["plain", "dist"])
def test_mq_coder_matches_oracle(enc, case, passes):
    rev, plane, rects, orients, step, refs = case
    check_mix(refs)
    got = enc.stage_t1(plane.copy(), rects, orients, [step] * len(rects), rev, want_passes=passes)
    assert len(got) == NBLOCKS
    for i, (g, ref) in enumerate(zip(got, refs)):
        where = (i // 64, i % 64)  # workgroup, lane
        assert g["numbps"] == ref["numbps"], where
        assert g["npasses"] == ref["npasses"], where
        assert g["length"] == len(ref["data"]), where
        assert g["data"] == ref["data"], where
        if passes:
            assert g["rates"] == ref["rates"], where
            assert g["nmsedec"] == ref["nmsedec"], where
