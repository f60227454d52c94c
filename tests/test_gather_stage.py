"""GPU: the codestream assembly alone (gather.hip: gather_kernel with copy_bytes, pack_offsets_kernel) through
j2k_hip_stage_gather and j2k_hip_stage_pack_offsets, against numpy.  The whole destination buffer is compared: the bytes of
every piece, the gaps between pieces and the bytes around them.

Pieces (gather_cases.py): every pair (destination address mod 4, source address mod 4) at lengths 0 .. 1027, each list
through each of the kernel's three roles -- blocks (a code-block table, 4-byte aligned sources, zero lengths skipped),
headers (32-bit offsets into the blob), segments (64-bit offsets) -- alone and all three in one launch, where a role's
index is its workgroup's number less the counts of the roles before it.  Header pieces read a blob of other bytes than
the codeword arena, so a role that reads the wrong buffer shows.

Reads outside a piece's source.  A test cannot see them without provoking a fault and does not try; the argument is in
copy_bytes itself.  Head and tail read src[lane] for lane < len only.  The word loop reads aligned words sw[i], i < words,
where sw is the source pointer behind the head rounded DOWN to a word: with an aligned source these are bytes of the piece;
with a misaligned one sw[0] starts up to three bytes before the piece's first word byte -- inside the same aligned word, so
inside any allocation that holds the piece's first byte -- and sw[i + 1] is read only while i + 1 < src_words, the number of
aligned words that hold bytes of the piece: the last of them may end up to three bytes behind the piece, again inside the
aligned word that holds its last byte.  Device allocations start on 256-byte boundaries and the hook's have at least 64
spare bytes, as a frame's.
"""
import numpy as np
import pytest

import gather_cases as gc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from j2k_amd import api
    return api


@pytest.fixture(scope="module")
def enc(api):
    e = api.Encoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def lay():
    return gc.layout()


def test_the_pieces_cover_every_alignment_pair_and_length(lay):
    src, blob, dst, pieces = lay
    assert {(d % 4, s % 4, ln) for d, s, ln in pieces} == {(a, b, ln) for a in range(4) for b in range(4) for ln in gc.LENGTHS}
    ends = sorted((d, d + ln) for d, s, ln in pieces)
    assert all(b[0] - a[1] >= gc.GAP for a, b in zip(ends, ends[1:]))


@pytest.mark.parametrize("role", ["blocks", "headers", "segments"])
def test_each_role_alone(enc, lay, role):
    src, blob, dst, pieces = lay
    if role == "blocks":
        pieces = [p for p in pieces if p[1] % 4 == 0]
        assert len(pieces) == 4 * len(gc.LENGTHS)
    source = blob if role == "headers" else src
    got = enc.stage_gather(src, dst, blob=blob, **{role: pieces})
    want = gc.expected(dst, [(source, pieces)])
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:20]


def test_all_roles_in_one_launch(enc, lay):
    src, blob, dst, pieces = lay
    aligned = [p for p in pieces if p[1] % 4 == 0]
    rest = [p for p in pieces if p[1] % 4]
    blocks, headers, segments = aligned[::2], aligned[1::2] + rest[::2], rest[1::2]
    assert blocks and headers and segments
    got = enc.stage_gather(src, dst, blob=blob, blocks=blocks, headers=headers, segments=segments)
    want = gc.expected(dst, [(src, blocks), (blob, headers), (src, segments)])
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:20]


def test_pieces_that_touch_the_buffers_ends(enc):
    """A piece at offset 0 and one that ends with its source and with the destination: nothing before, nothing behind."""
    rng = np.random.default_rng(11)
    src = rng.integers(0, 256, size=601, dtype=np.uint8)
    dst = np.full(700, gc.FILL, np.uint8)
    segs = [(0, 0, 259), (700 - 341, 601 - 341, 341)]
    got = enc.stage_gather(src, dst, segments=segs)
    assert np.array_equal(got, gc.expected(dst, [(src, segs)]))
    got = enc.stage_gather(src, dst, headers=segs)
    assert np.array_equal(got, gc.expected(dst, [(src, segs)]))


def test_refusals(api, enc, lay):
    src, blob, dst, pieces = lay
    S, D = src.size, dst.size
    bad = [dict(segments=[(0, S - 3, 4)]), dict(segments=[(D - 3, 0, 4)]), dict(headers=[(0, S - 3, 4)]), dict(headers=[(D, 0, 1)]),
           dict(blocks=[(0, 2, 4)]), dict(blocks=[(0, S - S % 4, 8)]), dict(segments=[(1 << 40, 0, 1)]), dict(segments=[(0, 1 << 40, 1)]),
           dict(segments=[(10, 0, 8)], headers=[(17, 0, 4)]), dict(blocks=[(4, 0, 8)], segments=[(0, 0, 5)])]
    for kw in bad:
        with pytest.raises(api.J2kHipError) as x:
            enc.stage_gather(src, dst, blob=blob, **kw)
        assert x.value.code == 1, kw  # J2K_HIP_ERR_PARAM
    # pieces that only touch, and a block of length 0 inside another piece's destination (it is skipped), are fine
    ok = enc.stage_gather(src, dst, blob=blob, segments=[(10, 0, 8)], headers=[(18, 0, 4)], blocks=[(12, 0, 0)])
    assert np.array_equal(ok, gc.expected(dst, [(src, [(10, 0, 8)]), (blob, [(18, 0, 4)])]))
    assert np.array_equal(enc.stage_gather(src, dst), dst)


@pytest.mark.parametrize("n", gc.PACK_COUNTS)
def test_pack_offsets(enc, n):
    lens = gc.pack_lengths(n, n)
    for base in gc.PACK_BASES:
        got = enc.stage_pack_offsets(lens, base)
        want = np.uint64(base) + np.concatenate([[0], np.cumsum(lens.astype(np.uint64))[:-1]]).astype(np.uint64)
        assert np.array_equal(got, want), (n, base, np.flatnonzero(got != want)[:10])


def test_pack_offsets_past_32_bits(enc):
    for n in (3, 1025, 2049):
        lens = gc.pack_lengths(n, 100 + n, near_top=True)
        got = enc.stage_pack_offsets(lens, (1 << 40) + 12)
        want = np.uint64((1 << 40) + 12) + np.concatenate([[0], np.cumsum(lens.astype(np.uint64))[:-1]]).astype(np.uint64)
        assert int(want[-1]) - (1 << 40) > 1 << 32 or n < 3
        assert np.array_equal(got, want), n


def test_pack_offsets_of_nothing(enc):
    """n = 0: no launch, dst is left alone."""
    assert enc.stage_pack_offsets(np.array([], np.uint32), 5).size == 0
    dst = np.full(4, 0x1122334455667788, np.uint64)
    lens = np.full(4, 9, np.uint32)
    assert enc.L.j2k_hip_stage_pack_offsets(enc.h, lens.ctypes.data, 0, 5, dst.ctypes.data) == 0
    assert np.array_equal(dst, np.full(4, 0x1122334455667788, np.uint64))
