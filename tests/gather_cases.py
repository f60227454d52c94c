"""Inputs of the gather stage (j2k_hip_stage_gather, j2k_hip_stage_pack_offsets), shared helpers of test_gather_stage.py:
no fixtures, no tests.  Everything comes from seeded numpy generators.

copy_bytes (gather.hip) copies a piece as a head of up to 3 bytes to the destination's 4-byte boundary, whole words in a
64-lane loop -- assembled from two source words when the source is not aligned with the destination -- and a tail of up
to 3 bytes.  The pieces cover every pair (destination address mod 4, source address mod 4) at the lengths below: head only,
no word, one wave of words exactly (256 bytes + head), the loop's second trip, every tail length.  Device buffers are
256-byte aligned, so an offset's residue mod 4 is the address's.
"""
import numpy as np

LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257, 259, 260, 263, 1023, 1027]
GAP = 8
FILL = 0xC3


def layout(seed=7):
    """(src bytes, blob bytes, dst bytes before, pieces): one piece (dst, src, len) per (dst mod 4, src mod 4, length), laid
    out in both buffers with 8-byte gaps (and whatever the residues ask for on top)."""
    rng = np.random.default_rng(seed)
    pieces, d, s = [], GAP, GAP
    for dm in range(4):
        for sm in range(4):
            for ln in LENGTHS:
                d += (dm - d) % 4
                s += (sm - s) % 4
                pieces.append((d, s, ln))
                d += ln + GAP
                s += ln + GAP
    src = rng.integers(0, 256, size=s + GAP, dtype=np.uint8)
    blob = rng.integers(0, 256, size=s + GAP, dtype=np.uint8)
    dst = np.full(d + GAP, FILL, np.uint8)
    dst[::5] = 0x3C  # (a pattern, so that a word written whole over a gap shows whatever it holds)
    return src, blob, dst, pieces


def expected(dst, lists):
    """numpy's gather: lists = [(source bytes, pieces)]."""
    out = dst.copy()
    for source, pieces in lists:
        for d, s, ln in pieces:
            out[d:d + ln] = source[s:s + ln]
    return out


def pack_lengths(n, seed, near_top=False):
    """n lengths in [0, 4096) with runs of zeros; near_top: near 2^32 - 1, so that a prefix passes 2^32 at once."""
    rng = np.random.default_rng(seed)
    if near_top:
        return ((1 << 32) - 1 - rng.integers(0, 4096, size=n)).astype(np.uint32)
    v = rng.integers(0, 4096, size=n)
    for start in rng.integers(0, max(n, 1), size=max(1, n // 200)):
        v[start:start + int(rng.integers(1, 40))] = 0
    return v.astype(np.uint32)


PACK_COUNTS = [1, 2, 1023, 1024, 1025, 2048, 2049, 5000]
PACK_BASES = [0, 4, (1 << 40) + 12]
