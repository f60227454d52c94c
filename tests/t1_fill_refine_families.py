"""Synthetic code-blocks for the two shortcuts of the Tier-1 modelling kernel that tests/t1_families.py does not aim at
(used by test_t1_fill_refine.py).  Plain helpers: no fixtures, no tests.

  (a) run-length fills: a cleanup stripe in which every column of the block is in run-length mode and holds no 1 is
      written as w identical bytes.  Blocks whose top planes hold a handful of isolated 1 bits over a floor of small
      values: the stripes away from those samples are fills, the ones around them go through the stripe loop, between
      fills, before and after them, in the first and the last stripe of a 32-row half and across the rows 31 | 32;
  (b) the refinement pass: its decision bytes are compacted per stripe by a selector indexed with the refined rows of the
      column and ORed into the stage as words.  Blocks whose top plane holds a chosen pattern of samples, so that the
      refinement pass of the next plane sees exactly that pattern: every 4-row pattern in either stripe of a pair at
      every byte alignment, stripe pairs with a chosen number of refined samples, refined samples with and without
      significant neighbours beside samples refined before.

Magnitudes are integers (the reversible path codes them as they are; the 9/7 path scales them by a constant, which keeps
what is isolated isolated and what is equal equal).
"""
import numpy as np

FLUSH = 1024  # the kernel's stage leaves for memory in pieces of this many decisions

FILL_SHAPES = [(w, h) for h in (64, 32) for w in (1, 3, 17, 33, 63, 64)] + [(64, 62), (63, 35), (33, 30), (17, 61), (3, 47), (64, 7)]


def _signs(rng, shape):
    return np.where(rng.random(shape) < 0.5, -1, 1)


def fill_block(rng, w, h, spots, floor_bits=3):
    """Random magnitudes below 2^floor_bits and the samples `spots` = [(row, column, value)] above them."""
    b = rng.integers(0, 1 << floor_bits, size=(h, w)) if floor_bits else np.zeros((h, w), dtype=np.int64)
    for y, x, v in spots:
        b[y % h, x % w] = v
    return (b * _signs(rng, (h, w))).astype(np.int64)


def fill_families(rng):
    """[(block, orientation)]: every shape of FILL_SHAPES with 1, 2 ... isolated samples one to three planes above the rest."""
    cases = []
    k = 0
    for w, h in FILL_SHAPES:
        last = h - 1
        layouts = [
            [(0, 0, 0x700)],                                          # first stripe, column 0 only
            [(last, w - 1, 0x400)],                                   # last row (a partial stripe where h % 4), last column only
            [(31, w // 2, 0x500), (32, w // 3, 0x280)],               # either side of the rows 31 | 32
            [(9, 1, 0x600), (22, w - 2, 0x300), (23, 0, 0x180)],      # fills before, between and after dense stripes
            [(3, w - 1, 0x440), (4, 0, 0x220), (28, w // 2, 0x110)],  # last row of a stripe / first of the next, last stripe of a half
            [(h // 2, w // 2, 0x7ff)],                                # one sample whose lower planes are all 1
        ]
        for spots in layouts:
            for i, floor_bits in enumerate((0, 3, 6)):
                if (k + i) % 3 == 0 or w >= 63:  # all floors for the widest blocks, one of them for the others
                    cases.append((fill_block(rng, w, h, spots, floor_bits), k % 4))
            k += 1
    # many isolated samples: 2 .. 40 of them, one to three planes above a floor of 2 bits
    for n in (2, 3, 5, 8, 13, 21, 40):
        for w, h in ((64, 64), (64, 32), (63, 64), (33, 61)):
            spots = [(int(rng.integers(0, h)), int(rng.integers(0, w)), int(rng.integers(1 << 5, 1 << 8))) for _ in range(n)]
            cases.append((fill_block(rng, w, h, spots, 2), k % 4))
            k += 1
    return cases


def flush_crossing_blocks():
    """Blocks in which fills cross the 1 KiB flush of the stage at every offset mod 4, and the fills' stream positions.

    One sample in row 62 carries several planes above an empty block.  In every plane the significance pass then codes the
    sample's 8 (5 at the block's edge) neighbours, the refinement pass one decision, and the cleanup pass writes stripes
    0 .. 14 as fills -- 15 x w bytes from the start of the pass -- and then stripe 15.  The oracle's per-pass decision
    counts give the start of every cleanup pass, so a test can tell where each fill lies (fill_positions).  Widths and the
    sample's column (edge or not: 5 or 8 neighbours) vary the phase.  Deterministic: no random numbers."""
    blocks = []
    for w in (64, 63, 33, 17, 64, 64, 63, 64):
        x = (0, 5, w - 1, 7)[len(blocks) % 4]
        b = np.zeros((64, w), dtype=np.int64)
        b[62, x] = 0x3a5 + 2 * len(blocks) if len(blocks) % 2 else -(0x2d3 + 2 * len(blocks))
        if len(blocks) >= 4:  # a second sample beside it: other counts in stripe 15
            b[61, (x + 1) % w] = 0x155
        blocks.append(b)
    return [(b, i % 4) for i, b in enumerate(blocks)]


def fill_positions(block, pass_nsym):
    """Stream positions (first byte, length) of the fills of stripes 0 .. 14 of a flush_crossing_blocks() block: the start of
    each cleanup pass (passes 0, 3, 6 ...) + k * w, for the planes in which nothing above row 56 is significant yet -- all of
    them here."""
    w = block.shape[1]
    out = []
    for p in range(0, len(pass_nsym), 3):
        start = pass_nsym[p - 1] if p else 0
        out += [(start + k * w, w) for k in range(15)]
    return out


def crosses_flush(pos, n):
    return (pos + n) // FLUSH > pos // FLUSH


# ---- (b) refinement
def pattern_block(shift, top=9, w=64, h=64, low=None):
    """Column c, stripe s holds samples of magnitude 2^top (+ low bits) in the rows of the 4-bit pattern
    (5 c + 3 s + shift) % 16 -- every pattern in every stripe, 64 / 16 times, at whatever byte offsets the columns before it
    leave.  Everything else is 0: the refinement pass of the plane below the top one refines exactly these samples."""
    b = np.zeros((h, w), dtype=np.int64)
    for s in range(h // 4):
        for c in range(w):
            p = pattern_of(c, s, shift)
            for r in range(4):
                if (p >> r) & 1:
                    b[4 * s + r, c] = (1 << top) | (0 if low is None else int(low[4 * s + r, c]))
    return b


def pattern_of(c, s, shift):
    return (5 * c + 3 * s + shift) % 16


def pattern_coverage(shift, start, w=64, h=64):
    """(stripe of the pair, pattern, stream position mod 4 of the column's first byte) of every column-stripe of the first
    refinement pass of a pattern_block(), which starts at stream position `start`."""
    seen = set()
    pos = start
    for s in range(h // 4):
        for c in range(w):
            p = pattern_of(c, s, shift)
            seen.add((s % 2, p, pos % 4))
            pos += bin(p).count("1")
    return seen


PAIR_COUNTS = (1, 63, 64, 447, 448, 511, 512, 0)


def pair_count_block(counts=PAIR_COUNTS, top=8, order=0):
    """Stripe pair j (rows 8 j .. 8 j + 7) holds counts[j] samples of magnitude 2^top + 1, the first ones in scan order
    (order 0) or the last ones (order 1): the refinement pass below the top plane refines exactly that many in the pair."""
    b = np.zeros((64, 64), dtype=np.int64)
    for j, n in enumerate(counts):
        cells = [(8 * j + 4 * s + r, c) for s in range(2) for c in range(64) for r in range(4)]
        for y, x in (cells[:n] if order == 0 else cells[len(cells) - n:]):
            b[y, x] = (1 << top) + 1
    return b


def mixed_age_block(rng, w, h):
    """Samples that become significant in three successive planes, side by side and alone: in the planes below, one stripe
    holds first refinements with and without significant neighbours next to later refinements."""
    b = np.zeros((h, w), dtype=np.int64)
    tops = rng.integers(0, 6, size=(h, w))  # 0, 1, 2: significant from plane 10, 9, 8; the others empty
    for t, top in ((0, 10), (1, 9), (2, 8)):
        b = np.where(tops == t, (1 << top) | rng.integers(0, 1 << top, size=(h, w)), b)
    # isolated ones in an empty quarter (no neighbour: context 14 at the first refinement)
    b[: h // 2, : w // 2] = 0
    for y in range(1, h // 2 - 1, 3):
        for x in range(1 + (y % 2), w // 2 - 1, 3):
            b[y, x] = (1 << (8 + (x + y) % 3)) | int(rng.integers(0, 1 << 8))
    return (b * _signs(rng, (h, w))).astype(np.int64)


def refine_families(rng):
    cases = []
    for shift in range(8):  # (the shifts move every pattern to other columns: other offsets in front of it)
        cases.append((pattern_block(shift), shift % 4))
    low = rng.integers(0, 1 << 9, size=(64, 64))
    for shift, w, h in ((1, 64, 64), (2, 63, 64), (3, 33, 64), (4, 17, 62), (5, 3, 64), (6, 1, 64), (7, 64, 32), (8, 50, 35)):
        cases.append((pattern_block(shift, 9, w, h, low) * _signs(rng, (h, w)), shift % 4))
    for order in (0, 1):
        for rot in range(4):
            counts = PAIR_COUNTS[rot:] + PAIR_COUNTS[:rot]
            cases.append((pair_count_block(counts, 8, order) * _signs(rng, (64, 64)), (order + rot) % 4))
    for w, h in ((64, 64), (64, 64), (64, 32), (63, 64), (33, 64), (17, 64), (3, 63), (1, 64), (64, 30)):
        cases.append((mixed_age_block(rng, w, h), (w + h) % 4))
    # dense blocks of narrow widths with long streams: many flushes inside refinement passes
    for w in (63, 47, 33, 17, 5):
        cases.append((np.rint(rng.laplace(0, 300, size=(64, w))).astype(np.int64), w % 4))
    return cases
