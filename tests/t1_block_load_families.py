"""Synthetic code-blocks aimed at the block load of the Tier-1 modelling kernel (used by test_t1_block_load.py): a block of
64 or 32 rows is read 32 rows at a time, scaled to sign-magnitude in registers, transposed to one word per bit-plane and
the plane words are written over the block's own rows; any other height scales its samples in place.  Plain helpers: no
fixtures, no tests.

Every group is a dict: plane (int64 for the reversible path; the 9/7 plane is given as float32 or derived from the
integers), rects [(x, y, w, h)], orients, and for the 9/7 path one step size per block.

  shapes      the block shapes of either path: 64 x 64, 32 x 32, w 64 x h 32, w 32 x h 64, w 17 x h 64, w 1 x h 64 (plane
              words), heights 5, 31, 33, 63 (in place), four kinds of content each;
  neighbours  a plane 150 words wide tiled without a gap by blocks of widths 17, 64, 32, 1, 36 and heights 64, 32, 33,
              5, 63, 31: a word stored by a lane beyond the block's width, or into a row of the block below, lands in a
              neighbour that is compared too;
  walking     64 x 64 blocks of independent random bits for every number of bit-planes 1 .. 25 (the most a 32-bit word
              with 6 fractional bits holds without its top bit; 25 planes are 73 passes, fewer than the 96 the pass
              tables hold, so the kernel's "more bit-planes than the tables hold" branch cannot be reached from any
              coefficient word), signs mixed: the 64 column bits of every (row, plane) pair differ from those of every
              other pair, so a transposition that swaps two rows or two planes changes the decisions; plus an all-zero
              block and blocks of the largest magnitudes;
  values      (9/7 only) per step size 2^k, (1 + 2047/2048) 2^k and 2^-13: quotients exactly on a rounding tie, |f| just
              below, at and just above stepsize / 128, -0.0, the smallest subnormal and the smallest normal float, the
              largest magnitudes the word holds, over random mantissas at all scales.
"""
import numpy as np

from t1_families import layout, random_block

FRAC = 6
MAX_PLANES = 25  # |q| < 2^31 with 6 fractional bits
PLANE_SHAPES = [(64, 64), (32, 32), (64, 32), (32, 64), (17, 64), (1, 64)]  # (w, h)
INPLACE_HEIGHTS = [5, 31, 33, 63]
STEPS = [1.0, 2.0 ** -3, 2.0 ** 4, (1 + 2047 / 2048) * 1.0, (1 + 2047 / 2048) * 2.0 ** -5, (1 + 2047 / 2048) * 2.0 ** 3, 2.0 ** -13]


def _signs(rng, shape):
    return np.where(rng.random(shape) < 0.5, -1, 1)


def _group(cases, steps=None):
    plane, rects, orients = layout(cases)
    return dict(plane=plane, rects=rects, orients=orients, steps=steps)


def shapes_group(rng):
    cases = []
    k = 0
    for w, h in PLANE_SHAPES + [(w, h) for h in INPLACE_HEIGHTS for w in (64, 17)]:
        for kind in range(4):
            cases.append((random_block(rng, w, h, kind), k % 4))
            k += 1
    return _group(cases)


NEIGHBOUR_WIDTHS = [17, 64, 32, 1, 36]
NEIGHBOUR_HEIGHTS = [64, 32, 33, 5, 63, 31]


def neighbours_group(rng):
    W, H = sum(NEIGHBOUR_WIDTHS), sum(NEIGHBOUR_HEIGHTS)
    plane = (np.rint(rng.laplace(0, 300, size=(H, W))) + _signs(rng, (H, W))).astype(np.int64)  # (no block is empty)
    rects, orients = [], []
    y = 0
    for h in NEIGHBOUR_HEIGHTS:
        x = 0
        for w in NEIGHBOUR_WIDTHS:
            rects.append((x, y, w, h))
            orients.append(len(rects) % 4)
            x += w
        y += h
    return dict(plane=plane, rects=rects, orients=orients, steps=None)


def walking_block(rng, planes):
    """64 x 64 magnitudes of `planes` random bits, the top plane set in one sample of every row at least, mixed signs."""
    mag = rng.integers(0, 1 << planes, size=(64, 64), dtype=np.int64)
    mag[np.arange(64), rng.permutation(64)] |= 1 << (planes - 1)
    return mag * _signs(rng, (64, 64))


def walking_blocks(rng):
    blocks = [walking_block(rng, n) for n in range(1, MAX_PLANES + 1)]
    top = (1 << MAX_PLANES) - 1
    largest = np.full((64, 64), top, dtype=np.int64)
    largest[::3, ::5] -= rng.integers(0, 1 << 12, size=largest[::3, ::5].shape)
    largest *= _signs(rng, (64, 64))
    return blocks + [np.zeros((64, 64), dtype=np.int64), largest, np.full((32, 32), -top, dtype=np.int64)]


def walking_group(rng):
    return _group([(b, i % 4) for i, b in enumerate(walking_blocks(rng))])


def row_plane_vectors(block):
    """The 64 column bits of every (row, plane) pair of a 64 x 64 block as integers, and its sign rows."""
    mag = np.abs(block)
    planes = int(mag.max()).bit_length()
    weights = 1 << np.arange(64, dtype=object)
    vec = {(r, p): int((((mag[r] >> p) & 1).astype(object) * weights).sum()) for r in range(64) for p in range(planes)}
    signs = [int(((block[r] < 0).astype(object) * weights).sum()) for r in range(64)]
    return vec, signs


# ---- the 9/7 quantiser's edges
def ties(step, n):
    """n floats f with f / step * 64 exactly on k + 1/2 (k even and odd, both signs): (2 k + 1) * mantissa(step) fits a float."""
    ks = np.arange(n, dtype=np.int64)
    f = (np.float64(step) * (2 * ks + 1) / 128.0)
    f32 = f.astype(np.float32)
    assert (f32.astype(np.float64) == f).all()
    return f32 * np.where(ks % 4 < 2, 1, -1).astype(np.float32)


def dead_zone(step):
    """|f| just below, at and just above step / 128 (f / step * 64 = 1/2: rounds to 0, the neighbours to 0 and 1), both signs."""
    e = np.float32(np.float64(step) / 128.0)
    lo, hi = np.nextafter(e, np.float32(0)), np.nextafter(e, np.float32(np.inf))
    return np.array([lo, e, hi, -lo, -e, -hi], dtype=np.float32)


def tiny():
    return np.array([-0.0, 0.0, 1e-45, -1e-45, np.finfo(np.float32).tiny, -np.finfo(np.float32).tiny], dtype=np.float32)


def largest(step):
    """The largest |f| whose scaled magnitude stays below 2^31, and a few below it."""
    lim = np.float32(np.float64(step) * (2.0 ** 25))
    out = []
    v = lim
    for _ in range(4):
        v = np.nextafter(v, np.float32(0))
        v = np.nextafter(v, np.float32(0))  # (two steps: the quotient by a step size with a long mantissa may round up)
        out += [v, -v]
    return np.array(out, dtype=np.float32)


def values_block(rng, step, big):
    """64 x 64 floats: random mantissas at scales 2^-9 .. 2^10 of the step size (2^23 with `big`), then rows 0, 31, 32 and 63
    and columns 0 and 63 carry the edge values."""
    scale = np.float64(step) * 2.0 ** rng.integers(-9, 24 if big else 11, size=(64, 64))
    b = (rng.random((64, 64)) + 1.0) * scale * _signs(rng, (64, 64))
    b = b.astype(np.float32)
    t = ties(step, 64)
    b[0, :] = t
    b[32, :] = -t[::-1]
    edge = np.concatenate([dead_zone(step), tiny(), largest(step) if big else dead_zone(step)])
    b[31, :edge.size] = edge
    b[63, 64 - edge.size:] = edge
    b[1:1 + edge.size, 0] = edge
    b[40:40 + edge.size, 63] = edge
    return b


def values_group(rng):
    """One full block per step size with the largest magnitudes and one without, a 32 x 32 and a 17 x 64 cut of each."""
    blocks, steps = [], []
    for step in STEPS:
        for big in (False, True):
            b = values_block(rng, step, big)
            for cut in (b, b[:32, :32], b[:, 47:]):
                blocks.append(cut)
                steps.append(float(np.float32(step)))
    ncol = 16
    nrow = (len(blocks) + ncol - 1) // ncol
    plane = np.zeros((64 * nrow, 64 * ncol), dtype=np.float32)
    rects, orients = [], []
    for i, b in enumerate(blocks):
        h, w = b.shape
        x, y = 64 * (i % ncol), 64 * (i // ncol)
        plane[y:y + h, x:x + w] = b
        rects.append((x, y, w, h))
        orients.append(i % 4)
    return dict(plane=plane, rects=rects, orients=orients, steps=steps)


GROUPS = {"shapes": (shapes_group, 4101), "neighbours": (neighbours_group, 4102), "walking": (walking_group, 4103),
          "values": (values_group, 4104)}


def group(name):
    make, seed = GROUPS[name]
    return make(np.random.default_rng(seed))
