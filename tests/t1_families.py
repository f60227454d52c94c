"""Synthetic code-blocks built to hit the edges of the Tier-1 kernels, shared by the encode-side tests
(test_t1_emission.py, test_t1_sparse_pass.py) and their decode-side mirror (test_decode_stages.py).  Plain helpers: no
fixtures, no tests.

  (a) emission families: every width 1..64, heights that are not multiples of 4, 32-row blocks, stripe columns at the
      10-decision maximum of run-length mode, full blocks with long streams;
  (b) sparse families: 64 x 64 Gaussian / Laplacian magnitudes at scales 2^4 .. 2^12, isolated significant samples and
      single significant rows / columns at block edges and stripe boundaries (rows 3|4, 31|32, 63; columns 0 and 63), a
      sweep of the fraction of non-zero samples, partial last stripes.
"""
import numpy as np


# ---- (a) the emission families
def max_stripes(rng, w, h, top):
    """Odd columns of even stripes carry the top bit-plane with their first 1 in row (column // 2 + stripe // 2) % 5 of
    the stripe (4 = none), everything else lies below it: run-length columns of up to 10 decisions per lane."""
    blk = rng.integers(0, 1 << (top - 2), size=(h, w))
    for s in range(0, h, 8):
        for c in range(1, w, 2):
            r = (c // 2 + s // 8) % 5
            if r < 4 and s + 4 <= h:
                rows = slice(s + r, s + 4)
                blk[rows, c] = (1 << top) | rng.integers(0, 1 << top, size=blk[rows, c].shape)
    return blk * np.where(rng.random((h, w)) < 0.5, -1, 1)


def random_block(rng, w, h, kind):
    if kind == 0:  # dense, Laplacian-like
        v = np.rint(rng.laplace(0, 200, size=(h, w)))
    elif kind == 1:  # a few large values among zeros
        v = np.where(rng.random((h, w)) < 0.05, rng.integers(-4000, 4000, size=(h, w)), 0)
    elif kind == 2:  # everything at one magnitude
        v = np.full((h, w), 1 << 9) * np.where(rng.random((h, w)) < 0.5, -1, 1)
    else:  # mixed scales by column
        v = np.rint(rng.standard_normal((h, w)) * (1 << rng.integers(1, 12, size=(1, w))))
    return v.astype(np.int64)


def emission_families(rng):
    blocks = []
    heights = [1, 2, 3, 5, 6, 7, 13, 31, 32, 33, 37, 61, 62, 63, 64]
    for w in range(1, 65):
        blocks.append(random_block(rng, w, heights[w % len(heights)], w % 4))
    for h in (64, 32, 63, 30):
        for w in (64, 63, 33, 17):
            blocks.append(max_stripes(rng, w, h, 10 + (w % 3)))
    for i in range(16):
        blocks.append(random_block(rng, 64, 64 if i % 4 else 32, i % 4))
    return [(b, i % 4) for i, b in enumerate(blocks)]


# ---- (b) the sparse regime
def signs(rng, shape):
    return np.where(rng.random(shape) < 0.5, -1, 1)


def sparse_families(rng):
    shapes = []
    # magnitudes at scales 2^4 .. 2^12: the planes below the scale are nearly all significant, those above nearly empty
    for e in range(4, 13):
        shapes.append(np.rint(rng.standard_normal((64, 64)) * (1 << e)))
        shapes.append(np.rint(rng.laplace(0, 1 << e, size=(64, 64))))
    # isolated significant samples, rows and columns at the block's edges and at stripe boundaries, over a floor of small
    # values so that the planes below the spike propagate from it sample by sample
    spots = [(0, 0), (0, 63), (63, 0), (63, 63), (3, 17), (4, 17), (31, 40), (32, 40), (3, 0), (4, 63), (31, 63), (32, 0)]
    for floor in (0, 3):
        b = rng.integers(0, floor + 1, size=(64, 64)) * signs(rng, (64, 64))
        for k, (y, x) in enumerate(spots):
            b[y, x] = (1 << (6 + k % 5)) + k
        shapes.append(b)
        for y, x in spots[:8]:  # one at a time
            b = rng.integers(0, floor + 1, size=(64, 64)) * signs(rng, (64, 64))
            b[y, x] = -(1 << 9) - 5
            shapes.append(b)
        for row in (0, 3, 4, 31, 32, 63):
            b = rng.integers(0, floor + 1, size=(64, 64)) * signs(rng, (64, 64))
            b[row, :] = rng.integers(1 << 7, 1 << 9, size=64) * signs(rng, 64)
            shapes.append(b)
        for col in (0, 1, 31, 32, 62, 63):
            b = rng.integers(0, floor + 1, size=(64, 64)) * signs(rng, (64, 64))
            b[:, col] = rng.integers(1 << 7, 1 << 9, size=64) * signs(rng, 64)
            shapes.append(b)
    # density sweep: the fraction of non-zero samples, two amplitude ranges each
    for frac in (0.001, 0.003, 0.01, 0.02, 0.04, 0.07, 0.1, 0.15, 0.2, 0.3):
        for top in (7, 12):
            mag = rng.integers(1, 1 << top, size=(64, 64))
            shapes.append(np.where(rng.random((64, 64)) < frac, mag, 0) * signs(rng, (64, 64)))
    # heights of one half and partial last stripes in the sparse regime
    for h, w in ((32, 64), (33, 64), (47, 50), (64, 9)):
        shapes.append(np.where(rng.random((h, w)) < 0.03, rng.integers(1, 1 << 10, size=(h, w)), 0) * signs(rng, (h, w)))
    # every shape under all four orientations
    return [(np.asarray(b, dtype=np.int64), o) for b in shapes for o in range(4)]


def layout(cases):
    """One 64 x 64 cell per block in a plane of 16 cells per row (the kernel rewrites each block in place)."""
    ncol = 16
    nrow = (len(cases) + ncol - 1) // ncol
    coef = np.zeros((64 * nrow, 64 * ncol), dtype=np.int64)
    rects, orients = [], []
    for i, (b, o) in enumerate(cases):
        h, w = b.shape
        x, y = 64 * (i % ncol), 64 * (i // ncol)
        coef[y:y + h, x:x + w] = b
        rects.append((x, y, w, h))
        orients.append(o)
    return coef, rects, orients
