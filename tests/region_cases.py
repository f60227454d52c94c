"""Shapes, windows and poisoned planes shared by the region-decode tests (test_region_footprint.py on the CPU,
test_idwt_window.py on the GPU).

The shapes are the smallest at which the footprint arithmetic can go wrong: odd sizes, an origin of odd parity on both
axes (parity decides which band a sample is in), and 1 .. 4 levels -- at 4 levels of an 8 x 5 plane resolutions are one
sample wide or empty."""
import numpy as np

SHAPES = [(37, 29), (8, 5)]          # (width, height)
ORIGINS = [(0, 0), (3, 5)]
LEVELS = [1, 2, 3, 4]
CASES = [(w, h, x0, y0, lv, rev) for (w, h) in SHAPES for (x0, y0) in ORIGINS for lv in LEVELS for rev in (True, False)]


def case_id(c):
    w, h, x0, y0, lv, rev = c
    return f"{w}x{h}-at{x0}_{y0}-{lv}lvl-{'53' if rev else '97'}"


def windows(w, h, seed):
    """(x, y, w, h): each corner pixel, a 1-wide column, a 1-high row at the last row, the whole plane, 20 random ones."""
    ws = [(0, 0, 1, 1), (w - 1, 0, 1, 1), (0, h - 1, 1, 1), (w - 1, h - 1, 1, 1),
          (w // 2, 0, 1, h), (0, h - 1, w, 1), (0, 0, w, h)]
    rng = np.random.default_rng(seed)
    for _ in range(20):
        x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
        ws.append((x, y, int(rng.integers(1, w - x + 1)), int(rng.integers(1, h - y + 1))))
    return ws


def plane(rng, w, h, rev):
    if rev:
        return rng.integers(-4000, 4000, size=(h, w)).astype(np.int32)
    return (rng.standard_normal((h, w)) * 300).astype(np.float32)


def footprint_mask(rects, w, h):
    m = np.zeros((h, w), dtype=bool)
    for (x, y, rw, rh) in rects:
        assert x + rw <= w and y + rh <= h, (x, y, rw, rh)
        m[y:y + rh, x:x + rw] = True
    return m


def poison(a, mask, rev, rng, hard):
    """A copy of plane `a` with everything outside `mask` overwritten: large random values, or (hard) the values that spoil
    whatever they touch -- ints near 2^30 and NaN bit patterns."""
    p = a.copy()
    n = int((~mask).sum())
    if rev:
        lo, hi = ((1 << 29), (1 << 30)) if hard else (100000, 1 << 24)
        p[~mask] = (rng.integers(lo, hi, size=n) * rng.choice([-1, 1], size=n)).astype(np.int32)
    elif hard:
        p.view(np.uint32)[~mask] = (0x7fc00000 | rng.integers(0, 1 << 22, size=n)).astype(np.uint32)
    else:
        p[~mask] = (rng.standard_normal(n) * 1e12).astype(np.float32)
    return p
