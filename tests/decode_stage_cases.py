"""Inputs and expectations of the decode-stage tests (test_decode_stages.py on the GPU, test_decode_stage_refs.py on the
CPU).  Plain helpers: no fixtures, no tests.

Tier-1: a case is a dict -- w, h, orient, numbps, npasses, data (codeword bytes), half_step, roishift -- made from a block of
coefficients by the oracle's encoder; what a decoder must leave in the plane for it comes from the oracle's block decoder
exactly as the oracle's tile decoder uses it (oracle/j2k_oracle_dec.c, the loop over code-blocks of j2ko_decode).
Inverse DWT: the (width, height, origin, levels) sweep, packed as regions of one plane per level count.
"""
import numpy as np

STEP = 0.37          # band step size of the irreversible cases (as in the encode-side Tier-1 tests)
CELL, NCOL = 64, 16  # one 64 x 64 cell per block, 16 cells per row of the plane


# ------------------------------------------------------------------------------------------------ Tier-1
def code_block(oracle, coef, orient, rev, roishift=0):
    """coef: (h, w) integer coefficients -> a case with every pass.  Reversible: the samples with 6 fractional bits;
    irreversible: 0.61 x coef quantised with STEP, like the encode-side tests feed the GPU encoder."""
    coef = np.asarray(coef, dtype=np.int64)
    if rev:
        data = (coef << 6).astype(np.int32)
    else:
        blk = (coef * 0.61).astype(np.float32)
        data = np.array([[oracle.L.j2ko_quant97(float(v), STEP) for v in row] for row in blk], dtype=np.int32)
    return code_scaled(oracle, data, orient, roishift)


def code_scaled(oracle, data, orient, roishift=0):
    """data: (h, w) int32 as the block coder takes it."""
    ref = oracle.t1_block(np.asarray(data, dtype=np.int32), orient)
    h, w = data.shape
    return dict(w=w, h=h, orient=orient, numbps=ref["numbps"], npasses=ref["npasses"], data=ref["data"], rates=ref["rates"],
                half_step=float(np.float32(0.5) * np.float32(STEP)), roishift=roishift)


def variant(case, **kw):
    c = dict(case)
    c.update(kw)
    return c


def kernel_passes(numbps, npasses):
    """The count a decoder works with: a block of numbps bit-planes has 3 numbps - 2 coding passes (T.800 D.3: the first
    plane has a cleanup pass only); none without a bit-plane."""
    return min(npasses, 3 * numbps - 2) if numbps else 0


def roi_unshift(v, shift):
    """T.800 H.1 (MAXSHIFT), on the decoder's values: a magnitude at or above 2^shift belongs to the region of interest
    and comes down by `shift` bits; every other sample stays as it is."""
    v = np.asarray(v, dtype=np.int64)
    if not shift:
        return v
    m = np.abs(v)
    return np.where(m >= (1 << shift), np.sign(v) * (m >> shift), v)


def expected_words(oracle, case, rev):
    """The block's rectangle as int32 words, or None for a block that holds nothing (its rectangle stays as it was)."""
    np_ = kernel_passes(case["numbps"], case["npasses"])
    if np_ == 0:
        return None
    v = oracle.t1_decode_block(case["data"], case["w"], case["h"], case["orient"], case["numbps"], np_)
    v = roi_unshift(v, case["roishift"])
    if rev:
        return (np.sign(v) * (np.abs(v) // 2)).astype(np.int32)  # v / 2 in C: truncation toward zero
    return (v.astype(np.float32) * np.float32(case["half_step"])).view(np.int32)


def fill_pattern(shape):
    """What the plane holds before the decode: words no decode produces by accident, none of them zero."""
    n = shape[0] * shape[1]
    return (((np.arange(n, dtype=np.uint64) * 2654435761) & 0x3fffffff) | 0x40000001).astype(np.int32).reshape(shape)


def lay_out(cases):
    """A rectangle per case: cell i of a plane of NCOL cells per row, every block pushed off the cell's corner where it is
    smaller than the cell (so that block origins are not all multiples of 64)."""
    nrow = (len(cases) + NCOL - 1) // NCOL
    rects = []
    for i, c in enumerate(cases):
        dx, dy = min(i % 3, CELL - c["w"]), min(i % 2, CELL - c["h"])
        rects.append((CELL * (i % NCOL) + dx, CELL * (i // NCOL) + dy, c["w"], c["h"]))
    return (CELL * nrow, CELL * NCOL), rects


def decode_and_expect(enc, oracle, cases, rev, kernel):
    """Runs the cases through the stage hook; returns (got, want, rects) as int32 planes."""
    shape, rects = lay_out(cases)
    fill = fill_pattern(shape)
    want = fill.copy()
    blocks = []
    for c, (x, y, w, h) in zip(cases, rects):
        e = expected_words(oracle, c, rev)
        if e is not None:
            want[y:y + h, x:x + w] = e
        blocks.append(dict(rect=(x, y, w, h), orient=c["orient"], numbps=c["numbps"], npasses=c["npasses"], data=c["data"],
                           half_step=c["half_step"], roishift=c["roishift"]))
    plane = fill if rev else fill.view(np.float32)
    got = enc.stage_t1_decode(plane, blocks, rev, kernel)
    return got.view(np.int32), want, rects


def assert_planes_equal(got, want, rects, cases):
    if np.array_equal(got, want):
        return
    for i, (x, y, w, h) in enumerate(rects):
        g, e = got[y:y + h, x:x + w], want[y:y + h, x:x + w]
        if not np.array_equal(g, e):
            c = cases[i]
            bad = np.argwhere(g != e)
            raise AssertionError(f"block {i} ({w} x {h}, orient {c['orient']}, numbps {c['numbps']}, npasses {c['npasses']}, "
                                 f"{len(c['data'])} bytes, roishift {c['roishift']}): {len(bad)} samples differ, first at "
                                 f"(y, x) = {tuple(bad[0])}: got {g[tuple(bad[0])]:#x}, want {e[tuple(bad[0])]:#x}")
    raise AssertionError(f"{int((got != want).sum())} words outside every block's rectangle were written")


def subset_blocks(rng):
    """The blocks the truncation cases are made of: 64 x 64 dense, 64 x 64 sparse, 1 wide, 1 high, partial last stripe."""
    from t1_families import random_block
    return [("dense", random_block(rng, 64, 64, 0), 0), ("sparse", random_block(rng, 64, 64, 1), 1),
            ("1-wide", random_block(rng, 1, 64, 0), 2), ("1-high", random_block(rng, 64, 1, 3), 3),
            ("partial-stripe", random_block(rng, 37, 13, 0), 1)]


def long_stream_block(rng):
    """64 x 64 coefficients of uniform random 16-bit magnitudes, as the block coder takes them (6 fractional bits):
    16 bit-planes, 46 passes, about 9 KB of codeword."""
    return ((rng.integers(0, 1 << 16, size=(64, 64)) * np.where(rng.random((64, 64)) < 0.5, -1, 1)) << 6).astype(np.int32)


def top_planes_block(rng):
    """A small block whose input to the block coder reaches 2^30: 25 bit-planes, 73 passes."""
    b = rng.integers(-(1 << 30), 1 << 30, size=(7, 5)).astype(np.int64)
    b[0, 0], b[3, 2], b[6, 4] = 1 << 30, -(1 << 30), (1 << 30) - 1
    return b.astype(np.int32)


# ------------------------------------------------------------------------------------------------ inverse DWT
SWEEP_W = list(range(1, 14)) + [16, 17, 31, 64, 65]
SWEEP_H = list(range(1, 14)) + [24, 65]
SWEEP_ORIGINS = [(0, 0), (1, 0), (0, 1), (1, 1), (3, 2)]
SWEEP_LEVELS = [1, 2, 3, 5]
# the DWT list of test_gpu_parity.py (w, h, levels, x0, y0), plus two shapes for the grid strides
IDWT_SHAPES = [(64, 64, 1, 0, 0), (300, 200, 5, 0, 0), (301, 199, 3, 0, 0), (128, 128, 5, 128, 128), (97, 61, 4, 33, 7),
               (1, 40, 2, 0, 0), (40, 1, 2, 1, 1), (2, 2, 1, 1, 0), (3, 5, 2, 0, 1), (1000, 37, 5, 0, 0), (513, 515, 6, 0, 0),
               (4097, 33, 5, 0, 0), (33, 4097, 5, 0, 0)]


def sweep_shapes():
    return [(w, h, x0, y0) for w in SWEEP_W for h in SWEEP_H for (x0, y0) in SWEEP_ORIGINS]


def pack_regions(shapes, plane_w=1024, gap=1):
    """Shelf packing of (w, h, x0, y0) into one plane, `gap` words between neighbours and along the plane's edges:
    -> (plane height, [(x, y, w, h, x0, y0)])."""
    regions, x, y, shelf = [], gap, gap, 0
    for (w, h, x0, y0) in shapes:
        if x + w + gap > plane_w:
            x, y, shelf = gap, y + shelf + gap, 0
        regions.append((x, y, w, h, x0, y0))
        x += w + gap
        shelf = max(shelf, h)
    return y + shelf + gap, regions


def idwt_input(rng, shape, rev, tiny=False):
    """5/3: integers within +-2^24.  9/7: standard_normal x 3000, or (tiny) exact zeros among values near 2^-120, whose
    lifting products are denormal."""
    if rev:
        return rng.integers(-(1 << 24), (1 << 24) + 1, size=shape).astype(np.int32)
    if tiny:
        v = (rng.standard_normal(shape) * 2.0 ** -120).astype(np.float32)
        return np.where(rng.random(shape) < 0.25, np.float32(0), v).astype(np.float32)
    return (rng.standard_normal(shape) * 3000).astype(np.float32)


def idwt_regions_reference(oracle, plane, regions, levels, rev):
    """Every region synthesised by the oracle on its own; the words between the regions stay."""
    out = plane.copy()
    f = oracle.idwt53 if rev else oracle.idwt97
    for (x, y, w, h, x0, y0) in regions:
        out[y:y + h, x:x + w] = f(plane[y:y + h, x:x + w], levels, x0, y0)
    return out


# float64 restatement of the 9/7 synthesis (T.800 F.3.8: 1D_FILTR over the symmetric extension of F.3.7) with
# libopenjp2's gains: low band x K, high band x 13318 / 8192 (its historic constant for 2 / K)
_K, _TWO_INVK = 1.230174105, 13318.0 / 8192.0
_ALPHA, _BETA, _GAMMA, _DELTA = -1.586134342, -0.052980118, 0.882911075, 0.443506852


def _synth97_lines(a, cas):
    """a: (lines, n) float64, each line low-pass samples first; cas = parity of the line's first absolute coordinate."""
    n = a.shape[1]
    if n == 1:
        return a.copy()  # the library leaves a line of one sample as it is (no gain): lines of n == 1 are not checked
    sn = (n + 1 - cas) // 2
    x = np.empty_like(a)
    x[:, cas::2] = a[:, :sn] * _K
    x[:, 1 - cas::2] = a[:, sn:] * _TWO_INVK
    idx = np.arange(n)

    def ext(i):
        i = np.abs(i)
        return np.where(i >= n, 2 * (n - 1) - i, i)
    for first, c in ((cas, -_DELTA), (1 - cas, -_GAMMA), (cas, -_BETA), (1 - cas, -_ALPHA)):
        p = idx[first::2]
        x[:, p] = x[:, p] + (x[:, ext(p - 1)] + x[:, ext(p + 1)]) * c
    return x


def idwt97_float64(plane, levels, x0, y0):
    a = np.asarray(plane, dtype=np.float64).copy()
    h, w = a.shape
    cdp2 = lambda v, l: (v + (1 << l) - 1) >> l
    for lev in range(levels - 1, -1, -1):
        cx0, cx1, cy0, cy1 = cdp2(x0, lev), cdp2(x0 + w, lev), cdp2(y0, lev), cdp2(y0 + h, lev)
        rw, rh = cx1 - cx0, cy1 - cy0
        if rw <= 0 or rh <= 0:
            continue
        a[:rh, :rw] = _synth97_lines(a[:rh, :rw], cx0 & 1)              # horizontal first
        a[:rh, :rw] = _synth97_lines(a[:rh, :rw].T.copy(), cy0 & 1).T   # then vertical
    return a
