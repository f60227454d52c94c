"""Case tables and CPU references of the forward-DWT sweep (test_dwt_sweep.py on the GPU, test_dwt_sweep_refs.py anywhere).
Plain helpers: no fixtures, no tests.

Sweep: the (width, height, origin) sweep of the inverse transform (decode_stage_cases.sweep_shapes), packed as regions of one
plane 1024 words wide -- the jobs of one launch per level of Encoder.stage_dwt_regions.
Boundaries: an explicit region list around the strip counts of dwt_level_kernel (124 column pairs per wave with two pairs
per lane, 60 with one) and around its wave-uniform fast-path test, every region at a plane x that is a multiple of 4 and, for
the fast-eligible widths at origin (0,1) and height 16, twice more: at x = 2 and at x = 1 (mod 4).
Inputs: one plane per input class, all planes of a transform in one call.
Restatements: dwt53_int64 and dwt97_float64, written from T.800 F.4.8 without the oracle.
Launch model: region_jobs() makes the hook's job table of a level for dwt_variant_cases.level_launch.
"""
from __future__ import annotations

import numpy as np
import pytest

import dwt_variant_cases as V
from decode_stage_cases import SWEEP_LEVELS, idwt_input, pack_regions, sweep_shapes  # noqa: F401  (SWEEP_LEVELS: for the tests)

PLANE_W = 1024
TOP = 1 << 17  # the top of the 18-bit range an RCT of 16-bit samples has
KNOBS = [dict(dwt_pairs=p, dwt_ppc=c, dwt_xcd=x) for p in (1, 2) for c in (0, 1, 3) for x in (0, 1)]
BOUNDARY_KNOBS = [dict(dwt_pairs=p, dwt_ppc=c) for p in (1, 2) for c in (0, 3)]
BOUNDARY_LEVELS = [1, 2]


# ------------------------------------------------------------------------------------------------ region lists
def sweep_regions():
    """(plane height, [(x, y, w, h, x0, y0)]) of the sweep: 1350 regions, one word between neighbours."""
    return pack_regions(sweep_shapes(), PLANE_W)


# one strip / two strips with two pairs and with one pair per lane; around the fast threshold (rw >= 500, rw % 4 == 0)
BOUNDARY_W = [247, 248, 249, 250, 119, 120, 121, 122, 496, 500, 502, 504, 748, 752]
BOUNDARY_H = [15, 16, 17]
BOUNDARY_ORIGINS = [(0, 0), (0, 1), (1, 0), (2, 1)]
FAST_W = [w for w in BOUNDARY_W if w % 4 == 0 and w >= 500]
# the order that fills shelves of 1024 words
_SHELF_ORDER = [748, 250, 752, 249, 504, 502, 500, 496, 247, 248, 119, 120, 121, 122]


def boundary_regions():
    """(plane height, regions, twins): every (width, height, origin) at a plane x that is a multiple of 4 with at least one
    word between neighbours; then, at origin (0,1) and height 16, every fast-eligible width three times -- twins[w] =
    (index at x = 0, at x = 2, at x = 1 (mod 4))."""
    assert sorted(_SHELF_ORDER) == sorted(BOUNDARY_W)
    regions, twins = [], {}
    x, y, shelf = 0, 1, 0

    def place(w, h, x0, y0, xmod):
        nonlocal x, y, shelf
        x = -(-x // 4) * 4 + xmod
        if x + w + 1 > PLANE_W:
            y, shelf = y + shelf + 1, 0
            x = xmod
        regions.append((x, y, w, h, x0, y0))
        x += w + 1
        shelf = max(shelf, h)
        return len(regions) - 1
    for h in BOUNDARY_H:
        for (x0, y0) in BOUNDARY_ORIGINS:
            for w in _SHELF_ORDER:
                place(w, h, x0, y0, 0)
    for w in FAST_W:
        twins[w] = tuple(place(w, 16, 0, 1, xmod) for xmod in (0, 2, 1))
    return y + shelf + 1, regions, twins


# ------------------------------------------------------------------------------------------------ inputs
PATTERNS = ["constant", "checkerboard", "columns", "rows", "first row and column", "zero"]


def pattern(k, w, h):
    """Structured region k (mod 6) as int64: a flat field, the three alternations at +-2^17, an L of 2^17 on zeros, zeros --
    a black frame, an opaque alpha channel, the inputs whose coefficients are exact zeros."""
    yy, xx = np.mgrid[0:h, 0:w]
    k %= len(PATTERNS)
    if k == 0:
        return np.full((h, w), TOP, np.int64)
    if k == 1:
        return np.where((xx + yy) & 1, -TOP, TOP).astype(np.int64)
    if k == 2:
        return np.where(xx & 1, -TOP, TOP).astype(np.int64)
    if k == 3:
        return np.where(yy & 1, -TOP, TOP).astype(np.int64)
    if k == 4:
        return np.where((xx == 0) | (yy == 0), TOP, 0).astype(np.int64)
    return np.zeros((h, w), np.int64)


def input_planes(rev, height, regions, seed):
    """The planes of one call, one per input class.  5/3: (a) integers of (-2^17, 2^17], (b) structured.  9/7: (a)
    standard_normal x 3000, (b) zeros among values near 2^-120, (c) structured.  The structured plane holds pattern i mod 6
    in region i and random non-zero words between the regions."""
    rng = np.random.default_rng(seed)
    shape = (height, PLANE_W)
    if rev:
        planes = [rng.integers(-TOP + 1, TOP + 1, size=shape).astype(np.int32)]
    else:
        planes = [idwt_input(rng, shape, False), idwt_input(rng, shape, False, tiny=True)]
    s = rng.integers(1, TOP, size=shape).astype(np.int64)
    for i, (x, y, w, h, _, _) in enumerate(regions):
        s[y:y + h, x:x + w] = pattern(i, w, h)
    planes.append(s.astype(np.int32 if rev else np.float32))
    out = np.stack(planes)
    out.setflags(write=False)
    return out


INPUT_CLASSES = {True: ["(a) random", "(b) structured"], False: ["(a) random", "(b) tiny", "(c) structured"]}

_lists = {}


def region_list(which):
    """"sweep" / "boundary" -> (plane height, regions), made once."""
    if which not in _lists:
        _lists[which] = sweep_regions() if which == "sweep" else boundary_regions()[:2]
    return _lists[which]


_inputs = {}


def inputs(which, rev):
    """The input planes of a region list: made once, shared by every level count and knob set, never written."""
    if (which, rev) not in _inputs:
        height, regions = region_list(which)
        _inputs[(which, rev)] = input_planes(rev, height, regions, (5300 if rev else 9700) + (which == "boundary"))
    return _inputs[(which, rev)]


_refs = {}


def reference(oracle, which, rev, levels):
    """Every region of every plane transformed by the oracle on its own; the words between the regions stay.  Cached per
    (region list, transform, levels)."""
    key = (which, rev, levels)
    if key not in _refs:
        _, regions = region_list(which)
        a = inputs(which, rev)
        out = a.copy()
        f = oracle.dwt53 if rev else oracle.dwt97
        for p in range(a.shape[0]):
            for (x, y, w, h, x0, y0) in regions:
                out[p, y:y + h, x:x + w] = f(a[p, y:y + h, x:x + w], levels, x0, y0)
        out.setflags(write=False)
        _refs[key] = out
    return _refs[key]


def release():
    """Drops the cached inputs and references (they are made again on demand)."""
    _inputs.clear()
    _refs.clear()


_labels = {}


def _label_map(which):
    if which not in _labels:
        height, regions = region_list(which)
        m = np.full((height, PLANE_W), -1, np.int32)
        for i, (x, y, w, h, _, _) in enumerate(regions):
            assert (m[y:y + h, x:x + w] == -1).all() and x + w <= PLANE_W, "regions overlap or leave the plane"
            m[y:y + h, x:x + w] = i
        _labels[which] = m
    return _labels[which]


def difference(which, rev, levels, kn, got, ref):
    """None when got equals ref bit for bit over the whole planes (the int32 view: -0.0 is not 0.0), else the message:
    region, origin, levels, knobs, input class, sub-band and the first differing word."""
    g, r = got.view(np.int32), ref.view(np.int32)
    if g.shape == r.shape and np.array_equal(g, r):
        return None
    head = f"{which} {'53' if rev else '97'} L{levels} [{V.kid(kn)}]"
    if g.shape != r.shape:
        return f"{head}: shape {g.shape} against {r.shape}"
    _, regions = region_list(which)
    labels = _label_map(which)
    bad = np.argwhere(g != r)
    p, y, x = (int(v) for v in bad[0])
    nreg = len({(int(b[0]), int(labels[b[1], b[2]])) for b in bad[:100000]})
    words = f"got {got[p, y, x]!r} (0x{int(g[p, y, x]) & 0xffffffff:08x}), reference {ref[p, y, x]!r} (0x{int(r[p, y, x]) & 0xffffffff:08x})"
    head += f": {len(bad)} of {g.size} words differ in {nreg} (plane, region) pairs, first in plane {p} {INPUT_CLASSES[rev][p]} at (y {y}, x {x})"
    i = int(labels[y, x])
    if i < 0:
        return f"{head}, between the regions: a word outside every region was written: {words}"
    rx, ry, w, h, x0, y0 = regions[i]
    case = V.Case("", w, h, 1, rev, False, 0, 0, False, 0, levels, 0, "planes")
    pat = f", pattern {PATTERNS[i % 6]!r}" if p == len(INPUT_CLASSES[rev]) - 1 else ""
    band = V.subband(case, (x0, y0, x0 + w, y0 + h), x - rx, y - ry)
    return (f"{head}, region {i}: {w} x {h} at plane ({rx}, {ry}), origin ({x0}, {y0}){pat}, "
            f"local (y {y - ry}, x {x - rx}), sub-band {band}: {words}")


def check_regions(oracle, enc, which, rev, levels, kn):
    """One call of the region hook under the knobs against the cached reference; fails with difference()'s message."""
    _, regions = region_list(which)
    with V.knobs(kn):
        got = enc.stage_dwt_regions(inputs(which, rev), levels, rev, regions)
    msg = difference(which, rev, levels, kn, got, reference(oracle, which, rev, levels))
    if msg:
        pytest.fail(msg, pytrace=False)


# ------------------------------------------------------------------------------------------------ fused edge tiles
# (channels, colour transform, container bits, precision, Promote) -> the conversion path of dwt_fused_kernel it takes
EDGE_FORMATS = {"c1-8to8": (1, False, 8, 8, False), "c3m-8to8": (3, True, 8, 8, False), "c4-16to16": (4, False, 16, 16, False),
                "c3-16to12p": (3, False, 16, 12, True)}
EDGE_VARIANTS = {"c1-8to8": "generic", "c3m-8to8": "SPEC2", "c4-16to16": "SPEC1", "c3-16to12p": "GEN"}


def edge_tile_frames():
    """(w, h, tile): (t + n) x (t + m) in tiles of t -- edge tiles n x t, t x m and n x m at origin t (even: 16, odd: 17)."""
    return [(t + n, t + m, t) for t in (16, 17) for n in range(1, 14) for m in sorted({n, 14 - n})]


def edge_tile_cases(fmt, rev, levels):
    nc, mct, bits, prec, promote = EDGE_FORMATS[fmt]
    return [V.ae_case(w, h, nc, rev, mct, bits, prec, promote, 0, levels, t) for (w, h, t) in edge_tile_frames()]


# ------------------------------------------------------------------------------------------------ restatements
def _ext(i, n):
    """Whole-sample symmetric extension of the indices i onto [0, n), n >= 2, for |offsets| below n."""
    i = np.abs(i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def _split(x, cas):
    return np.concatenate([x[:, cas::2], x[:, 1 - cas::2]], axis=1)  # low half (even absolute positions) first


def _dwt53_lines(a, cas, peak):
    """a: (lines, n) int64, cas = parity of the absolute coordinate of sample 0 (T.800 F.4.8.1)."""
    n = a.shape[1]
    if n == 1:
        return a * 2 if cas else a.copy()  # a single odd-phase sample is doubled
    x = a.copy()
    idx = np.arange(n)
    p = idx[1 - cas::2]
    s = x[:, _ext(p - 1, n)] + x[:, _ext(p + 1, n)]
    peak[0] = max(peak[0], int(np.abs(s).max(initial=0)))
    x[:, p] -= s >> 1
    p = idx[cas::2]
    s = x[:, _ext(p - 1, n)] + x[:, _ext(p + 1, n)] + 2
    peak[0] = max(peak[0], int(np.abs(s).max(initial=0)))
    x[:, p] += s >> 2
    return _split(x, cas)


_A97, _B97, _G97, _D97, _K97 = -1.586134342, -0.052980118, 0.882911075, 0.443506852, 1.230174105  # dwt.hip: K97_*


def _dwt97_lines(a, cas, peak=None):
    n = a.shape[1]
    if n == 1:
        return a.copy()  # a line of one sample is left as it is
    x = a.copy()
    idx = np.arange(n)
    for first, c in ((1 - cas, _A97), (cas, _B97), (1 - cas, _G97), (cas, _D97)):
        p = idx[first::2]
        x[:, p] = x[:, p] + (x[:, _ext(p - 1, n)] + x[:, _ext(p + 1, n)]) * c
    x[:, cas::2] *= 1.0 / _K97
    x[:, 1 - cas::2] *= _K97
    return _split(x, cas)


def _mallat(plane, levels, x0, y0, dtype, lines, peak):
    a = np.asarray(plane, dtype=dtype).copy()
    h, w = a.shape
    cd = lambda v, l: (v + (1 << l) - 1) >> l
    for lev in range(levels):
        cx0, cx1, cy0, cy1 = cd(x0, lev), cd(x0 + w, lev), cd(y0, lev), cd(y0 + h, lev)
        rw, rh = cx1 - cx0, cy1 - cy0
        if rw <= 0 or rh <= 0:
            break
        a[:rh, :rw] = lines(a[:rh, :rw].T.copy(), cy0 & 1, peak).T  # vertical first
        a[:rh, :rw] = lines(a[:rh, :rw], cx0 & 1, peak)             # then horizontal
        peak[0] = max(peak[0], abs(a).max())
    return a


def dwt53_int64(plane, levels, x0, y0, peak=None):
    """The reversible transform in int64.  peak (a one-element list) receives the largest magnitude met at any level,
    the sums inside the lifting steps included."""
    return _mallat(plane, levels, x0, y0, np.int64, _dwt53_lines, peak if peak is not None else [0])


def dwt97_float64(plane, levels, x0, y0):
    """The irreversible transform in float64 with the constants of dwt.hip: low band x 1 / K, high band x K."""
    return _mallat(plane, levels, x0, y0, np.float64, _dwt97_lines, [0])


# ------------------------------------------------------------------------------------------------ launch model
def region_jobs(regions, level, plane_w, plane_h, nplanes):
    """j2k_hip_stage_dwt_regions' job table of `level` (0 = full resolution): one job per (plane, region) in that order,
    regions of which nothing is left skipped, every offset = c * plane + y * width + x."""
    jobs = []
    for c in range(nplanes):
        for (x, y, w, h, x0, y0) in regions:
            ax0, ax1, ay0, ay1 = V._cd(x0, level), V._cd(x0 + w, level), V._cd(y0, level), V._cd(y0 + h, level)
            if ax1 - ax0 <= 0 or ay1 - ay0 <= 0:
                continue
            off = c * plane_w * plane_h + y * plane_w + x
            jobs.append(V.Job(ax1 - ax0, ay1 - ay0, ax0 & 1, ay0 & 1, off, off, off, 0))
    return jobs


def region_launch(which, rev, level, kn):
    """The launch model of one level of check_regions(which, rev, ...) -> (jobs, model)."""
    height, regions = region_list(which)
    jobs = region_jobs(regions, level, PLANE_W, height, len(INPUT_CLASSES[rev]))
    return jobs, V.level_launch(jobs, kn, PLANE_W)
