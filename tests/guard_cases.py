"""Frames whose coefficients reach or outgrow the bit-planes their sub-bands signal: one case module for the CPU tier
(test_guard_bits_refs.py) and the GPU tier (test_guard_bits.py).  numpy and the plain-C oracle alone: no device, no library.

A sub-band signals Mb = exponent + guard bits - 1 bit-planes (two guard bits).  A lossless frame under the reversible colour
transform whose G plane is 0 or `amp` in a k x k checker (or a seeded random mask of k x k cells) and whose R = B = amp - G has
chroma planes that swing over +-amp: twice the range the exponent allows for.  The LL band of a shallow decomposition then gains
more than the one spare bit it has and a code-block holds Mb + 1 bit-planes (`over`).  The zero-bit-plane count of the packet
header would be negative: libopenjp2 writes such a file all the same and it does not decode to the frame; this encoder refuses
it (J2K_HIP_ERR_OVERFLOW).  A smaller amplitude puts the block exactly at Mb (`at_limit`: zero-bit-plane count 0), the other side
of the edge.

  frame(case)          the samples, (nc, h, w) int32
  classify(oracle, c)  every code-block of the frame in the encoder's table order (tile, resolution, component, band, raster), with
                       its Mb, its numbps by the oracle's Tier-1 and its class: `below`, `at_limit` (numbps == Mb) or `over`
  CASES                the named frames; `expect` is what the classifier must say of the whole frame (test_guard_bits_refs.py)
  search_97()          the 9/7 search over SEARCH_97_FAMILY
"""
from collections import namedtuple

import ctypes as C

import numpy as np

Case = namedtuple("Case", "name prec k numres w h tile nc amp mask seed rev rates jp2 expect pattern_tiles max_err")

SEED = 20261020


def _case(name, prec, k, numres, expect, w=64, h=64, tile=0, nc=3, amp=None, mask="checker", seed=0, rev=True, rates=None, jp2=False,
          pattern_tiles=None, max_err=None):
    return Case(name, prec, k, numres, w, h, tile, nc, (1 << prec) - 1 if amp is None else amp, mask, seed, rev,
                tuple(rates) if rates else None, jp2, expect, pattern_tiles, max_err)


# max_err: the largest sample error of libopenjp2's (= the oracle's) own file of an `over` frame after its own decode, as
# round_trip_error measures it; test_guard_bits_refs.py holds the table to the measurement.  It is the evidence that refusing
# such a frame is right, not a tolerance of anything.
# amp of the at_limit frames: the largest amplitude at which classify() finds no `over` block (find_amp; held to it there too).
# pattern_tiles: the tiles that carry the pattern; the others hold benign_frame's samples.
CASES = [
    _case("over_8_k2_r2", 8, 2, 2, "over", max_err=144),
    _case("over_8_k4_r3", 8, 4, 3, "over", max_err=156),
    _case("over_16_k2_r2", 16, 2, 2, "over", max_err=36864),
    _case("over_16_k4_r3", 16, 4, 3, "over", max_err=40000),
    _case("over_12_k2_r2", 12, 2, 2, "over", w=32, h=32, max_err=2304),
    _case("over_10_rand_r2", 10, 2, 2, "over", mask="random", seed=3, w=32, h=32, max_err=576),
    _case("limit_8_k2_r3", 8, 2, 3, "at_limit"),
    _case("limit_8_k2_r2", 8, 2, 2, "at_limit", amp=226),
    _case("limit_16_k2_r2", 16, 2, 2, "at_limit", amp=58253),
    _case("limit_12_k4_r3", 12, 4, 3, "at_limit", amp=3354),
    _case("limit_10_rand_r2", 10, 2, 2, "at_limit", mask="random", seed=3, w=32, h=32, amp=910),
    _case("over_tiles_8_k2_r2", 8, 2, 2, "over", w=128, h=64, tile=64, pattern_tiles=(1,), max_err=144),
    _case("limit_tiles_8_k2_r2", 8, 2, 2, "at_limit", w=128, h=64, tile=64, pattern_tiles=(1,), amp=226),
    # (no 9/7 frame of search_97's family goes over: the rate-controlled case is a reversible frame with a byte budget)
    _case("over_rates_8_k2_r2", 8, 2, 2, "over", rates=[20.0]),
    _case("over_rgba_8_k2_r2", 8, 2, 2, "over", nc=4, max_err=144),
    _case("over_jp2_8_k2_r2", 8, 2, 2, "over", jp2=True, max_err=144),
    # six resolutions, what HipCodec::WriteFile always writes: the one `over` frame among the 33 x 33 and smaller ones of the family
    _case("over_8_rand7_r6", 8, 7, 6, "over", mask="random", seed=2, w=33, h=33, max_err=129),
]
OVER = [c for c in CASES if c.expect == "over"]
AT_LIMIT = [c for c in CASES if c.expect == "at_limit"]
BY_NAME = {c.name: c for c in CASES}


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------- frames
def mask_of(c: Case) -> np.ndarray:
    """(h, w) of 0 / 1: the k x k checker, or k x k cells of a seeded random mask."""
    y, x = np.arange(c.h)[:, None] // c.k, np.arange(c.w)[None, :] // c.k
    if c.mask == "checker":
        return ((x + y) & 1).astype(np.int32)
    cells = np.random.default_rng(SEED + c.seed).integers(0, 2, (cdiv(c.h, c.k), cdiv(c.w, c.k)))
    return cells[y, x].astype(np.int32)


def frame(c: Case, amp=None) -> np.ndarray:
    """(nc, h, w) int32: G = amp on the mask and 0 elsewhere, R = B = amp - G, a fourth channel = G.  The tiles outside
    c.pattern_tiles (where that is given) hold benign_frame's samples."""
    amp = c.amp if amp is None else amp
    g = mask_of(c) * amp
    pl = np.stack([amp - g, g, amp - g, g][:c.nc]).astype(np.int32)
    if c.pattern_tiles is not None:
        ben = benign_frame(c)
        ntx = cdiv(c.w, c.tile)
        for t in range(ntx * cdiv(c.h, c.tile)):
            if t not in c.pattern_tiles:
                x0, y0 = (t % ntx) * c.tile, (t // ntx) * c.tile
                pl[:, y0:y0 + c.tile, x0:x0 + c.tile] = ben[:, y0:y0 + c.tile, x0:x0 + c.tile]
    return np.ascontiguousarray(pl)


def benign_frame(c: Case) -> np.ndarray:
    """A frame of the case's geometry whose blocks all stay below Mb (asserted in test_guard_bits_refs.py)."""
    from j2k_amd import synth
    return synth.planes(c.w, c.h, c.nc, c.prec, 4242 + c.prec)


def oracle_params(c: Case):
    from oracle.oracle import make_params
    return make_params(c.w, c.h, c.nc, c.prec, reversible=c.rev, mct=True, numres=c.numres, tile=c.tile, layers=len(c.rates) if c.rates else 1)


def api_params(api, c: Case):
    # (color_space 1 = sRGB, the fourth channel an alpha channel: what the oracle's JP2 wrapper is given below)
    return api.make_params(c.w, c.h, c.nc, c.prec, reversible=c.rev, ycc=True, num_resolutions=c.numres, tile_size=c.tile, comment="",
                           rates=list(c.rates) if c.rates else None, jp2=c.jp2, color_space=1 if c.jp2 else 0,
                           alpha_channel=3 if (c.jp2 and c.nc == 4) else -1)


_files = {}


def oracle_file(oracle, c: Case, planes=None, key=None) -> bytes:
    """The oracle's file of the case's frame (or of `planes`, memoised under `key`): what libopenjp2 writes, byte for byte."""
    k = (c.name, key)
    if planes is not None and key is None:
        k = None
    if k in _files:
        return _files[k]
    pl = frame(c) if planes is None else planes
    p = oracle_params(c)
    prefix = len(oracle.jp2_wrap(b"", p, color_space=1, alpha_channel=3 if c.nc == 4 else -1)) if c.jp2 else 0
    cs = oracle.encode_rates(pl, p, list(c.rates), prefix_len=prefix) if c.rates else oracle.encode(pl, p)
    if c.jp2:
        cs = oracle.jp2_wrap(cs, p, color_space=1, alpha_channel=3 if c.nc == 4 else -1)
    if k is not None:
        _files[k] = cs
    return cs


# ---------------------------------------------------------------------------------------------------------------------- classifier
def block_table(w, h, nc, numres, tile, cb=64):
    """The code-blocks of a frame with maximal precincts, in the encoder's table order: dicts(tile, comp, res, band, orient,
    x, y, w, h -- x, y in the component's Mallat plane --, bandidx, and tx, ty = the block's corner inside the tile's plane)."""
    NL = numres - 1
    tw, th = (tile, tile) if tile else (w, h)
    ntx, nty = cdiv(w, tw), cdiv(h, th)
    out = []
    for t in range(ntx * nty):
        tx0, ty0 = (t % ntx) * tw, (t // ntx) * th
        tx1, ty1 = min(tx0 + tw, w), min(ty0 + th, h)
        for r in range(numres):
            lev = NL - r
            for c in range(nc):
                if r == 0:
                    bands = [(0, 0, cdiv(tx0, 1 << lev), cdiv(ty0, 1 << lev), cdiv(tx1, 1 << lev), cdiv(ty1, 1 << lev), 0, 0)]
                else:
                    nb = lev + 1
                    lw, lh = cdiv(tx1, 1 << nb) - cdiv(tx0, 1 << nb), cdiv(ty1, 1 << nb) - cdiv(ty0, 1 << nb)
                    bands = []
                    for o in (1, 2, 3):
                        xo, yo = (o & 1) << (nb - 1), (o >> 1) << (nb - 1)
                        bands.append((o - 1, o, cdiv(tx0 - xo, 1 << nb), cdiv(ty0 - yo, 1 << nb), cdiv(tx1 - xo, 1 << nb), cdiv(ty1 - yo, 1 << nb),
                                      lw if o & 1 else 0, lh if o & 2 else 0))
                for band, o, bx0, by0, bx1, by1, offx, offy in bands:
                    for gy in range(by0 // cb, cdiv(by1, cb)):
                        for gx in range(bx0 // cb, cdiv(bx1, cb)):
                            x0, y0 = max(bx0, gx * cb), max(by0, gy * cb)
                            x1, y1 = min(bx1, (gx + 1) * cb), min(by1, (gy + 1) * cb)
                            if x1 <= x0 or y1 <= y0:
                                continue
                            px, py = offx + x0 - bx0, offy + y0 - by0
                            out.append(dict(tile=t, comp=c, res=r, band=band, orient=o, x=tx0 + px, y=ty0 + py, w=x1 - x0, h=y1 - y0,
                                            bandidx=0 if r == 0 else 3 * (r - 1) + o, tx=px, ty=py))
    return out


def _transformed(oracle, planes, prec, rev, numres, tile):
    """Per tile the tile-components after level shift, colour transform and DWT (the oracle's own functions): [(nc, th, tw)]."""
    L = oracle.L
    L.j2ko_dc_mct.restype = None
    L.j2ko_dc_mct.argtypes = [C.POINTER(C.POINTER(C.c_int32)), C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int]
    nc, h, w = planes.shape
    tw, th = (tile, tile) if tile else (w, h)
    ntx, nty = cdiv(w, tw), cdiv(h, th)
    out = []
    for t in range(ntx * nty):
        x0, y0 = (t % ntx) * tw, (t // ntx) * th
        comps = [np.array(planes[c, y0:y0 + th, x0:x0 + tw], dtype=np.int32, order="C", copy=True) for c in range(nc)]  # (transformed in place)
        ptrs = (C.POINTER(C.c_int32) * 4)(*[a.ctypes.data_as(C.POINTER(C.c_int32)) for a in comps])
        L.j2ko_dc_mct(ptrs, nc, comps[0].size, prec, int(rev), int(nc >= 3))
        if rev:
            out.append(np.stack([oracle.dwt53(a, numres - 1, x0, y0) for a in comps]))
        else:
            out.append(np.stack([oracle.dwt97(a.view(np.float32), numres - 1, x0, y0) for a in comps]))
    return out


def scaled_block(coefs: np.ndarray, rev: bool, step: float) -> np.ndarray:
    """The block as Tier-1 takes it (6 fractional bits): 5/3 coefficients shifted, 9/7 coefficients by j2ko_quant97's arithmetic
    (float32 quotient, float32 product with 64, round to nearest even)."""
    if rev:
        return (coefs.astype(np.int64) << 6).astype(np.int32)
    q = (coefs.astype(np.float32) / np.float32(step)).astype(np.float32) * np.float32(64)
    return np.rint(q.astype(np.float32)).astype(np.int32)


def numbps_of(scaled: np.ndarray) -> int:
    return max(int(np.abs(scaled.astype(np.int64)).max()).bit_length() - 6, 0)


def classify_planes(oracle, planes, prec, rev, numres, tile, tier1=True, want_symbols=False):
    """block_table rows with Mb, numbps, maxabs (the largest coefficient magnitude in quantiser steps), cls, and with tier1 the
    oracle's Tier-1 result of the block under "t1" (numbps from there)."""
    nc, h, w = planes.shape
    tiles = _transformed(oracle, planes, prec, rev, numres, tile)
    rows = block_table(w, h, nc, numres, tile)
    for b in rows:
        _, _, Mb, step = oracle.band_quant(prec, rev, numres, b["bandidx"])
        co = tiles[b["tile"]][b["comp"], b["ty"]:b["ty"] + b["h"], b["tx"]:b["tx"] + b["w"]]
        sc = scaled_block(co, rev, step)
        b["Mb"], b["maxabs"] = Mb, int(np.abs(sc.astype(np.int64)).max()) >> 6
        b["numbps"] = numbps_of(sc)
        if tier1:
            b["t1"] = oracle.t1_block(sc, b["orient"], want_symbols=want_symbols)
            assert b["t1"]["numbps"] == b["numbps"]
        b["cls"] = "below" if b["numbps"] < Mb else ("at_limit" if b["numbps"] == Mb else "over")
    return rows


_classified = {}


def classify(oracle, c: Case, want_symbols=False):
    key = (c.name, want_symbols)
    if key not in _classified:
        _classified[key] = classify_planes(oracle, frame(c), c.prec, c.rev, c.numres, c.tile, want_symbols=want_symbols)
    return _classified[key]


def verdict(rows) -> str:
    """A frame's class: `over` with one such block, else `at_limit` with one such block, else `below`."""
    cls = {b["cls"] for b in rows}
    return "over" if "over" in cls else ("at_limit" if "at_limit" in cls else "below")


def find_amp(oracle, c: Case) -> int:
    """The largest amplitude at which the case's frame has no `over` block (bisection: a block's largest coefficient grows with
    the amplitude).  How the at_limit amplitudes of CASES were found; test_guard_bits_refs.py holds them to it."""
    lo, hi = 0, (1 << c.prec) - 1  # lo: never over
    if verdict(classify_planes(oracle, frame(c, hi), c.prec, c.rev, c.numres, c.tile, tier1=False)) != "over":
        return hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if verdict(classify_planes(oracle, frame(c, mid), c.prec, c.rev, c.numres, c.tile, tier1=False)) == "over":
            hi = mid
        else:
            lo = mid
    return lo


def round_trip_error(oracle, c: Case) -> int:
    """Largest sample error of the oracle's decode of the oracle's own file of the frame."""
    return int(np.abs(oracle.decode(oracle_file(oracle, c)).astype(np.int64) - frame(c)).max())


# ---------------------------------------------------------------------------------------------------------------------- 9/7 search
# The family: 64 x 64 RGB frames under the irreversible colour transform, every channel 0 or full scale; the mask is a k x k
# checker for k = 1 .. 8 or one of four seeded random masks of 1 x 1, 2 x 2, 3 x 3 and 4 x 4 cells; the colourings are the
# reversible family's (G against R = B), B against R = G (the widest Cb), R against G = B (the widest Cr) and R = G = B (the
# widest luma); prec in {8, 12, 16}; 1 to 5 decomposition levels.  720 frames.
SEARCH_97_FAMILY = dict(size=64, precs=(8, 12, 16), levels=(1, 2, 3, 4, 5), checkers=tuple(range(1, 9)), random_cells=(1, 2, 3, 4),
                        colourings=("g_vs_rb", "b_vs_rg", "r_vs_gb", "grey"))


def search_97(oracle):
    """(frames tried, [(prec, levels, mask, colouring, band index, numbps, Mb)] of the frames with an `over` block,
    the smallest Mb - numbps met)."""
    f = SEARCH_97_FAMILY
    n = f["size"]
    masks = [(f"checker{k}", mask_of(_case("s", 8, k, 2, None, w=n, h=n))) for k in f["checkers"]] + \
            [(f"random{k}", mask_of(_case("s", 8, k, 2, None, w=n, h=n, mask="random", seed=100 + k))) for k in f["random_cells"]]
    tried, found, margin = 0, [], 99
    for prec in f["precs"]:
        full = (1 << prec) - 1
        for mname, m in masks:
            on, off = m * full, full - m * full
            for col in f["colourings"]:
                pl = np.stack({"g_vs_rb": (off, on, off), "b_vs_rg": (off, off, on), "r_vs_gb": (on, off, off), "grey": (on, on, on)}[col]).astype(np.int32)
                for lv in f["levels"]:
                    tried += 1
                    for b in classify_planes(oracle, pl, prec, False, lv + 1, 0, tier1=False):
                        margin = min(margin, b["Mb"] - b["numbps"])
                        if b["cls"] == "over":
                            found.append((prec, lv, mname, col, b["bandidx"], b["numbps"], b["Mb"]))
    return tried, found, margin
