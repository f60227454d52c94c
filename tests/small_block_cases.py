"""Whole-pipeline cases with small code-blocks and precincts, shared by test_small_block_refs.py (CPU) and test_small_blocks.py
(GPU).  Helpers only: a table of named cases -- frame geometry, depth, wavelet, MCT, resolutions, progression, tile size,
code-block size, precincts, style, rates -- and what turns a case into a frame (synth.planes), the oracle's Params
(oracle.make_params) and the arguments of api.make_params.

The reference of every case is the oracle's encoder (byte-identical to libopenjp2 2.4.0 wherever that library encodes the
case at all) and, for the samples, libopenjp2's decoder of the oracle's bytes: libopenjp2's encoder refuses most precincts
below 8 samples and fails on styled 4 x 4 blocks, so it is compared only where safe_for_opj_encoder() allows.

A precinct spec halves below its last size; every resolution above the lowest must keep 2 samples or more (the encoder and
both readers refuse anything smaller), which bounds the resolutions of the small specs."""
import json
import os
from collections import namedtuple

from j2k_amd import synth

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

Case = namedtuple("Case", "name kind w h nc prec rev numres prog tile cblk precincts style rates seed")

SIDES = (4, 8, 16, 32, 64)
# the two small frames: odd sides that are no multiple of 4, partial blocks on both edges at every resolution
RGB8 = dict(w=67, h=45, nc=3, prec=8, rev=True, numres=3)
GREY12 = dict(w=53, h=39, nc=1, prec=12, rev=False, numres=4)
GREY16 = dict(w=53, h=39, nc=1, prec=16, rev=False, numres=4)
TILED = dict(w=90, h=61, tile=40)

PRECINCT_SPECS = {  # name -> (sizes, highest resolution first; the most resolutions that keep 2 above the lowest)
    "p8": ([(8, 8)], 4),
    "p4": ([(4, 4)], 3),
    "p2": ([(2, 2)], 2),
    "p4x16": ([(4, 16)], 3),
    "p16x4": ([(16, 4)], 3),
    "p64_8_2": ([(64, 64), (8, 8), (2, 2)], 4),
}
PRECINCT_CBLKS = ((64, 64), (4, 4), (8, 16))
STYLES = (1, 4, 5, 16, 32, 55)
STYLE_CBLKS = ((4, 4), (8, 4), (4, 32), (64, 8))
RATE_CBLKS = ((4, 4), (8, 8), (4, 64), (64, 4), (16, 4))
RATE_SETS = ([20.0], [30.0, 8.0], [25.0, 10.0, 0.0])
MANY_RATES = [12.0, 4.0, 0.0]


def _case(name, kind, w, h, nc, prec, rev, numres, cblk, seed, prog=0, tile=0, precincts=None, style=0, rates=None):
    return Case(name, kind, w, h, nc, prec, rev, numres, prog, tile, tuple(cblk), tuple(precincts) if precincts else None, style,
                tuple(rates) if rates else None, seed)


def _table():
    out, seed = [], 7000
    # every pair of sides on both frames; the progressions spread over all five (no precincts: all legal for the oracle)
    for i, cw in enumerate(SIDES):
        for j, ch in enumerate(SIDES):
            for k, fr in enumerate((RGB8, GREY16 if (i + j) & 1 else GREY12)):
                seed += 1
                tag = "rgb8_53" if k == 0 else f"grey{fr['prec']}_97"
                out.append(_case(f"size_{cw}x{ch}_{tag}", "size", cblk=(cw, ch), seed=seed, prog=(i * 5 + j + 2 * k) % 5, **fr))
    # precincts down to 2 x 2 (1 x 1 code-blocks), live against the oracle: progressions 0..2
    n = 0
    for pname, (spec, maxres) in PRECINCT_SPECS.items():
        for cb in PRECINCT_CBLKS:
            # ... and once per (spec, code-block) in tiles of 40 on 90 x 61, colour and grey in turn
            tiled = (dict(GREY12, **TILED), "grey12_97_tile40") if n & 1 else (dict(RGB8, **TILED), "rgb8_53_tile40")
            for fr, tag in ((RGB8, "rgb8_53"), (GREY12, "grey12_97"), tiled):
                seed += 1
                n += 1
                f = dict(fr, numres=min(fr["numres"], maxres))
                out.append(_case(f"prec_{pname}_{cb[0]}x{cb[1]}_{tag}", "precinct", cblk=cb, seed=seed, prog=n % 3, precincts=spec, **f))
    # code-block styles on small blocks, one reversible and one irreversible frame; no rates (refused together)
    for s in STYLES:
        for cb in STYLE_CBLKS:
            for k, (fr, tag) in enumerate(((RGB8, "rgb8_53"), (GREY12, "grey12_97"))):
                seed += 1
                out.append(_case(f"style{s}_{cb[0]}x{cb[1]}_{tag}", "style", cblk=cb, seed=seed, style=s, prog=(s + k) % 5, **fr))
    # byte budgets: 1, 2 and 3 layers, the last rate 0 in the three-layer set
    for i, cb in enumerate(RATE_CBLKS):
        for k, fr in enumerate((dict(w=150, h=100, nc=3, prec=8, rev=bool(i & 1), numres=4), dict(w=97, h=131, nc=1, prec=12, rev=not (i & 1), numres=5))):
            seed += 1
            rates = RATE_SETS[(i + k) % 3]
            tag = ("rgb8" if k == 0 else "grey12") + ("_53" if fr["rev"] else "_97")
            out.append(_case(f"rates{len(rates)}_{cb[0]}x{cb[1]}_{tag}", "rates", cblk=cb, seed=seed, rates=rates, prog=(i + 3 * k) % 5, **fr))
    # more than 8192 code-blocks in a frame that encodes in milliseconds: the paths of the big frames
    for rev in (True, False):
        for rates in (None, MANY_RATES):
            seed += 1
            out.append(_case(f"many_4x4_300x200_rgb8_{'53' if rev else '97'}{'_rates' if rates else ''}", "many", w=300, h=200, nc=3, prec=8,
                             rev=rev, numres=5, cblk=(4, 4), seed=seed, rates=rates))
    assert len({c.name for c in out}) == len(out)
    return out


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
MANY = [c for c in CASES if c.kind == "many"]
KINDS = ("size", "precinct", "style", "rates", "many")
# every entry point (begin / end, borrowed, device, a sequence of two) is held to the same bytes for these
ENTRY_POINT_NAMES = ["size_4x4_rgb8_53", "size_64x4_grey12_97", "prec_p2_4x4_rgb8_53", "prec_p64_8_2_4x4_rgb8_53_tile40", "style55_4x4_rgb8_53",
                     "rates3_4x64_rgb8_97"]
# region decode: 4 x 4 blocks 9/7, 4 x 4 blocks 5/3 under 8 x 8 precincts, 8 x 4 blocks in tiles
REGION_NAMES = ["size_4x4_grey12_97", "prec_p8_4x4_rgb8_53", "region_8x4_rgb8_53_tile40"]
REGION_EXTRA = _case("region_8x4_rgb8_53_tile40", "region", cblk=(8, 4), seed=7999, prog=2, **dict(RGB8, **TILED))
BY_NAME[REGION_EXTRA.name] = REGION_EXTRA

# PCRL / CPRL under small precincts: libopenjp2's own files (tests/golden/make_golden.py --ext), the encoder's goldens too
EXT_NAMES = ["k1_67x45_rgb8_53_pcrl_prec8_cblk4", "k2_67x45_rgb8_53_cprl_prec8_cblk4", "k3_67x45_rgb8_53_pcrl_prec16x8_cblk8x4",
             "k4_67x45_rgb8_53_cprl_prec16x8_cblk8x4", "k5_67x45_rgb8_53_pcrl_prec32_8_cblk64", "k6_67x45_rgb8_53_cprl_prec32_8_cblk64"]


def safe_for_opj_encoder(c):
    """libopenjp2 2.4.0's encoder may be asked for this case: style 0, and no precinct size below 8 in the spec.  Outside this
    it refuses ("Cannot encode tile", "Size of code block data exceeds system limits") or crashes (termall on 4 x 4 blocks)."""
    return not c.style and (c.precincts is None or all(pw >= 8 and ph >= 8 for pw, ph in c.precincts))


def precinct_sizes(c):
    """[(w, h)] of every resolution's precincts, lowest resolution first (sizes halve below the last one given, never below 1)."""
    if c.precincts is None:
        return [(32768, 32768)] * c.numres
    out = []
    for k in range(c.numres):  # k = 0: the highest resolution
        if k < len(c.precincts):
            out.append(c.precincts[k])
        else:
            sh = k - (len(c.precincts) - 1)
            out.append((max(c.precincts[-1][0] >> sh, 1), max(c.precincts[-1][1] >> sh, 1)))
    return out[::-1]


def planes(c, seed_offset=0):
    pl = synth.planes(c.w, c.h, c.nc, c.prec, c.seed + seed_offset, "B" if c.seed & 1 else "A")
    pl.setflags(write=False)
    return pl


def oracle_params(c):
    from oracle.oracle import make_params
    return make_params(c.w, c.h, c.nc, c.prec, reversible=c.rev, mct=c.nc >= 3, numres=c.numres, cblk=c.cblk, layers=len(c.rates) if c.rates else 1,
                       tile=c.tile, prog=c.prog, mode=c.style, precincts=list(c.precincts) if c.precincts else None)


def api_kwargs(c, comment=""):
    """The keyword arguments of api.make_params(c.w, c.h, c.nc, c.prec, ...)."""
    return dict(reversible=c.rev, ycc=c.nc >= 3, tile_size=c.tile, num_resolutions=c.numres, cblk=c.cblk, comment=comment, progression=c.prog,
                precincts=list(c.precincts) if c.precincts else None, cblk_style=c.style, rates=list(c.rates) if c.rates else None)


def api_params(api, c, **override):
    kw = api_kwargs(c)
    kw.update(override)
    return api.make_params(c.w, c.h, c.nc, c.prec, **kw)


_FILES = {}


def oracle_file(oracle, c, comment=None):
    """The oracle's codestream of a case, written once per process."""
    key = (c.name, comment)
    if key not in _FILES:
        pl, p = planes(c), oracle_params(c)
        _FILES[key] = oracle.encode_rates(pl, p, list(c.rates), comment=comment) if c.rates else oracle.encode(pl, p, comment=comment)
    return _FILES[key]


def max_subsample(c):
    """The largest power of two (up to 4) a decode of the case may be sub-sampled by."""
    return min(4, 1 << (c.numres - 1))


# -- the layout of a case, worked out here from T.800 B.5 - B.7 alone (what the claims test counts) -------------------------------
def _cdiv(a, b):
    return -(-a // b)


def layout(c):
    """Per tile: the packets (precincts of every component and resolution times the layers) and, for every (component,
    resolution, precinct, band) that holds code-blocks, the (columns, rows) of its block grid and the blocks' (w, h)."""
    tw, th = (c.tile, c.tile) if c.tile else (c.w, c.h)
    layers = len(c.rates) if c.rates else 1
    sizes = precinct_sizes(c)
    tiles = []
    for ty0 in range(0, c.h, th):
        for tx0 in range(0, c.w, tw):
            tx1, ty1 = min(tx0 + tw, c.w), min(ty0 + th, c.h)
            packets, grids, blocks = 0, [], []
            for r in range(c.numres):
                lvl = c.numres - 1 - r
                rx0, ry0, rx1, ry1 = _cdiv(tx0, 1 << lvl), _cdiv(ty0, 1 << lvl), _cdiv(tx1, 1 << lvl), _cdiv(ty1, 1 << lvl)
                pw, ph = sizes[r]
                px0, py0 = rx0 // pw * pw, ry0 // ph * ph
                npx = 0 if rx1 == rx0 else (_cdiv(rx1, pw) * pw - px0) // pw
                npy = 0 if ry1 == ry0 else (_cdiv(ry1, ph) * ph - py0) // ph
                packets += npx * npy * c.nc * layers
                gw, gh = (pw, ph) if r == 0 else (pw // 2, ph // 2)  # a precinct's share of a band
                cw, ch = min(c.cblk[0], gw), min(c.cblk[1], gh)
                for orient in ((0,) if r == 0 else (1, 2, 3)):
                    if r == 0:
                        bx0, by0, bx1, by1 = rx0, ry0, rx1, ry1
                    else:
                        ox, oy = (orient & 1) << lvl, (orient >> 1) << lvl
                        bx0, by0 = _cdiv(tx0 - ox, 2 << lvl), _cdiv(ty0 - oy, 2 << lvl)
                        bx1, by1 = _cdiv(tx1 - ox, 2 << lvl), _cdiv(ty1 - oy, 2 << lvl)
                    gx0, gy0 = (px0, py0) if r == 0 else (_cdiv(px0, 2), _cdiv(py0, 2))
                    for j in range(npy):
                        for i in range(npx):
                            x0, y0 = max(gx0 + i * gw, bx0), max(gy0 + j * gh, by0)
                            x1, y1 = min(gx0 + (i + 1) * gw, bx1), min(gy0 + (j + 1) * gh, by1)
                            if x1 <= x0 or y1 <= y0:
                                continue
                            cols, rows = _cdiv(x1, cw) - x0 // cw, _cdiv(y1, ch) - y0 // ch
                            grids.append((cols, rows))
                            for bj in range(rows):
                                for bi in range(cols):
                                    cx, cy = (x0 // cw + bi) * cw, (y0 // ch + bj) * ch
                                    blocks.append((min(cx + cw, x1) - max(cx, x0), min(cy + ch, y1) - max(cy, y0)))
            tiles.append(dict(packets=packets, grids=grids * c.nc, blocks=blocks * c.nc))
    return tiles


# -- the PCRL / CPRL goldens -----------------------------------------------------------------------------------------------------
_GOLDEN = {}


def ext_entry(name):
    if not _GOLDEN:
        with open(os.path.join(GOLDEN_DIR, "golden.json")) as f:
            g = json.load(f)
        _GOLDEN.update({k: g[k] for k in EXT_NAMES})
    return _GOLDEN[name]


def ext_bytes(name):
    with open(os.path.join(GOLDEN_DIR, "ext", name + ".j2k"), "rb") as f:
        return f.read()


def ext_planes(name):
    g = ext_entry(name)
    return synth.planes(g["width"], g["height"], g["ncomp"], g["prec"], g["seed"], g["dist"])


def ext_api_params(api, name):
    g = ext_entry(name)
    kw = g["ext"]
    return api.make_params(g["width"], g["height"], g["ncomp"], g["prec"], reversible=kw.get("reversible", True), ycc=kw.get("mct", False),
                           num_resolutions=kw["numres"], cblk=tuple(kw.get("cblk", (64, 64))), comment="", progression=kw.get("prog", 0),
                           precincts=[tuple(p) for p in kw["precincts"]])
