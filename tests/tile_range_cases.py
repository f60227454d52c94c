"""Cases of the tile-range parity sweep, shared by test_tile_range_refs.py (CPU) and test_tile_ranges.py (GPU).  Helpers only.

A tile range (first, count) is the one caller that moves the encoder's working box off (0, 0): prepare_geometry cuts the planes
to the bounding box of the requested tiles and every offset behind it (front end, fused level-1 jobs, DwtJob, CblkDev::coef_off,
the rows upload_planes copies) is relative to that box.  The reference of every case is the CPU oracle's codestream of the whole
frame, split at its SOT markers (sharding.split_tileparts): a range must return exactly parts[first:first + count] joined.

  Geo       frame size, components, depth, tile size, resolutions (the table of the geometries A .. F)
  Config    a Geo with its wavelet, MCT and the coding variant (layers, progression, precincts, code-block size / style, rates)
  view      how the frame reaches the encoder (VIEWS): an After Effects ARGB frame with padded rows, the same under no_fuse = 1,
            planar 16-bit planes of 10 significant bits with padded rows, both of them bottom-up (base = the last row, negative
            rowbytes), and a 15+1-bit ARGB64 world under promote_ae16
  Src       one (Config, view): the frame bytes, its channel views, the samples the codec is to see (numpy alone), the knobs

Deeper decompositions of 1 - 2-sample tiles are not in the table on purpose: libopenjp2 2.4.0 itself crashes on 133 x 100 / tile
33 with 6 or 7 resolutions, 61 x 47 / tile 20 with 6 and 134 x 101 / tile 33 with 6 under 9/7 (heap corruption or its
`dn + sn > 1` assertion), so no byte-exact reference exists for them.
"""
from __future__ import annotations

import random
from collections import namedtuple

import numpy as np

import depth_cases
import dwt_variant_cases as dv
from j2k_amd import sharding, synth

Geo = namedtuple("Geo", "id w h nc prec tile numres seed")
Config = namedtuple("Config", "name geo rev mct layers prog precincts cblk style rates")
Src = namedtuple("Src", "buf chans samples promote knobs")
Chan = dv.Chan

GEOS = {g.id: g for g in (
    Geo("A", 133, 100, 3, 8, 33, 3, 9101),    # odd tile origins, a 1-wide last column, a 1-high last row
    Geo("B", 150, 110, 3, 8, 40, 4, 9102),    # tiles no multiple of 64: code-blocks cut on the left and at the top
    Geo("C", 150, 130, 1, 16, 64, 5, 9103),   # aligned tiles, one component
    Geo("D", 199, 101, 3, 10, 100, 6, 9104),  # box origin 100; a 1-high bottom row under five levels
    Geo("E", 130, 129, 3, 8, 128, 6, 9105),   # 2-wide and 1-high edge tiles under 9/7
    Geo("F", 135, 102, 4, 16, 33, 3, 9106),   # four components, 3-sample edge tiles
)}

PROG_NAMES = ("lrcp", "rlcp", "rpcl", "pcrl", "cprl")


def _cfg(name, geo, rev, mct, layers=1, prog=0, precincts=None, cblk=(64, 64), style=0, rates=None):
    return Config(name, GEOS[geo], rev, mct, len(rates) if rates else layers, prog, tuple(precincts) if precincts else None, cblk, style,
                  tuple(rates) if rates else None)


BASE = [
    _cfg("A_53_rct", "A", True, True),
    _cfg("B_53_rct", "B", True, True),
    _cfg("B_97_ict", "B", False, True),
    _cfg("C_97", "C", False, False),
    _cfg("D_53_nomct", "D", True, False),
    _cfg("E_97_ict", "E", False, True),
    _cfg("F_97_ict", "F", False, True),
]
# the coding variants, on geometry B only: 2 layers under every progression order (5/3 and 9/7 in turn), RPCL with 32 x 32
# precincts and 3 layers, 16 x 16 code-blocks under bypass | termall, a byte budget of two layers under 9/7
VARIANTS = [_cfg(f"B_{'53_rct' if k % 2 == 0 else '97_ict'}_2layers_{PROG_NAMES[k]}", "B", k % 2 == 0, True, layers=2, prog=k) for k in range(5)] + [
    _cfg("B_97_ict_rpcl_prec32_3layers", "B", False, True, layers=3, prog=2, precincts=[(32, 32)]),
    _cfg("B_53_rct_cblk16_bypass_termall", "B", True, True, cblk=(16, 16), style=1 | 4),
    _cfg("B_97_ict_rates_20_5", "B", False, True, rates=[20.0, 5.0]),
]
CONFIGS = BASE + VARIANTS
BY_NAME = {c.name: c for c in CONFIGS}
assert len(BY_NAME) == len(CONFIGS)

VIEWS = ("ae", "ae_nofuse", "planar10", "ae_bottomup", "planar10_bottomup", "promote")
# which samples a view carries: the frame's own, 10-bit planes converted to the file depth, the Promote of a 15+1-bit world
KIND = {"ae": "ae", "ae_nofuse": "ae", "ae_bottomup": "ae", "planar10": "planar", "planar10_bottomup": "planar", "promote": "promote"}
# every geometry gets the first view, every view at least A and B; the others where they fit (10-bit planes on the 10-bit frame,
# Promote on the four-component 16-bit frame, the stand-alone front end on the deepest transform of edge tiles)
_VIEWS_OF = {
    "A_53_rct": VIEWS,
    "B_53_rct": VIEWS,
    "B_97_ict": ("ae", "ae_nofuse", "planar10_bottomup", "promote"),
    "C_97": ("ae", "planar10"),
    "D_53_nomct": ("ae", "planar10", "ae_bottomup"),
    "E_97_ict": ("ae", "ae_nofuse"),
    "F_97_ict": ("ae", "planar10_bottomup", "promote"),
}
PAIRS = [(c, v) for c in CONFIGS for v in _VIEWS_OF.get(c.name, ("ae",))]
ENTRIES = ("device", "host")


def pair_id(cv):
    return f"{cv[0].name}-{cv[1]}"


# ---------------------------------------------------------------------------------------------------------------------- tiles
def grid(g: Geo):
    """(ntx, nty)."""
    return -(-g.w // g.tile), -(-g.h // g.tile)


def ntiles(g: Geo) -> int:
    ntx, nty = grid(g)
    return ntx * nty


def tile_rect(g: Geo, t: int):
    ntx, _ = grid(g)
    x0, y0 = (t % ntx) * g.tile, (t // ntx) * g.tile
    return x0, y0, min(x0 + g.tile, g.w), min(y0 + g.tile, g.h)


def box(g: Geo, first: int, count: int):
    """(x0, y0, x1, y1) of the working box of a range: the bounding box of its tiles, as prepare_geometry takes it."""
    r = [tile_rect(g, t) for t in range(first, first + count)]
    return min(a[0] for a in r), min(a[1] for a in r), max(a[2] for a in r), max(a[3] for a in r)


def unrequested(g: Geo, first: int, count: int):
    """The tiles that lie inside the box of the range without belonging to it."""
    x0, y0, x1, y1 = box(g, first, count)
    out = []
    for t in range(ntiles(g)):
        a = tile_rect(g, t)
        if not first <= t < first + count and a[0] < x1 and x0 < a[2] and a[1] < y1 and y0 < a[3]:
            out.append(t)
    return out


def box_kind(g: Geo, first: int, count: int) -> str:
    ntx, _ = grid(g)
    if count == 1:
        x0, y0, _, _ = box(g, first, 1)
        return "single_interior" if x0 and y0 else "single"
    if first // ntx == (first + count - 1) // ntx:
        return "whole_rows" if count == ntx else "row_run"
    if first % ntx == 0 and count % ntx == 0:
        return "whole_rows"
    return "crosses_row_end"


def ranges(g: Geo):
    """Every contiguous (first, count) for grids of at most 12 tiles; for larger grids every single tile, the whole grid and every
    range of count 2, ntx and ntx + 1."""
    n, (ntx, _) = ntiles(g), grid(g)
    if n <= 12:
        return [(f, c) for f in range(n) for c in range(1, n - f + 1)]
    out = [(t, 1) for t in range(n)] + [(0, n)]
    for c in (2, ntx, ntx + 1):
        out += [(f, c) for f in range(n - c + 1)]
    return list(dict.fromkeys(out))


def shuffled_ranges(g: Geo, seed: int):
    """ranges(g) in the order one handle sees them: the geometry cache is keyed on the range."""
    r = ranges(g)
    random.Random(seed).shuffle(r)
    return r


def single_tiles(g: Geo):
    return [(t, 1) for t in range(ntiles(g))]


def partitions(g: Geo):
    """[(world, [(first, count), ...])] for world = 1 .. ntiles + 1, empty shares left out."""
    n = ntiles(g)
    return [(w, [s for s in sharding.partition_tiles(n, w) if s[1]]) for w in range(1, n + 2)]


BAD_RANGES = ("count_zero", "first_at_ntiles", "first_beyond", "end_beyond", "end_wraps_32_bits")


def bad_range(g: Geo, what: str):
    n = ntiles(g)
    return {"count_zero": (0, 0), "first_at_ntiles": (n, 1), "first_beyond": (n + 7, 1), "end_beyond": (n - 1, 2),
            "end_wraps_32_bits": (n - 1, 0xffffffff - (n - 1) + 2)}[what]  # (first + count = 2^32 + 1: 1 in 32 bits)


# ---------------------------------------------------------------------------------------------------------------------- samples
_samples = {}


def _world16(g: Geo):
    """After Effects 15+1-bit samples 0 .. 32768, as test_gpu_parity.py::_ae16_planes makes them."""
    pl = synth.planes(g.w, g.h, g.nc, 15, g.seed + 2, "A")
    pl[:, ::7, ::5] = 32768
    pl[:, 1::9, 2::11] = 16384
    pl[:, 2::13, 1::3] = 16385
    pl[:, 3::17, ::19] = 0
    return pl


def _stored(g: Geo, kind: str):
    """What the frame stores, (nc, h, w) int32: samples of the file depth, of 10 bits, or of the 15+1-bit world."""
    if kind == "ae":
        return synth.planes(g.w, g.h, g.nc, g.prec, g.seed)
    if kind == "planar":
        return synth.planes(g.w, g.h, g.nc, 10, g.seed + 1)
    return _world16(g)


def samples(g: Geo, kind: str) -> np.ndarray:
    """(nc, h, w) int32: the unsigned samples of g.prec bits the codec is to see -- numpy alone, no oracle.  "planar": CopyChannel
    10 -> prec; "promote": Promote, then CopyChannel 16 -> prec (the model of test_promote_ae16_whole_codestream)."""
    key = (g, kind)
    if key not in _samples:
        st = _stored(g, kind).astype(np.int64)
        if kind == "planar":
            st = depth_cases.convert(st, 10, g.prec)
        elif kind == "promote":
            st = depth_cases.convert(np.where(st > 16384, ((st - 1) << 1) + 1, st << 1), 16, g.prec)
        out = np.ascontiguousarray(st.astype(np.int32))
        assert out.min() >= 0 and out.max() < (1 << g.prec)
        out.setflags(write=False)
        _samples[key] = out
    return _samples[key]


# ---------------------------------------------------------------------------------------------------------------------- sources
PLANAR_PAD = 6  # bytes behind every row of a 16-bit plane: rows of 2-byte, not 4-byte, alignment
_sources = {}


def source(g: Geo, view: str) -> Src:
    key = (g, view)
    if key in _sources:
        return _sources[key]
    kind, up = KIND[view], view.endswith("bottomup")
    st = _stored(g, kind)
    if up:
        st = st[:, ::-1]  # row r of the image is row h - 1 - r of the buffer
    if kind == "planar":
        rowbytes = 2 * g.w + PLANAR_PAD
        psize = -(-g.h * rowbytes // 16) * 16
        buf = np.full(g.nc * psize, 0xEE, np.uint8)
        chans = []
        for c in range(g.nc):
            rows = buf[c * psize:c * psize + g.h * rowbytes].reshape(g.h, rowbytes)
            rows[:, :2 * g.w] = np.ascontiguousarray(st[c].astype("<u2")).view(np.uint8).reshape(g.h, 2 * g.w)
            chans.append(Chan(c * psize, 2, rowbytes, 2, 10))
    else:
        bits = 16 if kind == "promote" else (8 if g.prec <= 8 else 16)
        buf, lay = synth.ae_frame(st, g.prec if kind == "ae" else 16, row_pad_bytes=bits // 2)  # (a multiple of the pixel: still interleaved)
        offs = lay["channel_offsets"]
        order = [offs[1], offs[2], offs[3], offs[0]]
        chans = [Chan(order[c], lay["colbytes"], lay["rowbytes"], lay["sample_bytes"], bits) for c in range(g.nc)]
    if up:
        chans = [ch._replace(off=ch.off + (g.h - 1) * ch.rowbytes, rowbytes=-ch.rowbytes) for ch in chans]
    buf.setflags(write=False)
    src = Src(buf, chans, samples(g, kind), kind == "promote", dict(no_fuse=1) if view == "ae_nofuse" else {})
    _sources[key] = src
    return src


def read_back(g: Geo, src: Src) -> np.ndarray:
    """The stored samples as the channel views address them, (nc, h, w) int64: numpy's reading of base / colbytes / rowbytes."""
    out = np.empty((g.nc, g.h, g.w), np.int64)
    y, x = np.arange(g.h)[:, None], np.arange(g.w)[None, :]
    for c, ch in enumerate(src.chans):
        at = ch.off + y * ch.rowbytes + x * ch.colbytes
        out[c] = src.buf[at] if ch.sample_bytes == 1 else src.buf[at].astype(np.int64) | (src.buf[at + 1].astype(np.int64) << 8)
    return out


POISON = 0xA5


def poisoned(g: Geo, src: Src, y0: int, y1: int) -> np.ndarray:
    """A copy of the frame in which every byte is flipped by POISON except the samples of rows [y0, y1) of the channels: a host
    encode of a range whose box covers those rows may read nothing else, and whatever else it read as a sample would differ."""
    keep = np.zeros(src.buf.size, bool)
    y, x = np.arange(y0, y1)[:, None], np.arange(g.w)[None, :]
    for ch in src.chans:
        at = ch.off + y * ch.rowbytes + x * ch.colbytes
        for b in range(ch.sample_bytes):
            keep[at + b] = True
    return np.where(keep, src.buf, src.buf ^ POISON).astype(np.uint8)


def plane_views(api, src: Src):
    """address of the buffer (host or device) -> j2k_hip_plane array."""
    return dv.plane_views(api, src.chans)


# ---------------------------------------------------------------------------------------------------------------------- parameters
def oracle_params(c: Config):
    from oracle.oracle import make_params
    g = c.geo
    return make_params(g.w, g.h, g.nc, g.prec, reversible=c.rev, mct=c.mct, numres=g.numres, cblk=c.cblk, layers=c.layers, tile=g.tile,
                       prog=c.prog, mode=c.style, precincts=list(c.precincts) if c.precincts else None)


def api_params(api, c: Config, promote: bool = False):
    g = c.geo
    return api.make_params(g.w, g.h, g.nc, g.prec, reversible=c.rev, ycc=c.mct, layers=c.layers, tile_size=g.tile, num_resolutions=g.numres,
                           cblk=c.cblk, promote=promote, comment="", progression=c.prog, precincts=list(c.precincts) if c.precincts else None,
                           cblk_style=c.style, rates=list(c.rates) if c.rates else None)


_files = {}


def oracle_file(oracle, c: Config, kind: str = "ae", comment=None) -> bytes:
    """The oracle's whole codestream of a configuration's samples, written once per process."""
    key = (c.name, kind, comment)
    if key not in _files:
        pl, p = samples(c.geo, kind), oracle_params(c)
        _files[key] = oracle.encode_rates(pl, p, list(c.rates), comment=comment) if c.rates else oracle.encode(pl, p, comment=comment)
    return _files[key]


def reference(oracle, c: Config, kind: str = "ae"):
    """(whole file, main header, [tile-part bytes])."""
    cs = oracle_file(oracle, c, kind)
    hdr, parts = sharding.split_tileparts(cs)
    return cs, hdr, parts


def safe_for_opj_encoder(c: Config) -> bool:
    """libopenjp2 2.4.0's encoder is asked for style 0 only: under termall it has crashed on small blocks, in-process."""
    return not c.style


# ---------------------------------------------------------------------------------------------------------------------- launch shapes
# the knob sets dwt_variant_cases.knobs() takes, for the single-tile ranges of A and F: the fused level-1 kernel's workgroup and
# chunk shapes, the level kernel's under the stand-alone front end (level 1 included) and three of them behind the fused kernel
LAUNCH_CONFIGS = ("A_53_rct", "F_97_ict")
LAUNCH_KNOBS = dv.FUSED_KNOBS + [dict(fused_generic=1)] + [dict(k, no_fuse=1) for k in dv.LEVEL_KNOBS] + \
    [dict(dwt_pairs=1), dict(dwt_ppc=1), dict(dwt_xcd=0)]


# ---------------------------------------------------------------------------------------------------------------------- GPU calls
def tiles_device(api, enc, planes, p, first: int, count: int) -> bytes:
    """j2k_hip_encode_tiles_device of any channel views (device pointers)."""
    import ctypes as C
    dptr, n = C.c_void_p(), C.c_size_t()
    enc._check(enc.L.j2k_hip_encode_tiles_device(enc.h, C.byref(p), planes, first, count, C.byref(dptr), C.byref(n), None, 0))
    return enc.d2h(dptr.value, n.value).tobytes()
