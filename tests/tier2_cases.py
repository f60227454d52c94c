"""What tests/test_tier2_plan_refs.py and tests/test_tier2_plan.py share: host Tier-2's plan (api.host_tier2_plan) against two
references that share no code with tier2.cpp -- the libopenjp2 files under tests/golden/ and the oracle's packet reader
(oracle/j2k_oracle_dec.c, written from T.800 Annex B).

A block table here is a list, in api.frame_blocks order, of a block's numbps and its *pieces*: [(layer, bytes, passes), ...],
one per length field a packet header holds for it -- the form Oracle.file_blocks(data, layers=True) reports.  From the pieces
follow the planner's inputs (table_inputs): npasses, length, the layer allocation np / len / off and, under a code-block style,
the per-pass byte counts at the piece ends.

The geometry used by the census (precinct grids, segment boundaries, Lblock) is worked out here from T.800 B.6, B.7, B.10 and the
block table alone; nothing of it is read from the planner's output."""
import glob
import json
import os

import numpy as np

from j2k_amd.api import MAX_PASSES

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_oracle = None


def oracle():
    global _oracle
    if _oracle is None:
        from oracle.oracle import Oracle
        _oracle = Oracle()
    return _oracle


def cdp2(a, b):
    return -((-a) >> b)


def flog2(a):
    return max(int(a), 1).bit_length() - 1


# ---------------------------------------------------------------------------------------------------------------- files
def codestream_of(data: bytes) -> bytes:
    """The contiguous codestream box of a JP2 file; a raw codestream as it is."""
    if data[:4] == b"\xff\x4f\xff\x51":
        return data
    pos = 0
    while pos + 8 <= len(data):
        ln, typ, hdr = int.from_bytes(data[pos:pos + 4], "big"), data[pos + 4:pos + 8], 8
        if ln == 1:
            ln, hdr = int.from_bytes(data[pos + 8:pos + 16], "big"), 16
        elif ln == 0:
            ln = len(data) - pos
        if typ == b"jp2c":
            return data[pos + hdr:pos + ln]
        pos += ln
    raise ValueError("no codestream box")


def header_fields(cs: bytes) -> dict:
    """SIZ, COD and QCD of a codestream's main header, and the markers it holds."""
    f = dict(markers=[])
    i = 2
    while cs[i:i + 2] != b"\xff\x90":
        m, ln = int.from_bytes(cs[i:i + 2], "big"), int.from_bytes(cs[i + 2:i + 4], "big")
        s = cs[i + 4:i + 2 + ln]
        f["markers"].append(m)
        if m == 0xff51:
            u32 = lambda o: int.from_bytes(s[o:o + 4], "big")
            f.update(rsiz=int.from_bytes(s[0:2], "big"), width=u32(2), height=u32(6), origin=(u32(10), u32(14), u32(26), u32(30)), tile=(u32(18), u32(22)),
                     ncomp=int.from_bytes(s[34:36], "big"))
            f["comps"] = [(s[36 + 3 * c], s[37 + 3 * c], s[38 + 3 * c]) for c in range(f["ncomp"])]
        elif m == 0xff52:
            f.update(scod=s[0], prog=s[1], layers=int.from_bytes(s[2:4], "big"), mct=s[4], numres=s[5] + 1, cblk=(1 << (s[6] + 2), 1 << (s[7] + 2)),
                     style=s[8], reversible=s[9] == 1)
            f["pp"] = [(s[10 + r] & 15, s[10 + r] >> 4) for r in range(f["numres"])] if s[0] & 1 else None  # lowest resolution first
        elif m == 0xff5c:
            f.update(guard=s[0] >> 5)
        i += 2 + ln
    return f


def fixture_files():
    """Every .j2k / .jp2 under tests/golden outside cut/ and damaged/, as paths relative to tests/golden."""
    out = []
    for p in sorted(glob.glob(os.path.join(GOLDEN_DIR, "**", "*.j*"), recursive=True)):
        rel = os.path.relpath(p, GOLDEN_DIR)
        if p.endswith((".j2k", ".jp2")) and not rel.startswith(("cut" + os.sep, "damaged" + os.sep)):
            out.append(rel)
    return out


_fixtures = {}


def read_fixture(rel):
    """(codestream without COM, the reader's parse with pieces) or (codestream, None) where the oracle's reader refuses it."""
    from oracle.oracle import strip_com
    if rel not in _fixtures:
        cs = strip_com(codestream_of(open(os.path.join(GOLDEN_DIR, rel), "rb").read()))
        try:
            _fixtures[rel] = cs, oracle().file_blocks(cs, layers=True)
        except RuntimeError:
            _fixtures[rel] = cs, None
    return _fixtures[rel]


def is_candidate(cs, parsed) -> bool:
    """The reader takes it, and its COD has neither SOP / EPH nor vertically causal contexts (the encoder writes neither)."""
    if parsed is None:
        return False
    f = header_fields(cs)
    return not (f["scod"] & 6) and not (f["style"] & 8)


with open(os.path.join(GOLDEN_DIR, "golden.json")) as _f:
    GOLDEN = json.load(_f)


def params_for(api, rel, cs):
    """The encoder's parameters for a committed file: from golden.json as tests/test_gpu_parity.py derives them where the file
    is listed there, from the main header otherwise; what golden.json does not hold (progression, precincts, code-block style,
    guard bits, cinema profile) from the main header in both cases.  comment = "": no COM.  Raises ValueError with the reason
    where the parameters cannot express the file."""
    f = header_fields(cs)
    if any(f["origin"]):
        raise ValueError("image or tile grid offset")
    if any(c != (f["comps"][0][0], 1, 1) for c in f["comps"]) or f["comps"][0][0] & 0x80:
        raise ValueError("components differ in depth, are signed or sub-sampled")
    tw, th = f["tile"]
    if tw >= f["width"] and th >= f["height"]:
        tile = 0
    elif tw == th:
        tile = tw
    else:
        raise ValueError("tiles are not square")
    kw = dict(width=f["width"], height=f["height"], channels=f["ncomp"], depth=(f["comps"][0][0] & 0x7f) + 1, reversible=f["reversible"], ycc=bool(f["mct"]),
              layers=f["layers"], tile_size=tile, num_resolutions=f["numres"], cblk=f["cblk"])
    g = GOLDEN.get(os.path.splitext(os.path.basename(rel))[0]) if os.sep not in rel else None
    if g is not None:
        k = g["params"]
        kw.update(width=g["width"], height=g["height"], channels=g["ncomp"], depth=g["prec"], reversible=k.get("reversible", True), ycc=k.get("mct", False),
                  layers=k.get("layers", kw["layers"]), tile_size=k.get("tile", 0), num_resolutions=k.get("numres", 6), cblk=tuple(k.get("cblk", (64, 64))))
    if f["rsiz"] in (3, 4):
        kw.update(dci_profile=f["rsiz"])
    elif f["rsiz"]:
        raise ValueError("Rsiz %d" % f["rsiz"])
    if f["pp"] is not None and not kw.get("dci_profile"):
        kw.update(precincts=[(1 << px, 1 << py) for px, py in reversed(f["pp"])])
    if f["guard"] != 2:
        kw.update(guard_bits=f["guard"])
    w, h, c, d = (kw.pop(n) for n in ("width", "height", "channels", "depth"))
    return api.make_params(w, h, c, d, progression=f["prog"], cblk_style=f["style"], comment="", **kw)


# ------------------------------------------------------------------------------------------------------- block tables
def band_origin_in_plane(fb):
    """Per row of frame_blocks, the block's (x, y) relative to its band's origin: a band's first block starts there."""
    key = (fb[:, 0].astype(np.int64) << 32) | (fb[:, 1].astype(np.int64) << 24) | (fb[:, 2].astype(np.int64) << 8) | fb[:, 4].astype(np.int64)
    rel = np.zeros((fb.shape[0], 2), np.int64)
    for k in np.unique(key):
        m = key == k
        rel[m, 0] = fb[m, 5].astype(np.int64) - int(fb[m, 5].min())
        rel[m, 1] = fb[m, 6].astype(np.int64) - int(fb[m, 6].min())
    return rel


def table_from_reader(api, params, cs, parsed):
    """The reader's blocks in frame_blocks order: (numbps list, pieces list, bytes list).  Blocks are matched by tile, component,
    resolution, orientation and position relative to the band's origin (the reader's x, y lie in the tile-component's plane: the
    band's origin there is the size of the resolution below); a block the file does not list has no passes."""
    f = header_fields(cs)
    fb = api.frame_blocks(params)
    rel = band_origin_in_plane(fb)
    index = {(int(r[0]), int(r[1]), int(r[2]), int(r[4]), int(x), int(y)): i for i, (r, (x, y)) in enumerate(zip(fb, rel))}
    n = fb.shape[0]
    numbps, pieces, data = [0] * n, [[] for _ in range(n)], [b""] * n
    tw, th = f["tile"]
    ntx = -(-f["width"] // tw)
    NL = f["numres"] - 1
    seen = set()
    for b in parsed["blocks"]:
        t, r, o = b["tile"], b["res"], b["orient"]
        tx0, ty0 = (t % ntx) * tw, (t // ntx) * th
        tx1, ty1 = min(tx0 + tw, f["width"]), min(ty0 + th, f["height"])
        lv = NL - r + 1  # the resolution below this one
        offx = cdp2(tx1, lv) - cdp2(tx0, lv) if r and (o & 1) else 0
        offy = cdp2(ty1, lv) - cdp2(ty0, lv) if r and (o & 2) else 0
        i = index[(t, b["comp"], r, o, b["rect"][0] - offx, b["rect"][1] - offy)]
        assert i not in seen and (int(fb[i, 7]), int(fb[i, 8])) == (b["w"], b["h"])
        seen.add(i)
        numbps[i], pieces[i], data[i] = b["numbps"], list(b["pieces"]), b["data"]
    return numbps, pieces, data


def pass_terminates(style, p):
    """Does pass p end a codeword segment (T.800 D.4 / D.6; the block's last pass aside)?  Every pass under termall; under
    bypass the fourth bit-plane's cleanup pass (p = 9), then every refinement pass (it closes the raw pair) and every cleanup."""
    return bool(style & 4) or (bool(style & 1) and (p == 9 or (p >= 10 and p % 3 != 1)))


def table_inputs(style, layers, numbps, pieces, with_alloc):
    """The planner's inputs of a block table: dict(numbps, npasses, length, rates, alloc)."""
    n = len(numbps)
    npasses = np.array([sum(p[2] for p in pc) for pc in pieces], np.uint32)
    length = np.array([sum(p[1] for p in pc) for pc in pieces], np.uint32)
    rates = alloc = None
    if style:
        rates = np.zeros((n, MAX_PASSES), np.uint32)
        for i, pc in enumerate(pieces):
            done = nbytes = 0
            for _, ln, npass in pc:  # the passes of a piece all carry the piece's end: the table stays non-decreasing
                nbytes += ln
                rates[i, done:done + npass] = nbytes
                done += npass
    if with_alloc:
        alloc = tuple(np.zeros((n, layers), np.uint32) for _ in range(3))
        for i, pc in enumerate(pieces):
            at = 0
            for lay, ln, npass in pc:
                if alloc[0][i, lay] == 0:
                    alloc[2][i, lay] = at
                alloc[0][i, lay] += npass
                alloc[1][i, lay] += ln
                at += ln
    return dict(numbps=np.array(numbps, np.uint32), npasses=npasses, length=length, rates=rates, alloc=alloc)


def plan_table(api, params, style, layers, numbps, pieces, with_alloc, workers=0):
    t = table_inputs(style, layers, numbps, pieces, with_alloc)
    return api.host_tier2_plan(params, t["numbps"], t["npasses"], t["length"], rates=t["rates"], alloc=t["alloc"], workers=workers)


# -------------------------------------------------------------------------------------------------- synthetic tables
PASS_RANGES = ((1, 1), (2, 2), (3, 5), (6, 36), (37, 94))  # Table B.4's five codes
GRIDS = {"1x1": (4, 4), "1xn": (3, 20), "nx1": (20, 3), "2x2": (8, 8), "3x5": (12, 20), "17x17": (67, 65)}  # frames of 4 x 4 blocks, one resolution
PATTERNS = ("all", "none", "corner", "checker")


def layer_segments(style, first, npass):
    """The passes [first, first + npass) of one layer's contribution, cut into the runs that share a length field (B.10.7.2)."""
    out, run = [], 0
    for p in range(first, first + npass):
        run += 1
        if pass_terminates(style, p) or p + 1 == first + npass:
            out.append(run)
            run = 0
    return out


def block_geometry(case, fb):
    """Per row of frame_blocks: the packet it belongs to (tile, comp, res, precinct x, y) and its leaf (column, row) in the
    precinct's grid of its band (T.800 B.6, B.7), from the case's parameters alone."""
    W, H = case["size"]
    ts = case["mk"].get("tile_size", 0)
    tw, th = (ts, ts) if ts else (W, H)
    ntx = -(-W // tw)
    numres = case["mk"]["num_resolutions"]
    NL = numres - 1
    cbw, cbh = (flog2(v) for v in case["mk"]["cblk"])
    prc = case["mk"].get("precincts")
    rel = band_origin_in_plane(fb)
    packets, leaves = [], []
    for row, (rx, ry) in zip(fb.tolist(), rel.tolist()):
        t, c, r, _, o = row[:5]
        tx0, ty0 = (t % ntx) * tw, (t // ntx) * th
        ppx, ppy = (flog2(prc[numres - 1 - r][0]), flog2(prc[numres - 1 - r][1])) if prc else (15, 15)
        if r == 0:
            bx0, by0, pcx, pcy = cdp2(tx0, NL), cdp2(ty0, NL), ppx, ppy
        else:
            nb = NL - r + 1
            bx0, by0 = cdp2(tx0 - ((o & 1) << (nb - 1)), nb), cdp2(ty0 - ((o >> 1) << (nb - 1)), nb)
            pcx, pcy = ppx - 1, ppy - 1
        ax, ay = bx0 + rx, by0 + ry
        packets.append((t, c, r, ax >> pcx, ay >> pcy))
        leaves.append((ax >> min(cbw, pcx), ay >> min(cbh, pcy)))
    return packets, leaves


def units_of(case, fb):
    """{(packet, orientation): [(column, row, block), ...]} with columns and rows counted from the grid's corner."""
    packets, leaves = block_geometry(case, fb)
    units = {}
    for i, (pk, lf) in enumerate(zip(packets, leaves)):
        units.setdefault(pk + (int(fb[i, 4]),), []).append((lf[0], lf[1], i))
    for k, v in units.items():
        x0, y0 = min(a[0] for a in v), min(a[1] for a in v)
        units[k] = [(x - x0, y - y0, i) for x, y, i in v]
    return units


def _draw_len(rng, room):
    """A piece's bytes: nothing, one, a power of two or one less, or anything, within what the block's slot has left."""
    if room <= 0:
        return 0
    u = rng.random()
    if u < 0.12:
        return 0
    if u < 0.2:
        return 1
    lim = room if rng.random() < 0.25 else max(1, room // 8)
    if u < 0.6:
        k = int(rng.integers(1, flog2(lim) + 1)) if lim >= 2 else 0
        return min(lim, (1 << k) - int(rng.integers(0, 2)))
    return int(rng.integers(1, lim + 1))


def _draw_passes(rng, left):
    lo, hi = PASS_RANGES[int(rng.integers(0, sum(1 for a, _ in PASS_RANGES if a <= left)))]
    return int(rng.integers(lo, min(hi, left) + 1))


def _gen_block(rng, Mb, cap, layers, style, first=None, deep=False):
    """numbps <= Mb, passes <= 3 numbps - 2, bytes <= cap, a layer's pieces contiguous.  first: the layer of the first
    inclusion (None: drawn, or never); deep: as many bit-planes as the band has."""
    numbps = Mb if deep or rng.random() < 0.4 else int(rng.integers(0, Mb + 1))
    left = 3 * numbps - 2 if numbps else 0
    if first is None:
        first = int(rng.integers(0, layers + 1))  # `layers`: never included
    if left <= 0 or first >= layers:
        return 0, []
    pieces, done, room = [], 0, cap
    for lay in range(first, layers):
        if left == 0 or (lay > first and rng.random() < 0.35):
            continue  # the block skips this layer
        npass = _draw_passes(rng, left)
        for run in layer_segments(style, done, npass):
            ln = _draw_len(rng, room)
            pieces.append((lay, ln, run))
            room -= ln
            done += run
        left -= npass
    return numbps, pieces


def make_params(api, case, **over):
    w, h = case["size"]
    kw = dict(case["mk"], layers=case["layers"], cblk_style=case["style"], comment="")
    kw.update(over)
    return api.make_params(w, h, case["channels"], case["depth"], **kw)


_caps = {}


def capacities(api, fb, style):
    out = []
    for row in fb.tolist():
        k = (row[7] * row[8], row[9], style)
        if k not in _caps:
            _caps[k] = api.cblk_capacities(*k)[1]
        out.append(_caps[k])
    return out


def synth_table(api, case):
    """The block table of a case: dict(params, fb, caps, numbps, pieces, data)."""
    params = make_params(api, case)
    fb = api.frame_blocks(make_params(api, case, guard_bits=case["table_guard"]) if "table_guard" in case else params)
    rng = np.random.default_rng(case["seed"])
    L, style, flavor = case["layers"], case["style"], case.get("flavor", "")
    caps = capacities(api, fb, style)
    n = fb.shape[0]
    numbps, pieces = [0] * n, [[] for _ in range(n)]
    if flavor != "empty":
        for i in range(n):
            numbps[i], pieces[i] = _gen_block(rng, int(fb[i, 9]), caps[i], L, style, deep=case.get("deep", False))
    units = units_of(case, fb)
    if flavor.startswith("grid:"):
        # layer 0 holds the pattern on every grid; layer 1 brings every other block in
        pat = flavor[5:]
        for v in units.values():
            cw, ch = 1 + max(a[0] for a in v), 1 + max(a[1] for a in v)
            for x, y, i in v:
                inside = {"all": True, "none": False, "corner": (x, y) == (cw - 1, ch - 1), "checker": (x + y) % 2 == 0}[pat]
                numbps[i], pieces[i] = _gen_block(rng, int(fb[i, 9]), caps[i], L, style, first=0 if inside else 1, deep=True)
    elif flavor == "lblock":
        # one packet: Lblock steps of 0, 1 and 8 side by side, and a block whose Lblock rises in three layers
        v = sorted(max(units.values(), key=len), key=lambda a: (a[1], a[0]))
        assert len(v) >= 4 and all(caps[a[2]] >= 2048 for a in v[:4]) and L >= 3
        for (_, _, i), pc in zip(v, ([(0, 5, 1)], [(0, 8, 1)], [(0, 1024, 1)], [(0, 9, 1), (1, 70, 1), (2, 1500, 1)])):
            numbps[i], pieces[i] = int(fb[i, 9]), pc
    elif flavor == "zbp":
        # the band with the most bit-planes: zero bit-planes 0, 1, .., Mb - 1 in one precinct
        Mb = int(fb[:, 9].max())
        v = next(v for v in units.values() if int(fb[v[0][2], 9]) == Mb and len(v) >= Mb)
        for k, (_, _, i) in enumerate(v[:Mb]):
            numbps[i], pieces[i] = Mb - k, [(int(rng.integers(0, L)), int(rng.integers(0, 40)), 1)]
    elif flavor == "lengths":
        # every length 1, 2^k - 1, 2^k the largest slot holds, one pass each, spread over the blocks and layers
        kmax = flog2(max(caps))
        want = sorted({1} | {(1 << k) - d for k in range(1, kmax + 1) for d in (0, 1)}, reverse=True)
        room, slots = list(caps), [list(range(L)) for _ in range(n)]
        numbps, pieces = [int(v) for v in fb[:, 9]], [[] for _ in range(n)]
        for ln in want:
            i = max((i for i in range(n) if slots[i]), key=lambda i: room[i])
            assert room[i] >= ln, "the case's blocks cannot hold every length"
            pieces[i].append((slots[i].pop(0), ln, 1))
            room[i] -= ln
        numbps = [nb if pc else 0 for nb, pc in zip(numbps, pieces)]
    elif flavor == "ffend":
        # one block, one leaf: every bit of the packet headers is known.  Layer 0: 1 (packet), 1 (included), 1 (no zero
        # bit-planes), 10 (two passes), 1111111 0 (Lblock 3 -> 10), 10011111111 (1279 bytes in 10 + 1 bits) = F7 F4 FF: the last
        # bit is the last bit of a 0xFF byte.  Layer 1: 1 (packet), 1 (included), 0 (one pass), 1 0 (Lblock 10 -> 11),
        # 10011111111 (1279 bytes) = D4 FF: again.  B.10.1 wants a byte behind either.
        assert n == 1 and caps[0] >= 2 * 1279
        numbps[0], pieces[0] = int(fb[0, 9]), [(0, 1279, 2), (1, 1279, 1)][:L]
    elif flavor == "over":
        # a block beyond the floor's bit-planes: `fb` was made at table_guard, one block takes its band's full count there
        i = int(np.argmax(fb[:, 9]))
        numbps[i], pieces[i] = int(fb[i, 9]), [(0, 17, 3 * int(fb[i, 9]) - 2)]
    for i in range(n):
        assert numbps[i] <= fb[i, 9] and sum(p[2] for p in pieces[i]) <= max(0, 3 * numbps[i] - 2) and sum(p[1] for p in pieces[i]) <= caps[i]
    data = [rng.integers(0, 0x90, sum(p[1] for p in pc), dtype=np.uint8).tobytes() for pc in pieces]  # below 0x90: no marker
    return dict(case=case, params=params, fb=fb, caps=caps, numbps=numbps, pieces=pieces, data=data, units=units, packet_of=block_geometry(case, fb)[0])


def _case(name, size, channels, depth, layers, seed, style=0, flavor="", deep=False, **mk):
    mk.setdefault("num_resolutions", 2)
    mk.setdefault("cblk", (4, 4))
    return dict(name=name, size=size, channels=channels, depth=depth, layers=layers, seed=seed, style=style, flavor=flavor, deep=deep, mk=mk)


PRC3 = [(32, 32), (16, 16), (8, 8)]  # highest resolution first: another precinct size at every resolution
GUARD_AUTO = 0x100

CASES = [
    _case("l1_17x9_grey8", (17, 9), 1, 8, 1, 101),
    _case("l2_33x21_rgb8_ycc", (33, 21), 3, 8, 2, 102, ycc=True, num_resolutions=3, cblk=(8, 4)),
    _case("l3_41x27_rgba12_97", (41, 27), 4, 12, 3, 103, reversible=False, num_resolutions=3, cblk=(8, 8)),
    _case("l4_67x45_grey10", (67, 45), 1, 10, 4, 104, num_resolutions=4, cblk=(16, 16)),
    _case("l5_29x31_rgb8_97_ycc", (29, 31), 3, 8, 5, 105, reversible=False, ycc=True, cblk=(4, 8)),
    _case("l6_53x19_rgba8", (53, 19), 4, 8, 6, 106, num_resolutions=3, cblk=(8, 4)),
    _case("l7_67x45_grey16_g7_deep", (67, 45), 1, 16, 7, 107, deep=True, guard_bits=7, cblk=(8, 4)),
    _case("l7_45x37_rgb12", (45, 37), 3, 12, 7, 108, num_resolutions=3, precincts=[(16, 16), (8, 8), (8, 8)]),
    _case("l2_67x45_grey16_g7_deep", (67, 45), 1, 16, 2, 109, deep=True, guard_bits=7, cblk=(8, 8)),
    _case("zbp_67x45_grey16_g7", (67, 45), 1, 16, 3, 110, flavor="zbp", guard_bits=7),
    _case("lblock_64x64_grey8", (64, 64), 1, 8, 3, 111, flavor="lblock", num_resolutions=1, cblk=(32, 32)),
    _case("lengths_67x45_rgba16", (67, 45), 4, 16, 7, 112, flavor="lengths", num_resolutions=1, cblk=(64, 64)),
    _case("empty_33x21_rgb8", (33, 21), 3, 8, 2, 113, flavor="empty", num_resolutions=3),
    _case("prec8_67x45_rgb8", (67, 45), 3, 8, 3, 114, num_resolutions=3, precincts=[(8, 8), (8, 8), (8, 8)]),
    _case("ffend_l1_32x32_grey8", (32, 32), 1, 8, 1, 115, flavor="ffend", num_resolutions=1, cblk=(32, 32)),
    _case("ffend_l2_32x32_grey8", (32, 32), 1, 8, 2, 116, flavor="ffend", num_resolutions=1, cblk=(32, 32)),
]
CASES += [_case("grid_%s_%s" % (g, p), GRIDS[g], 1, 8, 2, 200 + 10 * gi + pi, flavor="grid:" + p, num_resolutions=1)
          for gi, g in enumerate(GRIDS) for pi, p in enumerate(PATTERNS)]
CASES += [_case("style%d_l%d_%dx%d" % (st, L, w, h), (w, h), nc, 16, L, 300 + st + L, style=st, deep=True, guard_bits=5, num_resolutions=nr, cblk=cb)
          for st, L, (w, h), nc, nr, cb in ((4, 1, (33, 21), 1, 2, (8, 8)), (4, 3, (41, 27), 3, 2, (8, 4)), (1, 1, (33, 21), 1, 2, (8, 8)), (1, 4, (67, 45), 1, 3, (16, 8)),
                                         (5, 1, (29, 31), 3, 2, (8, 8)), (5, 3, (41, 27), 1, 2, (4, 4)), (55, 2, (33, 21), 1, 2, (8, 8)), (50, 2, (33, 21), 1, 2, (8, 8)))]
CASES += [_case("prog%d_67x45_rgb8_tile32" % pg, (67, 45), 3, 8, 2, 400 + pg, progression=pg, tile_size=32, num_resolutions=3, precincts=PRC3, cblk=(8, 8))
          for pg in range(5)]
WORKER_CASES = [_case("tile4096_l%d" % L, (256, 256), 1, 8, L, 500 + L, num_resolutions=3) for L in (1, 2)]
GUARD_CASE = dict(_case("over_33x21_rgb8_auto", (33, 21), 3, 8, 2, 601, flavor="over", guard_bits=GUARD_AUTO), table_guard=3)
GATHER_CASES = ("l1_17x9_grey8", "l7_45x37_rgb12", "style4_l3_41x27", "tile4096_l2")  # the GPU test's four plans


def case_named(name):
    return next(c for c in CASES + WORKER_CASES + [GUARD_CASE] if c["name"] == name)


def readback(api, table, cs):
    """The oracle's parse of an assembled codestream, in the table's block order: (numbps, pieces, data, reader's packet
    figures = (packet headers read, those whose bits end on a complete 0xFF byte))."""
    parsed = oracle().file_blocks(cs, layers=True)
    return table_from_reader(api, table["params"], cs, parsed) + ((parsed["packets"], parsed["headers_ending_on_ff"]),)


def assert_reads_back(api, table, cs):
    """The reader finds, for every block of the table: the same numbps, the same pieces per layer (bytes and passes), the same
    bytes; and no block the table does not have."""
    numbps, pieces, data, stats = readback(api, table, cs)
    for i, pc in enumerate(table["pieces"]):
        assert pieces[i] == pc, (table["case"]["name"], i, pc, pieces[i])
        assert data[i] == table["data"][i], (table["case"]["name"], i)
        if pc:
            assert numbps[i] == table["numbps"][i], (table["case"]["name"], i, table["numbps"][i], numbps[i])
    return stats


def packet_headers(plan):
    """The packet headers of a plan, one per header piece: SOT / SOD in front of a tile-part's first one taken off, the main
    header's piece and EOC's left out."""
    blob = plan["blob"].tobytes()
    out = []
    for d, s, ln in zip(*plan["headers"]):
        h = blob[int(s):int(s) + int(ln)]
        # (the main header by its place: a packet header may begin FF 4F; it cannot begin FF 90 or be FF D9 -- the byte behind a
        # 0xFF of a header has its top bit clear)
        if int(d) == 0 or h == b"\xff\xd9":
            continue
        if h[:2] == b"\xff\x90":
            h = h[14:]
        if h:
            out.append(h)
    return out


# -------------------------------------------------------------------------------------------------------------- census
def census(tables):
    """What the corpus reaches, from the block tables and the geometry alone (nothing of the planner's output)."""
    c = dict(b4_first=set(), b4_later=set(), max_passes=0, zero_len=0, lengths=set(), max_cap=0, lblock_packet=False, three_rises=0,
             grids=set(), zbp_full=0, zbp_Mb=0, max_Mb=0, layer_counts=set(), first_layers_of_7=set(), skip_middle=0, never=0, empty_frames=0,
             seg_termall=0, seg_bypass_1=0, seg_bypass_2=0, seg_both=0, boundary_in_segment=0, late_rise=set(), progressions=set(), blocks=0)
    rng_of = lambda n: next(k for k, (a, b) in enumerate(PASS_RANGES) if a <= n <= b)
    for t in tables:
        case, fb, L, style = t["case"], t["fb"], t["case"]["layers"], t["case"]["style"]
        c["layer_counts"].add(L)
        c["blocks"] += len(t["pieces"])
        c["max_cap"] = max(c["max_cap"], max(t["caps"]))
        c["max_Mb"] = max(c["max_Mb"], int(fb[:, 9].max()))
        if not any(t["pieces"]):
            c["empty_frames"] += 1
        if case["mk"].get("tile_size") and case["channels"] == 3 and case["mk"].get("precincts"):
            c["progressions"].add(case["mk"].get("progression", 0))
        steps = {}  # (packet, layer) -> Lblock steps of its blocks
        for i, pc in enumerate(t["pieces"]):
            if not pc:
                c["never"] += 1
                continue
            by_layer = {}
            for lay, ln, npass in pc:
                by_layer.setdefault(lay, []).append((ln, npass))
                c["lengths"].add(ln)
                c["zero_len"] += ln == 0
            lays = sorted(by_layer)
            if L == 7:
                c["first_layers_of_7"].add(lays[0])
            c["skip_middle"] += 0 in by_layer and 2 in by_layer and 1 not in by_layer  # layers 0 and 2, not 1
            lblock, rises, done = 3, 0, 0
            for lay in lays:
                npass = sum(p[1] for p in by_layer[lay])
                c["max_passes"] = max(c["max_passes"], npass)
                (c["b4_first"] if lay == lays[0] else c["b4_later"]).add(rng_of(npass))
                need = [max(1, ln.bit_length()) - (lblock + flog2(run)) for ln, run in by_layer[lay]]  # B.10.7.1
                step = max(0, max(need))
                if step and need[0] < step:
                    c["late_rise"].add(style & 5)
                lblock += step
                rises += step > 0
                steps.setdefault((t["case"]["name"],) + tuple(t["packet_of"][i]) + (lay,), set()).add(min(step, 8))
                if style & 5:
                    runs = [run for _, run in by_layer[lay]]
                    assert runs == layer_segments(style, done, npass)
                    if style & 4:
                        c["seg_both" if style & 1 else "seg_termall"] += len(runs) > 1
                    else:
                        tail = [(p, run) for p, run in zip(np.cumsum([done] + runs[:-1]).tolist(), runs) if p >= 10]
                        c["seg_bypass_1"] += any(run == 1 and p % 3 == 0 for p, run in tail)
                        c["seg_bypass_2"] += any(run == 2 for p, run in tail)
                        # the layer ends inside a segment: its last pass does not terminate one, and the block goes on
                        if not pass_terminates(style, done + npass - 1) and lay != lays[-1]:
                            c["boundary_in_segment"] += 1
                done += npass
            c["three_rises"] += rises >= 3
        c["lblock_packet"] = c["lblock_packet"] or any({0, 1, 8} <= s for s in steps.values())
        for (key, v) in t["units"].items():
            cw, ch = 1 + max(a[0] for a in v), 1 + max(a[1] for a in v)
            assert len(v) == cw * ch
            g = "1x1" if (cw, ch) == (1, 1) else "1xn" if cw == 1 else "nx1" if ch == 1 else "2x2" if (cw, ch) == (2, 2) else \
                "3x5" if (cw, ch) == (3, 5) else "16+" if min(cw, ch) >= 16 else None
            first0 = {(x, y) for x, y, i in v if t["pieces"][i] and t["pieces"][i][0][0] == 0}
            every = {(x, y) for x, y, _ in v}
            pat = "all" if first0 == every else "none" if not first0 else "corner" if len(first0) == 1 and first0 <= {(0, 0), (cw - 1, 0), (0, ch - 1), (cw - 1, ch - 1)} else \
                "checker" if first0 == {a for a in every if sum(a) % 2 == 0} else None
            if g and pat:
                c["grids"].add((g, pat))
            Mb = int(fb[v[0][2], 9])
            zb = {Mb - t["numbps"][i] for _, _, i in v if t["pieces"][i]}
            if zb >= set(range(Mb)) and Mb >= c["zbp_Mb"]:
                c["zbp_Mb"], c["zbp_full"] = Mb, c["zbp_full"] + 1
    return c
