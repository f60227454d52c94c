"""Files cut short: one case generator for the CPU tier (test_decode_cut_refs.py) and the GPU tier (test_decode_cut.py).

Pure Python plus the plain-C oracle: no reference program runs here and no device.  A case is a committed fixture cut at an
offset found by walking the SOT / Psot chain (never by searching for `ff 90`), optionally with an EOC appended:

 (a) boundary cuts: the first k tile-parts, k in {1, n / 2, n - 1}, with `ff d9` appended and bare; the whole file without its
     EOC and with half of it;
 (b) directed cuts inside the first and the last tile-part: inside the SOT segment (sot + 5, sot + 11), just after SOD, one
     byte later, and at 1/7 .. 6/7 of the tile-part's packet bytes;
 (c) 8 seeded random cuts over the packet range of the whole file.

The oracle decides whether a case decodes or is refused.  For the files it does not read only the (a) cuts with an EOC are
generated: libopenjp2 2.4.0 and 2.5.4 decode those (and refuse every cut inside a tile-part), their per-component hashes are
committed in tests/golden/cut/cut.json (make_cut_golden.py).

The PPT / PPM repacks of the SOP + EPH fixture (test_read_fallback._repack_headers) have all packet headers ahead of the
bodies, and the oracle does not read them.  A cut inside packet k's body there keeps exactly what the original keeps when cut
the same number of bytes into the same packet's body (packets before k whole, packet k's header whole): `twin` is that cut of
the original, and its decode is the reference."""
import json
import os

import numpy as np

from conftest import GOLDEN_DIR

SEED = 20261  # (c): the random cuts
SOP4 = b"\xff\x91\x00\x04"
EOC = b"\xff\xd9"

# tag -> path under tests/golden
ORACLE_FILES = {
    "g1": "g1_64x64_grey_5lvl.j2k",
    "g9": "g9_150x130_rgb8_97_tile64.j2k",
    "g4": "g4_300x200_rgb16_53_rct_tile128.j2k",
    "o3": "o3_200x300_rgba16_53_tile128_2layers_pcrl.j2k",
    "r8": "r8_300x200_rgba8_53_rct_7layers.j2k",
    "l1": "layers/l1_128_grey8_53_lrcp_4layers.j2k",
    "l2": "layers/l2_97x61_rgb8_97_ict_rlcp_5layers.j2k",
    "l4": "layers/l4_128_grey16_53_bypass_lrcp_4layers.j2k",
    "l5": "layers/l5_97x61_grey12_97_termall_vcausal_segsym_cprl_3layers.j2k",
    "s1": "ext/s1_300x200_rgb16_53_bypass.j2k",
    "s4": "ext/s4_300x200_rgb16_97_all_styles_2layers_tile128.j2k",
    "u7": "ext/u7_128_grey8_53_bypass_termall.j2k",
    "u8": "ext/u8_300x200_rgb8_53_sop_eph_pcrl_precincts.j2k",
    "u9": "ext/u9_256_rgb8_53_precincts_lrcp_tile100.j2k",
    "k1": "ext/k1_67x45_rgb8_53_pcrl_prec8_cblk4.j2k",
}
REPACKS = {"u8_ppt": ("u8", "ppt"), "u8_ppm": ("u8", "ppm")}
# boundary cuts with an EOC only; the reference is libopenjp2 (committed hashes, the live library where there is one)
OPJ_FILES = {
    "u2": "ext/u2_301x199_ycc422_10_97_tile128.j2k",
    "d1": "ext/d1_512x270_rgb12_cinema2k.j2k",
    "d2": "ext/d2_1024x540_rgb12_cinema4k_poc.j2k",
    "m2": "ext/m2_150x130_5comp12_97_tile64_2layers.j2k",
    # crafted: the multi-tile lossless file with every component declared signed (SIZ Ssiz bit 7), so that a missing tile's 0
    # meets the signed offset of the output stage
    "g4s": "g4_300x200_rgb16_53_rct_tile128.j2k#signed",
}
STYLED = ("l4", "l5", "s4", "u7")  # multi-segment code-block styles, layers: both Tier-1 kernels' ground
TAGS = list(ORACLE_FILES) + list(REPACKS) + list(OPJ_FILES)

_cache = {}


def load(tag: str) -> bytes:
    if tag not in _cache:
        if tag in REPACKS:
            import test_read_fallback as rf
            src, where = REPACKS[tag]
            _cache[tag] = rf._repack_headers(load(src), where)
        else:
            path, _, craft = {**ORACLE_FILES, **OPJ_FILES}[tag].partition("#")
            with open(os.path.join(GOLDEN_DIR, path), "rb") as f:
                data = bytearray(f.read())
            if craft == "signed":  # SIZ: marker at 2, Csiz at 40, then Ssiz, XRsiz, YRsiz per component
                for c in range(be(data[40:42])):
                    data[42 + 3 * c] |= 0x80
            _cache[tag] = bytes(data)
    return _cache[tag]


def be(b: bytes) -> int:
    return int.from_bytes(b, "big")


def walk(data: bytes) -> dict:
    """The raw codestream's structure by its own lengths: dict(first_sot, ntiles, tile_w .. , parts = [dict(sot, tile, sod =
    offset of the first packet byte, end)])."""
    assert data[:2] == b"\xff\x4f" and data[2:4] == b"\xff\x51"
    siz = 4
    x1, y1, x0, y0, tw, th, tx0, ty0 = (be(data[siz + 4 + 4 * i:siz + 8 + 4 * i]) for i in range(8))
    ntx, nty = -(-(x1 - tx0) // tw), -(-(y1 - ty0) // th)
    pos = 2
    while data[pos:pos + 2] != b"\xff\x90":
        assert data[pos] == 0xff, pos
        pos += 2 + be(data[pos + 2:pos + 4])
    first_sot, parts = pos, []
    while data[pos:pos + 2] == b"\xff\x90":
        tile, psot = be(data[pos + 4:pos + 6]), be(data[pos + 6:pos + 10])
        end = pos + psot if psot else len(data) - (2 if data[-2:] == EOC else 0)
        q = pos + 12
        while data[q:q + 2] != b"\xff\x93":
            assert data[q] == 0xff and q < end, q
            q += 2 + be(data[q + 2:q + 4])
        parts.append(dict(sot=pos, tile=tile, sod=q + 2, end=end))
        pos = end
    assert data[pos:] == EOC, "the fixture ends with its EOC"
    return dict(first_sot=first_sot, ntiles=ntx * nty, ntx=ntx, nty=nty, origin=(x0, y0), size=(x1 - x0, y1 - y0), tile=(tw, th),
                tile_origin=(tx0, ty0), parts=parts)


def tile_rect(w: dict, tile: int, reduce: int = 0, sub=(1, 1)):
    """(x0, y0, x1, y1) of the tile's samples in a component's delivered plane at `reduce`."""
    def cdiv(a, b):
        return -(-a // b)
    p, q = tile % w["ntx"], tile // w["ntx"]
    ox, oy = w["origin"]
    ex, ey = ox + w["size"][0], oy + w["size"][1]
    tx0, ty0 = max(w["tile_origin"][0] + p * w["tile"][0], ox), max(w["tile_origin"][1] + q * w["tile"][1], oy)
    tx1, ty1 = min(w["tile_origin"][0] + (p + 1) * w["tile"][0], ex), min(w["tile_origin"][1] + (q + 1) * w["tile"][1], ey)
    f = 1 << reduce
    cx = lambda v: cdiv(cdiv(v, sub[0]), f)
    cy = lambda v: cdiv(cdiv(v, sub[1]), f)
    return cx(tx0) - cx(ox), cy(ty0) - cy(oy), cx(tx1) - cx(ox), cy(ty1) - cy(oy)


def missing_tiles(tag: str, case: dict) -> list:
    """Tiles of which no tile-part (not even its SOT .. SOD) lies inside the cut."""
    w = walk(load(tag))
    have = {p["tile"] for p in w["parts"] if p["sod"] <= case["end"]}
    return [t for t in range(w["ntiles"]) if t not in have]


def _packets(data: bytes, part: dict) -> list:
    """A SOP + EPH tile-part's packets: (sop, header start, body start, end).  Neither codeword bytes nor packet-header bytes
    hold a marker above ff 8f, so the two are found by search inside the tile-part."""
    out, pos = [], part["sod"]
    while pos < part["end"]:
        assert data[pos:pos + 4] == SOP4, pos
        eph = data.index(b"\xff\x92", pos + 6, part["end"])
        nxt = data.find(SOP4, eph + 2, part["end"])
        nxt = part["end"] if nxt < 0 else nxt
        out.append((pos, pos + 6, eph + 2, nxt))
        pos = nxt
    return out


def _case(tag, kind, label, end, eoc=False, twin=None):
    return dict(tag=tag, kind=kind, label=label, end=end, eoc=eoc, twin=twin, id=f"{tag}-{kind}-{label}")


def cut_bytes(case: dict) -> bytes:
    return load(case["tag"])[:case["end"]] + (EOC if case["eoc"] else b"")


def reference_bytes(case: dict) -> bytes:
    """The bytes the oracle is given for this case: the case's own, or its twin's for a repack."""
    return cut_bytes(case["twin"]) if case["twin"] else cut_bytes(case)


def _boundary(tag, w, data, only_eoc=False):
    n, out = len(w["parts"]), []
    for k in sorted({1, n // 2, n - 1}):
        if not 1 <= k < n:
            continue
        out.append(_case(tag, "a", f"parts{k}of{n}+eoc", w["parts"][k - 1]["end"], eoc=True))
        if not only_eoc:
            out.append(_case(tag, "a", f"parts{k}of{n}", w["parts"][k - 1]["end"]))
    if not only_eoc:
        out.append(_case(tag, "a", "len-2", len(data) - 2))
        out.append(_case(tag, "a", "len-1", len(data) - 1))
    return out


def _repack_cases(tag):
    """Cuts of a PPT / PPM repack inside packet bodies, each with its twin cut of the original."""
    src = REPACKS[tag][0]
    data, orig = load(tag), load(src)
    w, wo = walk(data), walk(orig)
    assert len(w["parts"]) == 1 and len(wo["parts"]) == 1
    pk = _packets(orig, wo["parts"][0])
    # the repack's packet bytes: SOP, body, SOP, body ... (the headers and their EPH left)
    starts, pos = [], w["parts"][0]["sod"]
    for sop, hdr, body, end in pk:
        assert data[pos:pos + 6] == orig[sop:sop + 6] and data[pos + 6:pos + 6 + end - body] == orig[body:end]
        starts.append(pos + 6)
        pos += 6 + end - body
    assert pos == w["parts"][0]["end"]
    rng = np.random.default_rng(SEED + TAGS.index(tag))
    out = [_case(tag, "a", "len-2", len(data) - 2, twin=_case(src, "a", "len-2", len(orig) - 2))]
    with_body = [k for k, p in enumerate(pk) if p[3] - p[2] >= 2]
    picks = [with_body[0], with_body[len(with_body) // 2], with_body[-1]] + [int(k) for k in rng.choice(with_body, 8)]
    for i, k in enumerate(picks):
        n = pk[k][3] - pk[k][2]
        j = int(rng.integers(1, n))
        out.append(_case(tag, "b" if i < 3 else "c", f"packet{k}+{j}of{n}", starts[k] + j, twin=_case(src, "b", f"packet{k}+{j}of{n}", pk[k][2] + j)))
    return out


def cases(tag: str) -> list:
    if ("cases", tag) in _cache:
        return _cache[("cases", tag)]
    if tag in REPACKS:
        out = _repack_cases(tag)
    else:
        data = load(tag)
        w = walk(data)
        out = _boundary(tag, w, data, only_eoc=tag in OPJ_FILES)
        if tag in ORACLE_FILES:
            ends = []
            for which, p in (("first", w["parts"][0]), ("last", w["parts"][-1]))[:2 if len(w["parts"]) > 1 else 1]:
                n = p["end"] - p["sod"]
                ends += [(f"{which}-sot+5", p["sot"] + 5), (f"{which}-sot+11", p["sot"] + 11), (f"{which}-sod", p["sod"]), (f"{which}-sod+1", p["sod"] + 1)]
                ends += [(f"{which}-{i}of7", p["sod"] + i * n // 7) for i in range(1, 7)]
                if data[p["sod"]:p["sod"] + 4] == SOP4 and b"\xff\x92" in data[p["sod"]:p["end"]]:
                    # SOP + EPH show where packet headers lie (they are short, and the cuts above fall into bodies): one byte
                    # into the first packet's header, and the middle of the longest header
                    pk = _packets(data, p)
                    sop, hdr, body, end = max(pk, key=lambda k: k[2] - k[1])
                    ends += [(f"{which}-hdr+1", pk[0][1] + 1), (f"{which}-hdr-mid", hdr + (body - 2 - hdr) // 2 + 1)]
            out += [_case(tag, "b", label, end) for label, end in ends]
            rng = np.random.default_rng(SEED + TAGS.index(tag))
            lo, hi = w["parts"][0]["sod"], w["parts"][-1]["end"]
            out += [_case(tag, "c", f"at{int(e)}", int(e)) for e in sorted(rng.integers(lo + 1, hi, 8))]
    assert len({c["id"] for c in out}) == len(out)
    _cache[("cases", tag)] = out
    return out


def all_cases() -> list:
    return [c for tag in TAGS for c in cases(tag)]


def decodes(oracle, case: dict) -> bool:
    """The oracle's verdict on a case it reads (memoised: several tests ask)."""
    key = ("ok", case["id"])
    if key not in _cache:
        try:
            oracle.decode_info(reference_bytes(case))
            oracle.file_blocks(reference_bytes(case))
            _cache[key] = True
        except RuntimeError:
            _cache[key] = False
    return _cache[key]


def expected(oracle, case: dict, reduce: int = 0) -> np.ndarray:
    """The oracle's decode of a case that decodes, (ncomp, h, w) int32; computed once and handed out read-only."""
    key = ("dec", case["id"], reduce)
    if key not in _cache:
        a = oracle.decode(reference_bytes(case), reduce)
        a.setflags(write=False)
        _cache[key] = a
    return _cache[key]


def normalise(segs, npasses: int, nbytes: int) -> list:
    """A block's codeword segment table as both sides must agree on it: the leading segments until their passes reach the
    block's passes (a header may have promised passes whose bodies never arrived), each length clipped to the block's bytes
    left at its offset (decode_plan.h: cwseg_have)."""
    out, at, seen = [], 0, 0
    for ln, np_ in segs:
        if seen >= npasses:
            break
        out.append((min(ln, nbytes - at) if at < nbytes else 0, np_))
        at += ln
        seen += np_
    return out


def golden() -> dict:
    with open(os.path.join(GOLDEN_DIR, "cut", "cut.json")) as f:
        return json.load(f)
