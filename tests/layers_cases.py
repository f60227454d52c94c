"""Quality-layer fixtures (tests/golden/layers, written by tests/golden/make_layers_golden.py) and the reference of a decode
with a layer limit: strip(cs, L), the codestream that holds only the first L layers.

The files are written with SOP markers, so every packet starts at FF 91 00 04 (neither packet headers nor codeword bytes
can hold a marker above FF8F) and the layer of packet k of a tile-part follows from the progression order alone.
strip(cs, L) removes the packets of layers >= L, sets COD's layer count to L, renumbers Nsop and fixes Psot; a decode of
the ORIGINAL file with the limit L must deliver exactly the decode of strip(cs, L).  drop_sop(cs) is the same file without
its SOP segments (Scod bit 1 cleared): what the decoder has to do without the markers this module leans on.
"""
from __future__ import annotations

import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "layers")

LRCP, RLCP, RPCL, PCRL, CPRL = range(5)

# name -> (width, height, ncomp, prec, seed, dist, OpjReplay.encode_ext kwargs); every file is written with sop=True and one
# compression ratio per layer (0 = everything that is left: lossless under 5/3).  "sub" (l6): the chroma planes are the
# generator's planes taken at every second sample.
CASES = {
    "l1_128_grey8_53_lrcp_4layers": (128, 128, 1, 8, 301, "A", dict(numres=3, cblk=(32, 32), prog=LRCP, rates=[24.0, 10.0, 4.0, 0.0])),
    "l2_97x61_rgb8_97_ict_rlcp_5layers": (97, 61, 3, 8, 302, "A", dict(numres=3, mct=True, reversible=False, prog=RLCP,
                                                                      rates=[60.0, 30.0, 15.0, 8.0, 4.0])),
    "l3_150x130_rgb10_53_rct_tile64_prec32_rpcl_3layers": (150, 130, 3, 10, 303, "A", dict(numres=3, mct=True, tile=(64, 64), precincts=[(32, 32)],
                                                                                          prog=RPCL, rates=[30.0, 10.0, 0.0])),
    "l4_128_grey16_53_bypass_lrcp_4layers": (128, 128, 1, 16, 304, "A", dict(numres=2, mode=1, prog=LRCP, rates=[20.0, 8.0, 3.0, 0.0])),
    "l5_97x61_grey12_97_termall_vcausal_segsym_cprl_3layers": (97, 61, 1, 12, 305, "A", dict(numres=3, reversible=False, mode=4 | 8 | 32, prog=CPRL,
                                                                                            rates=[30.0, 12.0, 5.0])),
    "l6_97x61_ycc420_8_53_pcrl_3layers": (97, 61, 3, 8, 306, "A", dict(numres=3, prog=PCRL, sub=[(1, 1), (2, 2), (2, 2)], rates=[20.0, 8.0, 0.0])),
    # l1 with EPH markers as well: the one file whose packet headers tests/test_read_fallback.py: _repack_headers can move into PPT / PPM
    "l7_128_grey8_53_lrcp_4layers_eph": (128, 128, 1, 8, 301, "A", dict(numres=3, cblk=(32, 32), prog=LRCP, eph=True, rates=[24.0, 10.0, 4.0, 0.0])),
}
NAMES = list(CASES)
SOP = b"\xff\x91\x00\x04"


def layers_of(name: str) -> int:
    return len(CASES[name][6]["rates"])


def styled(name: str) -> bool:
    return CASES[name][6].get("mode", 0) != 0


def load(name: str) -> bytes:
    with open(os.path.join(GOLDEN, name + ".j2k"), "rb") as f:
        return f.read()


_meta = None


def meta() -> dict:
    global _meta
    if _meta is None:
        with open(os.path.join(GOLDEN, "layers.json")) as f:
            _meta = json.load(f)
    return _meta


def _main_header(cs: bytes) -> dict:
    """Offsets of COD and of the first SOT, and what COD / SIZ say."""
    assert cs[:2] == b"\xff\x4f"
    pos, out = 2, {}
    while cs[pos:pos + 2] != b"\xff\x90":
        m, ln = cs[pos:pos + 2], int.from_bytes(cs[pos + 2:pos + 4], "big")
        if m == b"\xff\x51":
            out["ncomp"] = int.from_bytes(cs[pos + 38:pos + 40], "big")
        elif m == b"\xff\x52":
            out.update(cod=pos, scod=cs[pos + 4], prog=cs[pos + 5], layers=int.from_bytes(cs[pos + 6:pos + 8], "big"))
        assert m not in (b"\xff\x55", b"\xff\x57", b"\xff\x60", b"\xff\x5f"), "TLM / PLM / PPM / POC: not what this helper rewrites"
        pos += 2 + ln
    out["sot"] = pos
    return out


def _tile_parts(cs: bytes, first_sot: int):
    """(sot, sod + 2, end) of every tile-part, then the offset of what follows the last (EOC)."""
    parts, pos = [], first_sot
    while cs[pos:pos + 2] == b"\xff\x90":
        psot = int.from_bytes(cs[pos + 6:pos + 10], "big")
        assert psot and cs[pos + 10] == 0 and cs[pos + 11] == 1, "one tile-part per tile"
        sod = cs.index(b"\xff\x93", pos + 12)
        assert sod == pos + 12, "a tile-part header without marker segments"
        parts.append((pos, sod + 2, pos + psot))
        pos += psot
    assert cs[pos:] == b"\xff\xd9"
    return parts, pos


def _packets(body: bytes) -> list:
    """The packets of a tile-part's body, each beginning with its SOP segment."""
    assert body[:4] == SOP
    starts = []
    pos = 0
    while pos >= 0:
        starts.append(pos)
        pos = body.find(SOP, pos + 6)
    return [body[a:b] for a, b in zip(starts, starts[1:] + [len(body)])]


def packet_layer(k: int, n: int, prog: int, layers: int, ncomp: int) -> int:
    """Layer of packet k of the n packets of a tile-part (RLCP: with maximal precincts, one per resolution and component)."""
    assert n % layers == 0
    if prog == LRCP:
        return k // (n // layers)
    if prog == RLCP:
        return (k // ncomp) % layers
    return k % layers


def strip(cs: bytes, keep: int) -> bytes:
    """The codestream with the first `keep` layers only."""
    h = _main_header(cs)
    assert h["scod"] & 2, "written with SOP markers"
    assert 1 <= keep <= h["layers"]
    parts, eoc = _tile_parts(cs, h["sot"])
    out = bytearray(cs[:h["sot"]])
    out[h["cod"] + 6:h["cod"] + 8] = keep.to_bytes(2, "big")
    for sot, body0, end in parts:
        pk = _packets(cs[body0:end])
        kept = [p for k, p in enumerate(pk) if packet_layer(k, len(pk), h["prog"], h["layers"], h["ncomp"]) < keep]
        assert len(kept) * h["layers"] == len(pk) * keep
        body = b"".join(p[:4] + (i & 0xffff).to_bytes(2, "big") + p[6:] for i, p in enumerate(kept))
        psot = body0 - sot + len(body)
        out += cs[sot:sot + 6] + psot.to_bytes(4, "big") + cs[sot + 10:body0] + body
    return bytes(out + cs[eoc:])


def drop_sop(cs: bytes) -> bytes:
    """The same codestream without its SOP segments."""
    h = _main_header(cs)
    assert h["scod"] & 2
    parts, eoc = _tile_parts(cs, h["sot"])
    out = bytearray(cs[:h["sot"]])
    out[h["cod"] + 4] = h["scod"] & ~2
    for sot, body0, end in parts:
        body = b"".join(p[6:] for p in _packets(cs[body0:end]))
        psot = body0 - sot + len(body)
        out += cs[sot:sot + 6] + psot.to_bytes(4, "big") + cs[sot + 10:body0] + body
    return bytes(out + cs[eoc:])


def packets_per_tile_part(cs: bytes) -> list:
    h = _main_header(cs)
    return [len(_packets(cs[b:e])) for _, b, e in _tile_parts(cs, h["sot"])[0]]
