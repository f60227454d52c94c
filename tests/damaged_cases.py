"""Damaged code-block bytes for the Tier-1 decoders (test_t1_dec_damaged_blocks.py on the GPU, test_t1_dec_damaged_refs.py on
the CPU) and damaged whole files (tests/golden/damaged, test_decode_damaged.py).  Plain helpers: no fixtures, no tests.

For arbitrary bytes the MQ decoder is still a total function (T.800 C.3.4): behind a 0xFF a byte above 0x8F is a marker --
nothing more is consumed, 1-bits follow -- and a byte up to 0x8F gives seven bits.  damage() writes such bytes into a
codeword; lengths, pass counts, bit-plane counts and segment tables stay those of the clean case, so a decoder reads what
it reads of the clean one.  A position `at` is the index of the FIRST byte a mode writes: for the pairs (marker, ff8f) the
index of the 0xFF, so that positions 3, 63, 255 and 511 put the 0xFF last in a dword, in the lane decoder's 64-byte ring
and in the wave decoder's 256-byte window, and the byte behind it first in the next.
"""
import json
import os
import zlib

import numpy as np

import decode_stage_cases as dsc
import layers_cases as lc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "damaged")

MARKER_BYTES = (0x90, 0xC3, 0xFF)
PLACED = ("flip", "marker", "ff8f", "ff_run")                          # modes that take a position
UNPLACED = ("ff_tail", "ff7f_tail", "all_ff", "all_00", "random")      # modes that do not
MODES = PLACED + UNPLACED


def damage(data, mode, at=None, byte=0x90):
    """data with the damage of `mode`; a function of its arguments alone.  flip: bit at % 8 of byte at; marker: FF `byte`
    at at, at + 1; ff8f: FF 8F; ff_run: FF FF FF; ff_tail: the last byte FF; ff7f_tail: the last two FF 7F; all_ff, all_00;
    random: every byte (seeded by the bytes themselves and `at`)."""
    d = bytearray(data)
    n = len(d)
    if mode in PLACED:
        width = {"flip": 1, "marker": 2, "ff8f": 2, "ff_run": 3}[mode]
        assert at is not None and 0 <= at and at + width <= n, (mode, at, n)
    if mode == "flip":
        d[at] ^= 1 << (at % 8)
    elif mode == "marker":
        assert byte > 0x8F
        d[at:at + 2] = bytes([0xFF, byte])
    elif mode == "ff8f":
        d[at:at + 2] = b"\xff\x8f"
    elif mode == "ff_run":
        d[at:at + 3] = b"\xff\xff\xff"
    elif mode == "ff_tail":
        assert n >= 1
        d[-1] = 0xFF
    elif mode == "ff7f_tail":
        assert n >= 2
        d[-2:] = b"\xff\x7f"
    elif mode == "all_ff":
        d[:] = b"\xff" * n
    elif mode == "all_00":
        d[:] = bytes(n)
    elif mode == "random":
        d[:] = np.random.default_rng([zlib.crc32(bytes(data)), n, at or 0]).integers(0, 256, size=n, dtype=np.uint8).tobytes()
    else:
        raise ValueError(mode)
    return bytes(d)


def positions(length):
    """The position set of a codeword of `length` bytes: the dword edges, fractions of the length, the edges of the lane
    ring's 64 bytes and of the wave kernel's 256-byte window, the codeword's end; those at which a pair of bytes fits."""
    cand = [1, 2, 3, 4, length // 8, length // 4, 63, 64, 255, 256, 511, 512, length // 2, length - 3, length - 2]
    return sorted({p for p in cand if 1 <= p <= length - 2})  # (a pair fits; ff_run needs a byte more: placed_modes)


def placed_modes(at, length):
    """(mode, byte) of every placed damage that fits at `at`."""
    out = [("flip", None)] + [("marker", b) for b in MARKER_BYTES] + [("ff8f", None)]
    if at + 3 <= length:
        out.append(("ff_run", None))
    return out


_blocks = {}


def blocks(oracle, rev):
    """[(name, case)]: the five blocks of decode_stage_cases.subset_blocks under this transform (as test_decode_stages.py
    codes them), then the 9 KB stream."""
    if rev not in _blocks:
        out = [(n, dsc.code_block(oracle, b, o, rev)) for n, b, o in dsc.subset_blocks(np.random.default_rng(1357 + int(rev)))]
        out.append(("long-stream", dsc.code_scaled(oracle, dsc.long_stream_block(np.random.default_rng(4242)), 0)))
        _blocks[rev] = out
    return _blocks[rev]


def codewords(oracle):
    """The eleven codewords: five blocks by two transforms, and the long stream (the same bytes under either)."""
    return [(f"{n}-rev", True, c) for n, c in blocks(oracle, True)[:5]] + [(f"{n}-irr", False, c) for n, c in blocks(oracle, False)]


def mode_cases(oracle, rev, mode):
    """Every block of blocks(rev) under one mode: a placed mode at every position of the block's set (marker: with each of
    the three bytes), the others once.  -> [(block name, at, byte, case)]"""
    out = []
    for name, c in blocks(oracle, rev):
        n = len(c["data"])
        if mode in UNPLACED:
            out.append((name, None, None, dsc.variant(c, data=damage(c["data"], mode))))
            continue
        for at in positions(n):
            for m, b in placed_modes(at, n):
                if m == mode:
                    out.append((name, at, b, dsc.variant(c, data=damage(c["data"], mode, at, b or 0x90))))
    return out


def window_edge_cases(oracle):
    """The long stream with a marker across every edge of the wave kernel's 256-byte window up to 4096: the 0xFF last in one
    window, the marker byte first in the next."""
    c = blocks(oracle, True)[-1][1]
    assert len(c["data"]) > 4096 + 2
    return [dsc.variant(c, data=damage(c["data"], "marker", 256 * k - 1, MARKER_BYTES[k % 3]), orient=k % 4) for k in range(1, 17)]


def cut_cases(oracle, rev):
    """Damaged and cut: a marker inside the bytes of the first pass, with 1, 4 and npasses - 1 passes kept -- the bytes cut
    at the coder's rate of the last kept pass, and all bytes kept.  -> [(clean case with p passes, damaged case)]"""
    out = []
    for name, c in blocks(oracle, rev):
        at = max(1, min(c["rates"][0], len(c["data"]) - 2) // 2)
        d = damage(c["data"], "marker", at, MARKER_BYTES[len(out) % 3])
        for p in (1, 4, c["npasses"] - 1):
            nb = c["rates"][p - 1]
            if at + 2 <= nb:
                out.append((dsc.variant(c, npasses=p, data=c["data"][:nb]), dsc.variant(c, npasses=p, data=d[:nb])))
            out.append((dsc.variant(c, npasses=p), dsc.variant(c, npasses=p, data=d)))
    return out


def behind_cases(oracle, rev):
    """A marker placed behind the bytes of the kept passes (1, 4, npasses - 1 of them; all of the codeword's bytes present):
    it must not matter.  -> [(clean case with p passes, damaged case)]; blocks whose kept passes reach the end are left out."""
    out = []
    for name, c in blocks(oracle, rev):
        n = len(c["data"])
        for p in (1, 4, c["npasses"] - 1):
            at = c["rates"][p - 1]
            if at + 2 <= n:
                out.append((dsc.variant(c, npasses=p), dsc.variant(c, npasses=p, data=damage(c["data"], "marker", at, MARKER_BYTES[len(out) % 3]))))
    return out


def unlike_wave(oracle, rev):
    """64 blocks for one wave of the lane kernel: the long stream in lane 0, clean and damaged copies of the five blocks in
    turn -- the damaged ones with a marker each at another depth of its position set, so that a lane whose decoder stands
    still on a marker runs beside lanes that advance and refill --, the long stream again with a marker at 511, and a 1 x 1
    block in the last lane."""
    bl = blocks(oracle, rev)
    long_ = bl[-1][1]
    cases = [long_, dsc.variant(long_, data=damage(long_["data"], "marker", 511, 0xFF))]
    k = 0
    while len(cases) < 63:
        c = bl[k % 5][1]
        if len(cases) % 2 == 0:
            cases.append(c)
        else:
            ps = positions(len(c["data"]))
            cases.append(dsc.variant(c, data=damage(c["data"], "marker", ps[(k // 5 * 3 + k) % len(ps)], MARKER_BYTES[k % 3])))
            k += 1
    one = dsc.code_block(oracle, np.array([[-1234]]), 0, rev)
    assert (one["w"], one["h"]) == (1, 1) and one["npasses"] >= 4
    cases.append(one)
    return cases


# ------------------------------------------------------------------------------------------------ whole files
# name -> (width, height, ncomp, prec, seed, dist, OpjReplay.encode_ext kwargs); every file is written with sop=True, eph=True
FILES = {
    "d1_97x61_grey8_53": (97, 61, 1, 8, 401, "A", dict(numres=3)),
    "d2_65x33_rgb8_97_ict": (65, 33, 3, 8, 402, "B", dict(numres=3, mct=True, reversible=False)),
    "d3_65x33_grey16_53_bypass": (65, 33, 1, 16, 403, "A", dict(numres=3, mode=1)),
    "d4_97x61_grey12_97_bypass_termall": (97, 61, 1, 12, 404, "B", dict(numres=3, mode=1 | 4, reversible=False)),
    "d5_33x17_rgb16_53_rct_vcausal_segsym_cblk16": (33, 17, 3, 16, 405, "A", dict(numres=2, mct=True, mode=8 | 32, cblk=(16, 16))),
    "d6_128x64_grey8_53_termall_3layers_tile64": (128, 64, 1, 8, 406, "A", dict(numres=3, mode=4, tile=(64, 64), rates=[20.0, 6.0, 0.0])),
}
FILE_NAMES = list(FILES)
FILE_MODES = ("flip", "marker", "ff_run", "random")
LAYERED, TILED = "d6_128x64_grey8_53_termall_3layers_tile64", "d6_128x64_grey8_53_termall_3layers_tile64"
SOP, EPH = b"\xff\x91\x00\x04", b"\xff\x92"


def styled(name):
    return FILES[name][6].get("mode", 0) != 0


def packet_bodies(cs):
    """[(begin, end)] of every packet body: the bytes between a packet's EPH and the next SOP, or the end of its tile-part.
    (Neither a packet header nor a conforming body holds FF 90 or above, so the first EPH behind a SOP is the packet's.)"""
    parts, _ = lc._tile_parts(cs, lc._main_header(cs)["sot"])
    out = []
    for _, body0, end in parts:
        pos = body0
        assert cs[pos:pos + 4] == SOP
        while pos < end:
            eph = cs.index(EPH, pos + 6, end)
            nxt = cs.find(SOP, eph + 2, end)
            nxt = end if nxt < 0 else nxt
            out.append((eph + 2, nxt))
            pos = nxt
    return out


def load(name):
    with open(os.path.join(GOLDEN, name + ".j2k"), "rb") as f:
        return f.read()


_meta = None


def meta():
    global _meta
    if _meta is None:
        with open(os.path.join(GOLDEN, "damaged.json")) as f:
            _meta = json.load(f)
    return _meta


def patched(name, mode):
    """The file with the committed patch list of `mode` applied."""
    d = bytearray(load(name))
    for off, b in meta()[name]["modes"][mode]["patch"]:
        d[off] = b
    return bytes(d)


def hashes(name, mode=None):
    """{reduce: [sha256 per component]} of libopenjp2's decode: of the clean file, or of the file damaged by `mode`."""
    m = meta()[name]
    src = m["decoded"] if mode is None else m["modes"][mode]["decoded"]
    return {int(r): list(v) for r, v in src.items()}
