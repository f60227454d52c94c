"""Cases of the block-level tests of the Tier-1 DECODER under code-block styles (test_t1_dec_styled_blocks.py on the GPU
through j2k_hip_stage_t1_decode_styled, test_t1_lane_styled_host.py on the CPU through the lane decoder's host program,
test_t1_dec_styled_refs.py for what the references must meet).  Plain helpers: no fixtures, no tests.

A case is a dict as in decode_stage_cases.py -- w, h, orient, numbps, npasses, data, half_step, roishift -- plus segs, the
block's codeword segments [(bytes, passes), ...] under bypass or termall (empty otherwise).  A batch is (reversible,
style, cases): one call of the hook.  A group is a list of batches with a name; the GPU test and the host program run the
same groups (GROUP_NAMES, group()).  What a decode must leave always comes from the oracle's styled block decoder
(j2ko_t1_decode_block_styled) on the same bytes and the same segment table.

Codewords come from the oracle's styled ENCODER (byte-pinned to libopenjp2): the blocks of t1_styled_families.py, which
meet the rare byte patterns (a raw segment ending in 0xFF or 0xFF 0x7F, an empty raw segment before an MQ restart, a
cleanup pass of segmentation symbols alone), and from libopenjp2's own files through Oracle.file_blocks, which is how
vertically causal contexts get here (nothing in this repository writes them).
"""
import json
import os
import struct

import numpy as np

import decode_stage_cases as dsc
import t1_styled_families as fam

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

LASTPASS_STYLES = [1, 4, 1 | 4, 1 | 2 | 32, 55]
MANYPLANES_STYLES = [1, 1 | 4]
# (w, h) of the six blocks of the small family that the every-last-pass and cut-short cases use, looked up by shape: the
# 64 x 64 16-bit noise, 37 x 64, 5 x 7 (first of each shape: the busy kind), steered_3x5 (index 0), drain_block, 1 x 1
SIX = [("noise64", None), ("37x64", None), ("5x7", None), ("steered_3x5", 0), ("drain_block", fam.DRAIN_INDEX), ("1x1", None)]


def styled_files():
    """(name, path, committed hashes per reduce: {reduce: [sha256 per component]}) of the eighteen styled fixtures and the
    decode-only ones."""
    out = []
    g = json.load(open(os.path.join(GOLDEN, "golden.json")))
    for name in sorted(g):
        p = os.path.join(GOLDEN, "ext", name + ".j2k")
        if os.path.exists(p) and g[name].get("ext", {}).get("mode"):
            out.append((name, p, {int(r): [c["sha256"] for c in comps] for r, comps in g[name]["decoded_comps"].items()}))
    for sub, index in (("styles", "styles.json"), ("styles_dec", "styles_dec.json")):
        m = json.load(open(os.path.join(GOLDEN, sub, index)))
        for name in sorted(m):
            if not name.startswith("_"):
                out.append((name, os.path.join(GOLDEN, sub, name + ".j2k"), {0: [c["sha256"] for c in m[name]["decoded_comps"]]}))
    return out


FILE_NAMES = [n for n, _, _ in styled_files()]


# ------------------------------------------------------------------------------------------------ segment tables
def partition_rule(style, npasses):
    """The pass counts of a block's codeword segments as B.10.7.2 and the plan's seg_capacity give them: termall one pass
    each; bypass 10, then 2, 1, 2, 1 ...; the last may be shorter."""
    if not style & 5:
        return []
    out, left, prev = [], npasses, 0
    while left:
        cap = 1 if style & 4 else (10 if not out else (1 if prev == 2 else 2))
        out.append(min(cap, left))
        left -= out[-1]
        prev = cap
    return out


def seg_table(r, style, p=None, full_open=False):
    """(segments, bytes) of the first p passes (default: all) of an oracle-coded block r as Tier-2 would hand them over at a
    layer that ends with pass p: the segments that are complete, and the open one with its passes so far and its bytes up
    to rates[p - 1] -- or, full_open, all its bytes."""
    total = r["npasses"]
    np_ = total if p is None else p
    if np_ == 0:
        return [], 0
    ends = [bool(r["seg_ends"][q]) or q == total - 1 for q in range(total)]
    if not style & 5:
        return [], (r["rates"][total - 1] if full_open else r["rates"][np_ - 1])
    segs, start_p, start_b = [], 0, 0
    for q in range(np_):
        if ends[q] or q == np_ - 1:
            at = q if (ends[q] or not full_open) else next(k for k in range(q, total) if ends[k])
            nbytes = max(r["rates"][at], start_b)
            segs.append((nbytes - start_b, q + 1 - start_p))
            start_p, start_b = q + 1, nbytes
    return segs, start_b


def clip_segs(segs, cw_len):
    """The plan's `have` rule: a segment ends where the block's bytes end."""
    out, at = [], 0
    for n, p in segs:
        out.append((min(n, cw_len - at) if at < cw_len else 0, p))
        at += n
    return out


def make_case(r, w, h, orient, style, half_step, p=None, full_open=False, roishift=0):
    segs, nbytes = seg_table(r, style, p, full_open)
    return dict(w=w, h=h, orient=orient, numbps=r["numbps"], npasses=r["npasses"] if p is None else p, data=r["data"][:nbytes], segs=segs,
                half_step=half_step, roishift=roishift)


def family_cases(oracle, family, rev, style):
    """Every block of the family, all passes."""
    _, rects, orients, step = fam.plane(family, rev)
    hs = float(np.float32(0.5) * np.float32(step))
    return [make_case(r, w, h, o, style, hs) for r, (_, _, w, h), o in zip(fam.refs(oracle, family, rev, style), rects, orients)]


def six_blocks():
    """Indices into the small family of the six blocks of SIX."""
    blocks = fam.small_blocks(True)
    idx = []
    for name, fixed in SIX:
        if fixed is not None:
            idx.append(fixed)
            continue
        want = {"noise64": (64, 64), "37x64": (64, 37), "5x7": (7, 5), "1x1": (1, 1)}[name]  # (h, w)
        idx.append(next(i for i, (b, _) in enumerate(blocks) if b.shape == want and i >= 2))
    assert len(set(idx)) == 6
    return idx


# ------------------------------------------------------------------------------------------------ expectations
def expected_words(oracle, case, rev, style):
    np_ = dsc.kernel_passes(case["numbps"], case["npasses"])
    if np_ == 0:
        return None
    v = oracle.t1_decode_block(case["data"], case["w"], case["h"], case["orient"], case["numbps"], np_, style=style, segs=case["segs"])
    v = dsc.roi_unshift(v, case["roishift"])
    if rev:
        return (np.sign(v) * (np.abs(v) // 2)).astype(np.int32)
    return (v.astype(np.float32) * np.float32(case["half_step"])).view(np.int32)


def decode_and_expect(enc, oracle, cases, rev, style):
    shape, rects = dsc.lay_out(cases)
    fill = dsc.fill_pattern(shape)
    want = fill.copy()
    blocks = []
    for c, (x, y, w, h) in zip(cases, rects):
        e = expected_words(oracle, c, rev, style)
        if e is not None:
            want[y:y + h, x:x + w] = e
        blocks.append(dict(rect=(x, y, w, h), orient=c["orient"], numbps=c["numbps"], npasses=c["npasses"], data=c["data"], segs=c["segs"],
                           half_step=c["half_step"], roishift=c["roishift"]))
    plane = fill if rev else fill.view(np.float32)
    got = enc.stage_t1_decode_styled(plane, blocks, rev, style)
    return got.view(np.int32), want, rects


def write_case_file(path, oracle, batches):
    """The case file of tests/native/t1_lane_styled_host.cpp; returns (cases, cases that are decoded)."""
    n = dec = 0
    with open(path, "wb") as f:
        f.write(b"T1LD" + struct.pack("<I", sum(len(c) for _, _, c in batches)))
        for rev, style, cases in batches:
            for c in cases:
                e = expected_words(oracle, c, rev, style)
                hs = int(np.array([c["half_step"]], dtype=np.float32).view(np.uint32)[0])
                f.write(struct.pack("<11I", style, int(rev), c["w"], c["h"], c["orient"], c["numbps"], c["npasses"], c["roishift"], hs,
                                    len(c["data"]), len(c["segs"])))
                for s in c["segs"]:
                    f.write(struct.pack("<2I", *s))
                f.write(c["data"])
                f.write(struct.pack("<I", int(e is not None)))
                if e is not None:
                    f.write(np.ascontiguousarray(e, dtype=np.int32).tobytes())
                    dec += 1
                n += 1
    return n, dec


# ------------------------------------------------------------------------------------------------ the groups
def _small(oracle, style, idx):
    _, rects, orients, _ = fam.plane("small", True)
    rs = fam.refs(oracle, "small", True, style)
    return [(rs[i], rects[i][2], rects[i][3], orients[i]) for i in idx]


def lastpass_cases(oracle, style):
    """Every p in 1 .. npasses of the six blocks, bytes cut at rates[p - 1]; every fifth p again with the open segment whole."""
    out = []
    for r, w, h, o in _small(oracle, style, six_blocks()):
        for p in range(1, r["npasses"] + 1):
            out.append(make_case(r, w, h, o, style, 1.0, p))
            if p % 5 == 0:
                out.append(make_case(r, w, h, o, style, 1.0, p, full_open=True))
    return out


def cutshort_cases(oracle, style):
    """The six blocks with cw_len cut to 0, 1, half and one byte before a segment end, the segment lengths clipped by the
    plan's rule; and with the table cut so that later passes open segments that are not listed (all bytes present)."""
    out = []
    for r, w, h, o in _small(oracle, style, six_blocks()):
        full = make_case(r, w, h, o, style, 1.0)
        n = len(full["data"])
        ends = np.cumsum([s[0] for s in full["segs"]]).tolist() or [n]
        cuts = {0, min(1, n), n // 2} | {e - 1 for e in (ends[0], ends[len(ends) // 2], ends[-1]) if e >= 1}
        for cut in sorted(cuts):
            out.append(dsc.variant(full, data=full["data"][:cut], segs=clip_segs(full["segs"], cut)))
        if style & 5:
            for keep in sorted({1, 2, len(full["segs"]) // 2, len(full["segs"]) - 1}):
                if 1 <= keep < len(full["segs"]):
                    out.append(dsc.variant(full, segs=full["segs"][:keep]))
    return out


SPOILED_STYLES = [1, 1 | 4]
SPOIL_PATTERNS = [b"\xff\x8f", b"\xff\x90", b"\xff\xff", b"\xff\x7f\xff\x8f"]


def spoiled_raw_cases(oracle, style):
    """Raw segments with bytes no encoder writes, as a damaged file has them: behind a raw 0xFF a byte of 0x8F (the largest
    that is still data: seven of its bits are read) and bytes above it (a marker: 1-bits from there on)."""
    out = []
    six = six_blocks()
    for r, w, h, o in _small(oracle, style, [six[0], six[1], six[4]]):  # the blocks with long raw segments
        full = make_case(r, w, h, o, style, 1.0)
        at, raws, p = 0, [], 0
        for n, k in full["segs"]:
            if p >= 10 and (p - 1) % 3 != 2 and n >= 8:
                raws.append((at, n))
            at, p = at + n, p + k
        assert raws
        for j, pat in enumerate(SPOIL_PATTERNS):
            data = bytearray(full["data"])
            for a, n in raws[j % 2::2]:
                for off in (1, n // 2):
                    data[a + off:a + off + len(pat)] = pat
            out.append(dsc.variant(full, data=bytes(data)))
    return out


DAMAGE_MQ_KINDS = ["marker90", "markerc3", "markerff", "ff8f", "flip", "ff_last", "ff_last_00"]
_dmq_cache = {}


def _damaged_mq(oracle, style):
    """[(damaged case, clean case, kind, indices of the segments touched)]"""
    if style in _dmq_cache:
        return _dmq_cache[style]
    assert style & 5
    out = []
    six = six_blocks()
    for r, w, h, o in _small(oracle, style, [six[0], six[1], six[4]]):  # the blocks with many and long segments
        full = make_case(r, w, h, o, style, 1.0)
        at, p, mq = 0, 0, []  # (index, offset, length, the next segment is MQ-coded and holds a byte) of the MQ-coded segments
        spans = []
        for n, k in full["segs"]:
            spans.append((at, n, not (style & 1 and p >= 10 and (p - 1) % 3 != 2)))
            at, p = at + n, p + k
        for i, (a, n, is_mq) in enumerate(spans):
            if is_mq and n >= 1:
                mq.append((i, a, n, i + 1 < len(spans) and spans[i + 1][2] and spans[i + 1][1] >= 1))
        assert len(mq) >= 2 and mq[0][0] == 0
        for kind in DAMAGE_MQ_KINDS:
            for half in (0, 1):  # the segments in turn: segment 0 (no restart before it) is in the first half alone
                data, touched = bytearray(full["data"]), []
                for j, (i, a, n, next_mq) in enumerate(mq[half::2]):
                    if kind in ("ff_last", "ff_last_00"):
                        if kind == "ff_last_00" and not next_mq:
                            continue
                        data[a + n - 1] = 0xFF  # the segment's last byte, directly before the next segment's first byte
                        if kind == "ff_last_00":
                            data[a + n] = 0x00  # (not a marker: a decoder that looked at it would take seven bits of it)
                        touched.append(i)
                        continue
                    off = min(1, n - 2) if j % 2 == 0 else n // 2 - 1  # near the segment's start, and half way into it
                    if off >= 0 and off + 2 <= n:
                        if kind == "flip":
                            data[a + off] ^= 1 << (off % 8)
                        else:
                            data[a + off:a + off + 2] = {"marker90": b"\xff\x90", "markerc3": b"\xff\xc3", "markerff": b"\xff\xff", "ff8f": b"\xff\x8f"}[kind]
                        touched.append(i)
                if touched and bytes(data) != full["data"]:
                    out.append((dsc.variant(full, data=bytes(data)), full, kind, sorted(set(touched))))
    _dmq_cache[style] = out
    return out


def damaged_mq_cases(oracle, style):
    """MQ-coded segments with bytes no encoder writes, as a damaged file has them (raw segments: spoiled_raw_cases): a marker
    inside a terminated segment, 0xFF 0x8F, a flipped bit, 0xFF as a segment's last byte directly before the next
    segment's first byte -- in the block's first segment and in segments that follow an MQ restart.  The segment table is
    the clean case's."""
    return [c for c, _, _, _ in _damaged_mq(oracle, style)]


def damaged_mq_info(oracle, style):
    """Per case of damaged_mq_cases: (the clean case, the kind of damage, the segments touched)."""
    return [(clean, kind, touched) for _, clean, kind, touched in _damaged_mq(oracle, style)]


_file_cache = {}


def file_batch(oracle, name):
    if name not in _file_cache:
        path = next(p for n, p, _ in styled_files() if n == name)
        fb = oracle.file_blocks(open(path, "rb").read())
        cases = [dict(w=b["w"], h=b["h"], orient=b["orient"], numbps=b["numbps"], npasses=b["npasses"], data=b["data"], segs=b["segs"],
                      half_step=b["half_step"], roishift=0) for b in fb["blocks"]]
        _file_cache[name] = (fb["reversible"], fb["style"], cases)
    return _file_cache[name]


def manyplanes_batches(oracle):
    rng = np.random.default_rng(77)
    blocks = [(dsc.top_planes_block(rng), 1), (dsc.long_stream_block(rng), 2)]
    out = []
    for style in MANYPLANES_STYLES:
        cases = []
        for data, o in blocks:
            r = oracle.t1_block(data, o, style=style)
            h, w = data.shape
            for shift in (0, 7):
                cases.append(make_case(r, w, h, o, style, 1.0, roishift=shift))
        out.append((True, style, cases))
    return out


ORDER_STYLE = 1 | 4


def order_batches(oracle):
    """The small family reversed (shortest block in lane 0) and interleaved with all-zero blocks; groups of 1, 63, 64 and 65
    blocks; one wave mixing blocks of at most 9 passes, empty blocks and raw-heavy blocks."""
    cases = family_cases(oracle, "small", True, ORDER_STYLE)
    empty = dict(w=64, h=64, orient=0, numbps=0, npasses=0, data=b"", segs=[], half_step=1.0, roishift=0)
    rev_mix = [c for pair in zip(cases[::-1], [empty] * len(cases)) for c in pair]
    out = [(True, ORDER_STYLE, rev_mix)]
    pool = (cases * 2)[:65]
    for n in (1, 63, 64, 65):
        out.append((True, ORDER_STYLE, pool[:n]))
    by1 = family_cases(oracle, "small", True, 1)
    short = [c for c in by1 if 1 <= c["npasses"] <= 9]
    heavy = [c for c in by1 if c["npasses"] >= 40]
    assert short and heavy
    wave = [(short + [empty] + heavy)[i % (len(short) + 1 + len(heavy))] for i in range(64)]
    out.append((True, 1, wave))
    return out


def _family_group(family, rev, style):
    return lambda oracle: [(rev, style, family_cases(oracle, family, rev, style))]


GROUPS = {}
for _s in fam.MIXED_STYLES_REV:
    GROUPS[f"mixed-rev-{_s}"] = _family_group("mixed", True, _s)
for _s in fam.MIXED_STYLES_IRR:
    GROUPS[f"mixed-irr-{_s}"] = _family_group("mixed", False, _s)
for _s in fam.SMALL_STYLES:
    GROUPS[f"small-{_s}"] = _family_group("small", True, _s)
for _s in LASTPASS_STYLES:
    GROUPS[f"lastpass-{_s}"] = (lambda s: lambda oracle: [(True, s, lastpass_cases(oracle, s))])(_s)
    GROUPS[f"cutshort-{_s}"] = (lambda s: lambda oracle: [(True, s, cutshort_cases(oracle, s))])(_s)
for _s in SPOILED_STYLES:
    GROUPS[f"spoiled-raw-{_s}"] = (lambda s: lambda oracle: [(True, s, spoiled_raw_cases(oracle, s))])(_s)
for _s in LASTPASS_STYLES:
    GROUPS[f"damaged-mq-{_s}"] = (lambda s: lambda oracle: [(True, s, damaged_mq_cases(oracle, s))])(_s)
for _n in FILE_NAMES:
    GROUPS[f"file-{_n}"] = (lambda n: lambda oracle: [file_batch(oracle, n)])(_n)
GROUPS["manyplanes"] = manyplanes_batches
GROUPS["order"] = order_batches
GROUP_NAMES = list(GROUPS)


def group(oracle, name):
    return GROUPS[name](oracle)
