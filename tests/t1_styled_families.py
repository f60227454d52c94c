"""Code-blocks for the block-level tests of the styled Tier-1 coder (test_t1_styled_blocks.py on the GPU,
test_t1_mq_styled_host.py and test_t1_styled_refs.py on the CPU), their references from the oracle, and the conditions
the references must meet before a comparison with them means anything.  Plain helpers: no fixtures, no tests.

  mixed   134 blocks of 64 x 64 cells = two full workgroups of the styled coder (a lane per block) and one of 6 lanes,
          built like the mix of test_mq_coder_paths.py: the longest block in lane 0, the shortest non-empty one in the last
          lane, all-zero blocks between them -- and one lane of eight holds a small block with many bit-planes
          (1 x 1, 1 x 64, 64 x 1, 4 x 4, 3 x 5; magnitudes up to 16 bits), whose passes end every few decisions.
  small   40 blocks = one workgroup: 32 x 32, 64 x 13, 37 x 64, 5 x 7, 1 x 1, 16 x 16, 64 x 64, the two steered blocks
          below, an 8 x 8 block found by a seed search (FF7F_SEEDS) and the 32 x 32 block of drain_block (DRAIN_SEED).

The coder kernel stages each lane's bytes and lets whole 16-byte units go once 64 wait, keeping 16..31: the end of a raw
segment looks back at (and takes back) up to two bytes, and a restart takes back the last byte of the segment before
it; they must still be staged.  FLUSH and the predictable termination keep the pending byte in a register and write at
least one byte, which the restart behind them finds.  Two things look back at a byte staged BEFORE the pass end, and so
possibly in front of a drain: the end of a raw segment (its last byte 0xFF, or 0xFF 0x7F), and the restart behind a raw
segment whose end wrote nothing (byte-aligned).  It matters only where that drain found a multiple of 16 bytes staged,
64 or more, so that a drain keeping less than a unit would have kept none.  The byte counts at segment ends cannot show
that (check_staged_ends asks only for ends near such counts), and noise meets it by chance: block 111 of the mixed
family does under bypass with PTERM.  drain_block is steered at it: its raw refinement passes end in a run of ones, and
DRAIN_SEED is a seed for which, under bypass alone and under bypass with TERMALL, a model of the stage that keeps 0..15
bytes gives another codeword than one that keeps 16..31 (the host program of test_t1_mq_styled_host.py holds both
models and that test asserts it for DRAIN_CASES).  Under the other bypass styles the block is one more long block.

Raw segments meet their 0xFF cases about once in 2^11 (a trailing 0xFF) or 2^18 (a trailing 0xFF 0x7F) segments, which no
fixed seed of noise shows.  Two small blocks are therefore steered at them (steered_3x5, steered_4x4): samples that are
significant from the first pass on and 1 in every raw plane, so that a raw refinement pass is the bits 0xFF 0x7F, or the
byte 0xFF, exactly; they sit in both families, in 5/3 and 9/7 values alike.

Conditions (check_lengths, check_staged_ends, check_bypass_events, check_segsym; `conditions` applies those that the
style calls for).  Not every condition asked of these families can be met as stated:

  * "An MQ segment whose predecessor ends in 0xFF before the take-back (a restart with CT = 13)" cannot occur: FLUSH and
    the predictable termination leave bp in front of a last byte 0xFF (it is not counted), the end of a raw segment takes
    a trailing 0xFF back or, under predictable termination, pads a byte behind it, and an empty raw segment leaves the MQ
    segment before it as it ended.  No terminated segment ends in 0xFF, so no restart sees one (libopenjp2 asserts the
    same in opj_mqc_restart_init_enc).  The oracle counts such restarts (events["restart_ct13"]) and check_bypass_events
    asserts that there is none; the branch `CT = 13` of StyledCoder::restart is therefore NOT covered by any test.
  * Under predictable termination nothing is taken back from a raw segment (a trailing 0xFF gets a padded byte behind it,
    0xFF 0x7F stays), so "a raw segment that ended on a dropped 0xFF" and "an MQ segment that follows a raw segment of
    length 0" do not exist under PTERM, and without TERMALL no raw segment of length 0 exists at all (a raw pair always
    holds the refinement bits of the samples significant by then; only a raw significance pass alone can have no bit,
    and the raw refinement pass follows it, not an MQ segment).  check_bypass_events asserts these counts to be 0 there
    and asks for the kept 0xFF 0x7F instead; the take-backs are covered by the eight bypass styles without PTERM.
  * The seed search for the 0xFF 0x7F ending in 8 x 8 blocks of 16 planes (search_ff7f, seeds 0 .. 2^20 - 1) found seed
    28813 for bypass with TERMALL (every raw pass a segment of its own) and NONE for bypass without TERMALL (raw pairs):
    the 64 refinement bits of such a block fill whole bytes only with no 0xFF among them, so a pair must also hold
    exactly seven significance bits.  Without TERMALL the case is covered by steered_3x5 alone.
"""
import numpy as np

from t1_families import layout, random_block, signs

ALL_FIVE = 1 | 2 | 4 | 16 | 32
MIXED_STYLES_REV = [1, 2, 4, 16, 32, 1 | 4, 1 | 16, 4 | 16, ALL_FIVE]
MIXED_STYLES_IRR = [1, ALL_FIVE]
SMALL_STYLES = [s for s in range(1, 64) if not s & 8]  # the 31 combinations of bypass, reset, termall, pterm, segsym
IRR_STEP = 0.37

NMIXED = 134  # 64 + 64 + 6
MIXED_SEED = 20
SMALL_SEED = 7
# 8 x 8 blocks of integers_block(seed, 8, 8, 16) in which a raw segment ends on 0xFF 0x7F: [0] under bypass without TERMALL
# (search_ff7f(oracle, 1, 2): none among the seeds 0 .. 2^20 - 1), [1] under bypass with TERMALL (search_ff7f(oracle, 5, 3):
# the first hit).  The orientations are those of the places the blocks take in the small family.
FF7F_SEEDS = (None, 28813)

# drain_block(DRAIN_SEED) in the small family (orientation 2, its place there): under each of DRAIN_STYLES the end of a raw
# segment looks back at bytes that a drain of the stage keeping fewer than 16 bytes would have let go (seeds 0 .. 399 tried
# with the host program's two stage models; 193 is the first that does so under both styles)
DRAIN_SEED = 193
DRAIN_STYLES = (1, 1 | 4)
DRAIN_INDEX = 38  # its index in the small family
# (family, block, style) for which the two stage models differ, each run by a GPU test; the last is noise that meets it
DRAIN_CASES = [("small", DRAIN_INDEX, s) for s in DRAIN_STYLES] + [("mixed", 111, 1 | 16)]

SMALL_SHAPES = [(1, 1), (1, 64), (64, 1), (4, 4), (3, 5)]  # (w, h)


def integers_block(seed, w, h, bits):
    rng = np.random.default_rng(seed)
    return rng.integers(-(1 << bits) + 1, 1 << bits, size=(h, w)).astype(np.int64)


def _noise(rng, bits):
    return rng.integers(-(1 << bits) + 1, 1 << bits, size=(64, 64))


def _few(rng, n, top):
    b = np.zeros((64, 64), dtype=np.int64)
    ys, xs = rng.integers(0, 64, size=n), rng.integers(0, 64, size=n)
    b[ys, xs] = rng.integers(2, 1 << top, size=n) * signs(rng, n)  # (two bit-planes at least: longer than the last lane's block)
    return b


def _quantised(v):
    """The integer magnitude the 9/7 path codes for the coefficient v of these planes (0.61 v in float32, step IRR_STEP)."""
    c = np.float32(v * 0.61)
    return int(np.rint(c / np.float32(IRR_STEP) * np.float32(64))) >> 6


def all_ones_values(rev):
    """Coefficients whose coded magnitudes are 0x8FFF, 0x9FFF .. 0xFFFF: 16 bit-planes, significant from the first pass on,
    and a 1 in each of the twelve planes that bypass writes as raw bits (reversible: the values themselves; 9/7: those of
    them that some coefficient quantises to)."""
    want = [(n << 12) | 0xfff for n in range(8, 16)]
    if rev:
        return want
    out = []
    for m in want:
        v0 = int(m * IRR_STEP / 0.61)
        out += [v for v in range(v0 - 2, v0 + 3) if _quantised(v) == m][:1]
    return out


def steered_3x5(rng, rev):
    """15 samples, all significant before the raw passes begin, all ones below: every refinement pass from pass 11 on is the
    bits 0xFF 0x7F exactly, its significance pass has no decision.  Without predictable termination both bytes are taken
    back: a raw segment of no bytes, and the MQ segment of the cleanup pass restarts behind it."""
    vals = all_ones_values(rev)
    return np.array([vals[i % len(vals)] for i in range(15)]).reshape(5, 3) * signs(rng, (5, 3))


def steered_4x4(rng, rev):
    """8 samples as in steered_3x5 and 8 zeros that never turn significant: every raw refinement pass is the byte 0xFF, taken
    back at the end of the segment (behind the eight 0 bits of the significance pass, or alone under TERMALL)."""
    vals = all_ones_values(rev)
    b = np.zeros((4, 4), dtype=np.int64)
    b[:, ::2] = np.array([vals[i % len(vals)] for i in range(8)]).reshape(4, 2) * signs(rng, (4, 2))
    return b


def drain_block(seed):
    """32 x 32 samples of 16 bit-planes, nearly all significant in the first one (a few turn significant later, which
    moves the pass ends among the chunks of 16 decisions), the last 8..16 of the scan all ones: every raw refinement pass
    is 1024 bits or nearly, so the stage drains many times inside it, and ends in 0xFF or 0xFF 0x7F."""
    rng = np.random.default_rng(seed)
    b = rng.integers(1 << 15, 1 << 16, size=(32, 32))
    late = rng.random((32, 32)) < 0.05
    b[late] >>= rng.integers(1, 12, size=int(late.sum()))
    tail = b[28:32, 28:32].T.reshape(-1)  # the scan runs down each column of the stripe
    tail[8 - seed % 9:] = 0xffff
    b[28:32, 28:32] = tail.reshape(4, 4).T
    return (b * signs(rng, (32, 32))).astype(np.int64)


def _workgroup(rng, lanes, first_small, rev):
    blocks = []
    for lane in range(lanes):
        k = lane % 8
        if lane == 0:
            b = _noise(rng, 16)  # the longest: noise over the whole 16-bit range
        elif lane == lanes - 1:
            b = np.ones((1, 1), dtype=np.int64)  # the shortest: one sample, one bit-plane, one pass (the 1 x 1 blocks of many planes take three bytes and more)
        elif k in (1, 5):
            b = _noise(rng, 13 + lane % 3)
        elif k == 2:
            b = _few(rng, 1 + lane % 5, 3 + lane % 4)
        elif k == 3:
            b = np.zeros((64, 64), dtype=np.int64)
        elif k == 4:
            b = np.where(rng.random((64, 64)) < 0.002 * (1 + lane % 7), rng.integers(1, 1 << (4 + lane % 9), size=(64, 64)), 0) * signs(rng, (64, 64))
        elif k == 6:
            b = random_block(rng, 64, 64, lane % 4)
        elif k == 0:
            b = np.rint(rng.laplace(0, 1 << (lane % 11), size=(64, 64))).astype(np.int64)
        else:  # one lane of eight: a small block with many bit-planes
            w, h = SMALL_SHAPES[(first_small + lane // 8) % len(SMALL_SHAPES)]
            if (w, h) == (3, 5):
                b = steered_3x5(rng, rev)
            elif (w, h) == (4, 4):
                b = steered_4x4(rng, rev)
            else:
                b = rng.integers(1 << 12, 1 << 16, size=(h, w)) * signs(rng, (h, w))
                if w * h > 1:
                    b[rng.random((h, w)) < 0.3] >>= 9  # some samples turn significant late
        blocks.append(np.asarray(b, dtype=np.int64))
    return blocks


def mixed_blocks(rev=True):
    rng = np.random.default_rng(MIXED_SEED)
    blocks = _workgroup(rng, 64, 0, rev) + _workgroup(rng, 64, 2, rev) + _workgroup(rng, NMIXED - 128, 0, rev)
    return [(b, i % 4) for i, b in enumerate(blocks)]


def small_blocks(rev=True):
    rng = np.random.default_rng(SMALL_SEED)
    shapes = [(32, 32), (64, 13), (37, 64), (5, 7), (1, 1), (16, 16), (64, 64)]
    blocks = [steered_3x5(rng, rev), steered_4x4(rng, rev)]
    for i in range(40 - 3 - len([s for s in FF7F_SEEDS if s is not None])):
        w, h = shapes[i % len(shapes)]
        kind = i // len(shapes)
        if kind == 0:
            b = rng.integers(-(1 << 16) + 1, 1 << 16, size=(h, w))  # every plane busy: long raw segments
        elif kind == 1:
            b = np.rint(rng.laplace(0, 1 << 9, size=(h, w)))
        elif kind == 2:
            b = np.where(rng.random((h, w)) < 0.1, rng.integers(1, 1 << 14, size=(h, w)), 0) * signs(rng, (h, w))
            b[0, 0] = 1 << 14
        elif kind == 3:
            b = rng.integers(0, 1 << 3, size=(h, w)) * signs(rng, (h, w))  # fewer than 10 passes
        else:
            b = random_block(rng, w, h, i % 4)
        blocks.append(np.asarray(b, dtype=np.int64))
    assert len(blocks) == DRAIN_INDEX
    blocks.append(drain_block(DRAIN_SEED))
    blocks += [integers_block(s, 8, 8, 16) for s in FF7F_SEEDS if s is not None]
    return [(b, i % 4) for i, b in enumerate(blocks)]


FAMILIES = {"mixed": mixed_blocks, "small": small_blocks}
_planes = {}
_refs = {}


def plane(family, rev):
    """(plane for the encoder, rectangles, orientations, step size) of a family; the same arrays at every call."""
    key = (family, rev)
    if key not in _planes:
        coef, rects, orients = layout(FAMILIES[family](rev))
        pl = coef.astype(np.int32) if rev else (coef * 0.61).astype(np.float32)
        pl.setflags(write=False)
        _planes[key] = (pl, rects, orients, 1.0 if rev else IRR_STEP)
    return _planes[key]


def scaled_blocks(oracle, family, rev):
    """The blocks as the Tier-1 coder sees them: int32 with 6 fractional bits."""
    pl, rects, orients, step = plane(family, rev)
    quant = oracle.L.j2ko_quant97
    out = []
    for (x, y, w, h), o in zip(rects, orients):
        blk = pl[y:y + h, x:x + w]
        if rev:
            data = (blk.astype(np.int64) << 6).astype(np.int32)
        elif not blk.any():
            data = np.zeros((h, w), dtype=np.int32)
        else:
            data = np.array([[quant(float(v), step) if v else 0 for v in row] for row in blk], dtype=np.int32)
        out.append((data, o))
    return out


_scaled = {}


def refs(oracle, family, rev, style):
    """The oracle's result for every block of the family under the style (with pass_nsym, without the decisions), computed
    once per session."""
    key = (family, rev, style)
    if key not in _refs:
        if (family, rev) not in _scaled:
            _scaled[(family, rev)] = scaled_blocks(oracle, family, rev)
        out = []
        for data, o in _scaled[(family, rev)]:
            r = oracle.t1_block(data, o, style=style, want_symbols=True)
            del r["symbols"]
            out.append(r)
        _refs[key] = out
    return _refs[key]


def where(i, style):
    return (i // 64, i % 64, style)  # workgroup, lane, style


# ---- the conditions
def check_lengths(rs):
    """Every workgroup: a block with no pass, one with 1..9 passes (bypass never leaves MQ), one with at least 40, and a
    codeword over 4096 bytes next to one under 16; the longest block in lane 0, the shortest non-empty one in the last."""
    assert len(rs) == NMIXED
    for g in range(0, NMIXED, 64):
        grp = rs[g:g + 64]
        nps = [r["npasses"] for r in grp]
        lens = [len(r["data"]) for r in grp]
        some = [n for n in lens if n]
        assert 0 in nps, g
        assert any(1 <= n <= 9 for n in nps), g
        assert max(nps) >= 40, g
        assert max(lens) > 4096 and min(some) < 16, (g, max(lens), min(some))
        assert lens[0] == max(lens) and lens[-1] == min(some), (g, lens[0], lens[-1], max(lens), min(some))


def seg_ends_of(r):
    """(pass, byte count, decisions so far) at every pass of the block that ends a codeword segment."""
    return [(p, r["rates"][p], r["pass_nsym"][p]) for p in range(r["npasses"]) if r["seg_ends"][p]]


def check_staged_ends(rs):
    """TERMALL: a segment that ends at a byte count just behind a multiple of 16 from 64 on, where the coder's stage may just
    have drained (what the drain must keep for a termination is held by drain_block, not by this: see the module
    docstring), and three or more segment ends inside one chunk of 16 decisions."""
    ends = [e for r in rs for e in seg_ends_of(r)]
    assert any(n >= 64 and (n - 64) % 16 < 4 for _, n, _ in ends)
    crowded = 0
    for r in rs:
        chunks = [s // 16 for _, _, s in seg_ends_of(r)]
        crowded += any(chunks.count(c) >= 3 for c in set(chunks))
    assert crowded


def check_bypass_events(rs, termall, pterm):
    """BYPASS: raw segments of no bytes, MQ segments right behind one, raw 0xFF bytes with bits behind them, raw segments that
    ended on a dropped 0xFF, and on 0xFF 0x7F: dropped without predictable termination, kept with it."""
    total = {k: sum(r["events"][k] for r in rs if r["npasses"]) for k in rs[0]["events"]} if rs else {}
    assert total["raw_ff_inside"] >= 1, total
    assert total["restart_ct13"] == 0, total  # cannot occur: see the module docstring
    if pterm:  # nothing is taken back: see the module docstring
        assert total["raw_ff7f_kept"] >= 1, total
        assert total["raw_ff_dropped"] == total["raw_ff7f_dropped"] == total["mq_after_empty_raw"] == 0, total
    else:
        assert total["raw_ff_dropped"] >= 1, total
        assert total["raw_ff7f_dropped"] >= 1, total
        assert total["mq_after_empty_raw"] >= 1, total
    assert any(r["npasses"] >= 11 for r in rs) and any(1 <= r["npasses"] <= 9 for r in rs)
    if pterm and not termall:
        assert total["raw_empty"] == 0, total
        return
    assert total["raw_empty"] >= 1, total
    # the same from the outside: a raw segment (it starts at a significance pass from pass 10 on) of no bytes
    empties = 0
    for r in rs:
        prev = 0
        for p, n, _ in seg_ends_of(r):
            if p >= 10 and (p + 2) % 3 != 2 and n == prev:
                empties += 1
            prev = n
    assert empties >= 1


def check_segsym(rs):
    """SEGSYM: a cleanup pass whose only decisions are the four segmentation symbols."""
    assert sum(r["events"]["segsym_alone"] for r in rs if r["npasses"]) >= 1


def conditions(family, style, rs):
    if family == "mixed":
        check_lengths(rs)
    if style & 4:
        check_staged_ends(rs)
    if style & 1:
        check_bypass_events(rs, bool(style & 4), bool(style & 16))
    if style & 32:
        check_segsym(rs)


def compare(got, rs, style):
    """A stage hook's result against the oracle's: bit-planes, passes, length and bytes exactly; the byte counts per pass
    exactly where a segment ends and at the last pass, elsewhere non-decreasing and within the length (all that the files
    of libopenjp2 pin, and all that a styled frame uses: test_oracle_golden.py)."""
    assert len(got) == len(rs)
    for i, (g, r) in enumerate(zip(got, rs)):
        at = where(i, style)
        assert g["numbps"] == r["numbps"], at
        assert g["npasses"] == r["npasses"], at
        assert g["length"] == len(r["data"]), at
        assert g["data"] == r["data"], at
        np_ = r["npasses"]
        assert len(g["rates"]) == np_, at
        for p in range(np_):
            if r["seg_ends"][p] or p == np_ - 1:
                assert g["rates"][p] == r["rates"][p], at + (p,)
            assert g["rates"][p] <= g["length"], at + (p,)
            assert p == 0 or g["rates"][p - 1] <= g["rates"][p], at + (p,)


def search_ff7f(oracle, style, orient, limit=1 << 20):
    """The first seed of integers_block(seed, 8, 8, 16) whose coding under `style` (1 or 1 | 4) in a band of orientation
    `orient` (the block's place in the small family decides it) meets the 0xFF 0x7F ending."""
    for seed in range(limit):
        data = (integers_block(seed, 8, 8, 16) << 6).astype(np.int32)
        if oracle.t1_block(data, orient, style=style)["events"]["raw_ff7f_dropped"]:
            return seed
    return None
