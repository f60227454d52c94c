"""CPU: what the block-level tests of the styled Tier-1 decoder stand on (test_t1_dec_styled_blocks.py on the GPU,
test_t1_lane_styled_host.py on the host), asserted before any comparison with them means anything.

The oracle's styled block decoder (oracle/j2k_oracle_dec.c: j2ko_t1_decode_block_styled) and its Tier-2 under styles are
pinned from three sides: whole files against the committed hashes of what libopenjp2 decodes (the eighteen styled
fixtures, at every size a hash is committed for, and the decode-only files with vertically causal contexts), and against
the live library where one is installed; style invariance against the unstyled block decoder (already pinned to
libopenjp2) on every block of both families under every style, at all passes and at every pass count that ends a
segment; and equality with the unstyled decoder at style 0.  Then the conditions on the cases themselves."""
import hashlib

import numpy as np
import pytest

import t1_dec_styled_cases as tc
import t1_families
import t1_styled_families as fam

FILES = tc.styled_files()
FAMILY_STYLES = [("mixed", True, s) for s in fam.MIXED_STYLES_REV] + [("mixed", False, s) for s in fam.MIXED_STYLES_IRR] + \
                [("small", True, s) for s in fam.SMALL_STYLES]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.mark.parametrize("name,path,hashes", FILES, ids=[f[0] for f in FILES])
def test_oracle_decodes_styled_files_like_libopenjp2(oracle, name, path, hashes):
    data = open(path, "rb").read()
    assert 0 in hashes
    for reduce, want in sorted(hashes.items()):
        dec = oracle.decode(data, reduce)
        assert [sha(dec[c].astype(np.int32)) for c in range(dec.shape[0])] == want, (name, reduce)


def test_oracle_decodes_styled_files_like_the_live_library(oracle, opj):
    for name, path, hashes in FILES:
        data = open(path, "rb").read()
        for reduce in sorted(hashes):
            ref = opj.decode_comps(data, reduce)
            dec = oracle.decode(data, reduce)
            assert len(ref) == dec.shape[0]
            for c, comp in enumerate(ref):
                assert np.array_equal(dec[c], comp["data"]), (name, reduce, c)


def test_the_decode_only_files_are_as_the_issue_lists_them(oracle):
    want = {"z1": (97, 61, 1, 8), "z2": (97, 61, 1, 8 | 1 | 4), "z3": (17, 9, 1, 63), "z4": (65, 33, 3, 8 | 2 | 32), "z5": (128, 128, 1, 8 | 1)}
    seen = {}
    for name, path, _ in FILES:
        if name[:2] in want:
            data = open(path, "rb").read()
            i = oracle.decode_info(data)
            seen[name[:2]] = (i["width"], i["height"], i["ncomp"], oracle.file_blocks(data)["style"])
            assert len(data) < 16384
    assert seen == want


def test_style_zero_is_the_unstyled_decoder(oracle):
    rng = np.random.default_rng(5)
    n = 0
    for kind in range(4):
        for (w, h) in [(64, 64), (37, 13), (5, 7), (1, 1), (64, 1), (1, 64)]:
            data = (t1_families.random_block(rng, w, h, kind).astype(np.int64) << 6).astype(np.int32)
            r = oracle.t1_block(data, kind)
            for p in {r["npasses"], r["npasses"] // 2, 1} - {0}:
                a = oracle.t1_decode_block(r["data"], w, h, kind, r["numbps"], p)
                b, _ = oracle.t1_decode_block(r["data"], w, h, kind, r["numbps"], p, style=0, segs=None, want_below=True)
                assert np.array_equal(a, b), (kind, w, h, p)
                n += 1
    assert n > 40


@pytest.mark.parametrize("family,rev,style", FAMILY_STYLES)
def test_a_style_changes_the_codeword_never_the_decisions(oracle, family, rev, style):
    """The styled decode of the styled codeword equals the unstyled decode of the unstyled codeword: with all passes, and at
    every pass count p that ends a segment (styled bytes up to that exact end; the unstyled decoder gets its whole codeword
    and npasses = p).  The segment partition is the plan's rule."""
    rs = fam.refs(oracle, family, rev, style)
    fam.conditions(family, style, rs)
    plain = fam.refs(oracle, family, rev, 0)
    _, rects, orients, _ = fam.plane(family, rev)
    cuts = 0
    for i, (r, u, (_, _, w, h), o) in enumerate(zip(rs, plain, rects, orients)):
        assert (r["numbps"], r["npasses"]) == (u["numbps"], u["npasses"]), i
        np_ = r["npasses"]
        if not np_:
            continue
        segs, nbytes = tc.seg_table(r, style)
        assert nbytes == len(r["data"]) and [p for _, p in segs] == tc.partition_rule(style, np_), (i, style)
        ends = [p + 1 for p in range(np_) if r["seg_ends"][p] or p == np_ - 1]
        if style & 5:
            assert ends == np.cumsum(tc.partition_rule(style, np_)).tolist(), (i, style)
        for p in ends:
            sg, nb = tc.seg_table(r, style, p)
            assert nb == r["rates"][p - 1] and sum(n for n, _ in sg) == (nb if style & 5 else 0)
            got = oracle.t1_decode_block(r["data"][:nb], w, h, o, r["numbps"], p, style=style, segs=sg)
            want = oracle.t1_decode_block(u["data"], w, h, o, u["numbps"], p)
            assert np.array_equal(got, want), (family, style, i, p)
            cuts += p < np_
    assert cuts or not style & 5


def test_termall_segments_meet_every_alignment_and_length(oracle):
    """Over the termall styles of the mixed family: segments begin at every residue of the byte offset mod 16, some segment
    is 0, 1 and 2 bytes long, and some raw segment is longer than 64 bytes (the lane decoder's ring)."""
    residues, lengths, long_raw = set(), set(), 0
    for style in [s for s in fam.MIXED_STYLES_REV if s & 4]:
        for c in tc.family_cases(oracle, "mixed", True, style):
            at = p = 0
            for n, k in c["segs"]:
                residues.add(at % 16)
                lengths.add(min(n, 3))
                long_raw += bool(style & 1 and p >= 10 and (p - 1) % 3 != 2 and n > 64)
                at, p = at + n, p + k
    assert residues == set(range(16))
    assert {0, 1, 2} <= lengths
    assert long_raw


def test_vertically_causal_files_show_the_style(oracle):
    """In every vertically causal fixture some block taller than four rows codes a sample of a stripe's last row while a
    neighbour in the row below is significant: without one the style decodes like ordinary contexts and shows nothing."""
    seen = 0
    for name in tc.FILE_NAMES:
        rev, style, cases = tc.file_batch(oracle, name)
        if not style & 8:
            continue
        seen += 1
        hits = 0
        for c in cases:
            _, below = oracle.t1_decode_block(c["data"], c["w"], c["h"], c["orient"], c["numbps"], c["npasses"], style=style, segs=c["segs"],
                                              want_below=True)
            hits += bool(c["h"] > 4 and below)
            # and the style matters: decoded without it, the block comes out different somewhere in the file
        assert hits >= 1, name
        differs = any(not np.array_equal(
            oracle.t1_decode_block(c["data"], c["w"], c["h"], c["orient"], c["numbps"], c["npasses"], style=style, segs=c["segs"]),
            oracle.t1_decode_block(c["data"], c["w"], c["h"], c["orient"], c["numbps"], c["npasses"], style=style & ~8, segs=c["segs"]))
            for c in cases if c["h"] > 4)
        assert differs, name
    assert seen >= 7  # s2, s4 and the five decode-only files


def test_the_groups_hold_what_they_are_for(oracle):
    """Every last pass: a raw pair holding only its significance pass, blocks cut to 10, 11, 12 and 13 passes under bypass.
    Cut short: tables that end before the passes do.  Order: groups of 1, 63, 64 and 65 blocks."""
    for style in tc.LASTPASS_STYLES:
        cases = tc.lastpass_cases(oracle, style)
        nps = {c["npasses"] for c in cases}
        assert {10, 11, 12, 13} <= nps
        if style & 1 and not style & 4:
            assert any(c["npasses"] > 10 and c["segs"][-1][1] == 1 and (c["npasses"] - 1) % 3 == 1 for c in cases)  # the pair's first pass alone
        cut = tc.cutshort_cases(oracle, style)
        assert any(len(c["data"]) == 0 for c in cut) and any(len(c["data"]) == 1 for c in cut)
        if style & 5:
            assert any(sum(p for _, p in c["segs"]) < c["npasses"] for c in cut)
            assert any(sum(n for n, _ in c["segs"]) < len(c["data"]) for c in cut)
    assert [len(c) for _, _, c in tc.order_batches(oracle)][1:5] == [1, 63, 64, 65]
    assert len(tc.family_cases(oracle, "mixed", True, 1)) == fam.NMIXED and len(tc.family_cases(oracle, "small", True, 1)) == 40
    assert len(tc.FILE_NAMES) == 18 + 5
