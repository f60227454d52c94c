"""CPU: what the damaged-bytes tests of the Tier-1 decoders stand on (test_t1_dec_damaged_blocks.py and
test_decode_damaged.py on the GPU), asserted on the references alone so that those tests cannot pass vacuously.

Blocks (oracle.t1_decode_block, pinned to libopenjp2 elsewhere): a marker behind a 0xFF stops the decoder's reading, so the
damaged codeword decodes like itself cut behind the 0xFF; every marker and every single bit flip of the position sets
changes the decode; 0xFF 0x8F (seven more bits) is told from 0xFF 0x90 (a marker) in at least nine of ten places; a marker
behind the bytes of the kept passes changes nothing.  The damaged-mq-* groups of t1_dec_styled_cases.py damage MQ-coded
segments only and change the decode.
Files (tests/golden/damaged): every damaged file decodes the same three ways -- the plain-C oracle, the live libopenjp2
where one is installed, and the committed hashes of libopenjp2's samples."""
import hashlib

import numpy as np
import pytest

import damaged_cases as dm
import decode_stage_cases as dsc
import layers_cases as lc
import t1_dec_styled_cases as tc


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def dec(oracle, c):
    return oracle.t1_decode_block(c["data"], c["w"], c["h"], c["orient"], c["numbps"], dsc.kernel_passes(c["numbps"], c["npasses"]))


# ------------------------------------------------------------------------------------------------ blocks
def test_damage_is_a_function_of_its_arguments():
    data = bytes(range(7, 207))
    state = np.random.get_state()[1].copy()
    for mode in dm.MODES:
        at = 5 if mode in dm.PLACED else None
        a, b = dm.damage(data, mode, at), dm.damage(data, mode, at)
        assert a == b and len(a) == len(data) and a != data, mode
    assert np.array_equal(np.random.get_state()[1], state)
    assert dm.damage(data, "flip", 13) == data[:13] + bytes([data[13] ^ (1 << 5)]) + data[14:]
    assert dm.damage(data, "marker", 63, 0xC3)[62:66] == bytes([data[62], 0xFF, 0xC3, data[65]])
    assert dm.damage(data, "ff8f", 3)[3:5] == b"\xff\x8f" and dm.damage(data, "ff_run", 3)[3:6] == b"\xff\xff\xff"
    assert dm.damage(data, "ff_tail")[-2:] == bytes([data[-2], 0xFF]) and dm.damage(data, "ff7f_tail")[-2:] == b"\xff\x7f"
    assert set(dm.damage(data, "all_ff")) == {0xFF} and set(dm.damage(data, "all_00")) == {0}
    assert dm.damage(data, "random") != dm.damage(data, "random", 1)


def test_the_position_sets_cover_the_edges(oracle):
    cw = dm.codewords(oracle)
    assert len(cw) == 11 and {(c["w"], c["h"]) for _, _, c in cw} == {(64, 64), (1, 64), (64, 1), (37, 13)}
    long_ = cw[-1][2]
    assert len(long_["data"]) > 8192 and long_["npasses"] == 46
    for name, _, c in cw:
        n, ps = len(c["data"]), dm.positions(len(c["data"]))
        assert {1, 2, 3, 4, 63, 64, n // 2, n - 3, n - 2} <= set(ps) and all(1 <= p <= n - 2 for p in ps), name
        if n >= 514:
            assert {255, 256, 511, 512} <= set(ps), name
    assert sum(len(dm.positions(len(c["data"]))) for _, _, c in cw) == 147
    assert [len(c["data"]) > 514 for _, _, c in cw].count(True) >= 5


def test_a_marker_ends_the_reading_and_every_marker_and_flip_shows(oracle):
    """marker at i: like the damaged bytes cut to [: i + 1]; marker and flip: never the clean decode; ff8f: mostly not the
    decode of a marker at the same place (96 % on this reference; the bound is nine in ten)."""
    markers = flips = ff8f = ff8f_differs = 0
    for name, _, c in dm.codewords(oracle):
        clean = dec(oracle, c)
        for at in dm.positions(len(c["data"])):
            at_90 = None
            for b in dm.MARKER_BYTES:
                bad = dm.damage(c["data"], "marker", at, b)
                v = dec(oracle, dsc.variant(c, data=bad))
                assert np.array_equal(v, dec(oracle, dsc.variant(c, data=bad[:at + 1]))), (name, at, b)
                assert not np.array_equal(v, clean), (name, at, b)
                at_90 = v if b == 0x90 else at_90
                markers += 1
            assert not np.array_equal(dec(oracle, dsc.variant(c, data=dm.damage(c["data"], "flip", at))), clean), (name, at)
            flips += 1
            ff8f_differs += not np.array_equal(dec(oracle, dsc.variant(c, data=dm.damage(c["data"], "ff8f", at))), at_90)
            ff8f += 1
    assert (markers, flips, ff8f) == (441, 147, 147)
    print(f"ff8f differs from marker 0x90 in {ff8f_differs} of {ff8f} places")
    assert ff8f_differs * 10 >= ff8f * 9


@pytest.mark.parametrize("rev", [True, False], ids=["rev", "irr"])
def test_cut_and_behind_cases(oracle, rev):
    """Damaged and cut: the marker lies inside the kept bytes and mostly shows.  Behind the kept passes: it never does."""
    cut = dm.cut_cases(oracle, rev)
    assert {c["npasses"] for c, _ in cut} >= {1, 4} and len(cut) >= 30
    assert all(len(a["data"]) == len(b["data"]) and a["data"] != b["data"] for a, b in cut)
    assert sum(not np.array_equal(dec(oracle, a), dec(oracle, b)) for a, b in cut) * 10 >= len(cut) * 9
    behind = dm.behind_cases(oracle, rev)
    assert len(behind) >= 10 and {c["npasses"] for c, _ in behind} >= {1, 4}
    for a, b in behind:
        assert a["data"] != b["data"] and np.array_equal(dec(oracle, a), dec(oracle, b)), (a["w"], a["h"], a["npasses"])


@pytest.mark.parametrize("rev", [True, False], ids=["rev", "irr"])
def test_the_unlike_wave_is_what_it_says(oracle, rev):
    w = dm.unlike_wave(oracle, rev)
    assert len(w) == 64 and len(w[0]["data"]) > 8192 and (w[63]["w"], w[63]["h"]) == (1, 1)
    clean = {c["data"] for _, c in dm.blocks(oracle, rev)}
    assert [c["data"] in clean for c in w[:63]] == [i % 2 == 0 for i in range(63)]
    depths = {next(i for i in range(len(c["data"]) - 1) if c["data"][i] == 0xFF and c["data"][i + 1] > 0x8F) for c in w[1:63:2]}
    assert len(depths) >= 10 and min(depths) <= 4 and max(depths) >= 512


@pytest.mark.parametrize("style", tc.LASTPASS_STYLES)
def test_damaged_mq_groups_touch_mq_segments_only_and_show(oracle, style):
    cases = tc.damaged_mq_cases(oracle, style)
    info = tc.damaged_mq_info(oracle, style)
    assert len(cases) == len(info) and 20 <= len(cases) <= 300
    kinds = {k for _, k, _ in info}
    # (without termall an MQ-coded segment is followed by a raw one or by nothing: no next MQ byte to set to zero)
    assert kinds == set(tc.DAMAGE_MQ_KINDS) - (set() if style & 4 else {"ff_last_00"})
    differs = {k: [0, 0] for k in kinds}
    restart = 0
    for c, (clean, kind, touched) in zip(cases, info):
        assert c["segs"] == clean["segs"] and len(c["data"]) == len(clean["data"]) and c["data"] != clean["data"]
        # every changed byte lies in an MQ-coded segment
        at, p, spans = 0, 0, []
        for n, k in clean["segs"]:
            spans.append((at, at + n, not (style & 1 and p >= 10 and (p - 1) % 3 != 2)))
            at, p = at + n, p + k
        for i in (i for i in range(len(c["data"])) if c["data"][i] != clean["data"][i]):
            assert next(mq for a, b, mq in spans if a <= i < b), (style, kind, i)
        restart += any(s > 0 for s in touched)
        same = np.array_equal(tc.expected_words(oracle, c, True, style), tc.expected_words(oracle, clean, True, style))
        differs[kind][0] += not same
        differs[kind][1] += 1
    assert restart >= 5
    for k, (d, n) in differs.items():
        assert d * 2 >= n, (style, k, d, n)  # (a segment's last bytes often decide nothing: most cases show, not all)
    assert differs["marker90"][0] and differs["ff8f"][0]


# ------------------------------------------------------------------------------------------------ whole files
FILE_CASES = [(n, m) for n in dm.FILE_NAMES for m in (None,) + dm.FILE_MODES]


def test_the_files_are_as_listed(oracle):
    want_style = {"d1": 0, "d2": 0, "d3": 1, "d4": 5, "d5": 8 | 32, "d6": 4}
    for name in dm.FILE_NAMES:
        data = dm.load(name)
        w, h, nc, prec, _, _, kw = dm.FILES[name]
        i = oracle.decode_info(data)
        assert (i["width"], i["height"], i["ncomp"], i["prec"]) == (w, h, nc, prec) and w <= 128 and h <= 64 and len(data) <= 21000
        assert i["reversible"] == int(kw.get("reversible", True)) and i["mct"] == int(kw.get("mct", False))
        assert oracle.file_blocks(data)["style"] == want_style[name[:2]]
        h_ = lc._main_header(data)
        assert h_["scod"] & 6 == 6  # SOP and EPH
        bodies = dm.packet_bodies(data)
        assert len(bodies) == sum(lc.packets_per_tile_part(data))
        inside = np.zeros(len(data), dtype=bool)
        for a, b in bodies:
            inside[a:b] = True
        for mode in dm.FILE_MODES:
            patch = dm.meta()[name]["modes"][mode]["patch"]
            assert patch and all(inside[off] and 0 <= b <= 255 for off, b in patch), (name, mode)
            bad = dm.patched(name, mode)
            assert bad != data and bad.count(lc.SOP) == data.count(lc.SOP), (name, mode)
            if mode == "random":
                assert len(patch) * 10 >= int(inside.sum()) * 9  # every byte was drawn; a few came out as they were
            if mode in ("marker", "ff_run"):
                assert any(bad[off] == 0xFF and bad[off + 1] > 0x8F for off, _ in patch)
    assert lc._main_header(dm.load(dm.LAYERED))["layers"] == 3 and len(lc.packets_per_tile_part(dm.load(dm.TILED))) == 2


@pytest.mark.parametrize("name,mode", FILE_CASES, ids=[f"{n[:2]}-{m or 'clean'}" for n, m in FILE_CASES])
def test_oracle_decodes_damaged_files_like_the_committed_hashes(oracle, name, mode):
    data = dm.load(name) if mode is None else dm.patched(name, mode)
    want = dm.hashes(name, mode)
    assert sorted(want) == [0, 1]
    for reduce in (0, 1):
        d = oracle.decode(data, reduce)
        assert [sha(d[c].astype(np.int32)) for c in range(d.shape[0])] == want[reduce], (name, mode, reduce)
    if mode is not None:
        assert want[0] != dm.hashes(name)[0], "the damage does not show"


def test_oracle_decodes_damaged_files_like_the_live_library(oracle, opj):
    for name, mode in FILE_CASES:
        data = dm.load(name) if mode is None else dm.patched(name, mode)
        for reduce in (0, 1):
            ref = opj.decode_comps(data, reduce)
            d = oracle.decode(data, reduce)
            assert len(ref) == d.shape[0]
            for c, comp in enumerate(ref):
                assert np.array_equal(d[c], comp["data"]), (name, mode, reduce, c)
                assert sha(comp["data"].astype(np.int32)) == dm.hashes(name, mode)[reduce][c], (name, mode, reduce, c)


def test_layer_cuts_of_the_damaged_layered_file_decode(oracle):
    """What test_decode_damaged.py holds a decode with a layer limit to: strip() of the damaged file reads, and differs by layer."""
    for mode in dm.FILE_MODES:
        bad = dm.patched(dm.LAYERED, mode)
        got = [oracle.decode(lc.strip(bad, L)) for L in (1, 2)] + [oracle.decode(bad)]
        assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2]), mode
