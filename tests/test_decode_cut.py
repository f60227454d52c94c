"""GPU: files cut short through the whole decode -- Tier-2 planner, gather, Tier-1, IDWT, output -- against the plain-C oracle's
decode of the same bytes (pinned to libopenjp2 where libopenjp2 decodes a cut: test_decode_cut_refs.py), sample for sample.
The cases are tests/cut_cases.py's.  What a complete file never exercises: blocks whose header arrived without their body,
segment tables longer than the passes that arrived, packets of which the first blocks are kept and later ones dropped, tiles
without a tile-part (their samples are component value 0, as libopenjp2 delivers them), and arenas that still hold the
previous frame."""
import hashlib

import numpy as np
import pytest

import compare_model as cm
import cut_cases as cc
import rgba_model as rm
from conftest import golden_case
from j2k_amd import api, synth

pytestmark = pytest.mark.gpu

J2K_HIP_ERR_PARAM = 1


@pytest.fixture(scope="module")
def enc():
    e = api.Encoder(0)
    yield e
    e.close()


@pytest.fixture
def knobs():
    """Sets tuning knobs for one test and puts back what they were."""
    before = {}

    def tune(key, value):
        before.setdefault(key, api.get_tune(key))
        api.tune(key, value)
    yield tune
    for k, v in before.items():
        api.tune(k, v)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.int32).tobytes()).hexdigest()


def _live():
    try:
        from oracle.oracle import OpjReplay
        return OpjReplay()
    except OSError:
        return None


def case_of(tag, label):
    return next(c for c in cc.cases(tag) if c["label"] == label)


def half_parts(tag):
    """The boundary cut that keeps half of the file's tile-parts, with an EOC."""
    n = len(cc.walk(cc.load(tag))["parts"])
    return case_of(tag, f"parts{n // 2}of{n}+eoc")


def check_planar(enc, oracle, case, subs=(1, 2)):
    data = cc.cut_bytes(case)
    for s in subs:
        got = enc.decode_planar(data, subsample=s)
        want = cc.expected(oracle, case, s.bit_length() - 1)
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            c, y, x = bad[0]
            raise AssertionError(f"{case['id']}, subsample {s}: {len(bad)} samples differ, first at component {c}, ({x}, {y}): {got[c, y, x]} for "
                                 f"{want[c, y, x]}; tiles without a tile-part: {cc.missing_tiles(case['tag'], case)}")


@pytest.mark.parametrize("tag", list(cc.ORACLE_FILES) + list(cc.REPACKS))
def test_planar_decode_equals_the_oracle(enc, oracle, tag):
    """Every cut of the file at full and half size; a cut the oracle refuses is refused with J2K_HIP_ERR_PARAM, and the handle
    decodes the complete file correctly afterwards."""
    decoded = refused = 0
    for case in cc.cases(tag):
        if cc.decodes(oracle, case):
            check_planar(enc, oracle, case)
            decoded += 1
            continue
        with pytest.raises(api.J2kHipError) as e:
            enc.decode_planar(cc.cut_bytes(case))
        assert e.value.code == J2K_HIP_ERR_PARAM, case["id"]
        refused += 1
        whole = cc.load(cc.REPACKS[tag][0] if tag in cc.REPACKS else tag)
        assert np.array_equal(enc.decode_planar(cc.load(tag)), oracle.decode(whole)), case["id"]
    assert decoded and decoded >= 4 * refused


@pytest.mark.parametrize("tag", list(cc.OPJ_FILES))
def test_planar_decode_equals_libopenjp2_where_the_oracle_does_not_read(enc, tag):
    """Whole tile-parts plus an EOC of the sub-sampled, cinema and five-component files and of a multi-tile file declared signed:
    the committed hashes of libopenjp2's decode (tests/golden/cut/cut.json), and the library itself where one is installed.
    The decode delivers the first four components, each replicated onto the image's grid."""
    g, lib = cc.golden()["cases"], _live()
    for case in cc.cases(tag):
        data = cc.cut_bytes(case)
        info = api.read_info(data)
        for s in (1, 2):
            got = enc.decode_planar(data, subsample=s)
            want = g[case["id"]]["decoded"][str(s.bit_length() - 1)]
            live = lib.decode_comps(data, s.bit_length() - 1) if lib else None
            for c in range(got.shape[0]):
                own = cm.own_grid(got[c], (info["sub_x"][c], info["sub_y"][c])).astype(np.int32)
                if info["comp_signed"][c]:  # (delivered with the offset 2^(depth - 1) that makes it unsigned)
                    own -= 1 << (info["comp_depth"][c] - 1)
                assert list(own.shape) == want[c]["shape"] and sha(own) == want[c]["sha256"], (case["id"], s, c)
                if live:
                    assert np.array_equal(own, live[c]["data"]), (case["id"], s, c)


@pytest.mark.parametrize("lanes", [0, 2], ids=["wave-per-block", "lane-per-block"])
@pytest.mark.parametrize("tag", cc.STYLED)
def test_both_tier1_kernels(enc, oracle, knobs, tag, lanes):
    """The styled and layered files under `t1dec_lanes` 0 and 2 (test_decode.py: test_both_tier1_decoders_agree_with_libopenjp2)."""
    knobs("t1dec_lanes", lanes)
    for case in cc.cases(tag):
        if cc.decodes(oracle, case):
            check_planar(enc, oracle, case, subs=(1,))


@pytest.mark.parametrize("tag", ["g4", "s4", "r8", "l4"])
def test_reused_handle_holds_nothing_of_the_previous_frame(oracle, tag):
    """One handle: the complete file, then each of its cuts -- every result is the oracle's, and a fresh handle's."""
    cases = [c for c in cc.cases(tag) if cc.decodes(oracle, c)]
    picks = [cases[0], cases[len(cases) // 2], cases[-1]]
    e = api.Encoder(0)
    try:
        assert np.array_equal(e.decode_planar(cc.load(tag)), oracle.decode(cc.load(tag)))
        for case in cases:
            check_planar(e, oracle, case, subs=(1,))
        reused = [e.decode_planar(cc.cut_bytes(c)) for c in picks]  # (each behind another cut's decode)
    finally:
        e.close()
    for case, got in zip(picks, reused):
        fresh = api.Encoder(0)
        try:
            assert np.array_equal(fresh.decode_planar(cc.cut_bytes(case)), got), case["id"]
        finally:
            fresh.close()


def test_smaller_cut_file_after_a_larger_complete_one(oracle):
    e = api.Encoder(0)
    try:
        assert np.array_equal(e.decode_planar(cc.load("g4")), oracle.decode(cc.load("g4")))
        for case in (half_parts("g9"), case_of("g9", "first-3of7"), case_of("g9", "last-sod")):
            check_planar(e, oracle, case)
    finally:
        e.close()


def _windows(tag, case, reduce):
    """A window that straddles an arrived and a missing tile, and one off the block grid inside the first tile (half-arrived in
    a cut inside its tile-part)."""
    w = cc.walk(cc.load(tag))
    W, H = -(-w["size"][0] >> reduce), -(-w["size"][1] >> reduce)
    out = []
    missing = cc.missing_tiles(tag, case)
    if missing:
        x0, y0, _, _ = cc.tile_rect(w, missing[0], reduce)
        x, y = max(x0 - 37, 0), max(y0 - 29, 0)
        out.append((x, y, min(83, W - x), min(61, H - y)))
    _, _, x1, y1 = cc.tile_rect(w, 0, reduce)
    out.append((5, 7, min(x1 - 11, 71), min(y1 - 9, 45)))
    return out


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_window_decode(enc, oracle, device):
    for tag, case in (("g4", half_parts("g4")), ("g4", case_of("g4", "first-3of7")), ("u9", half_parts("u9")), ("s4", case_of("s4", "last-2of7"))):
        data = cc.cut_bytes(case)
        for s in (1, 2):
            want = cc.expected(oracle, case, s.bit_length() - 1)
            for rect in _windows(tag, case, s.bit_length() - 1):
                x, y, w, h = rect
                got = enc.decode_region_planar(data, rect, subsample=s, device=device)
                assert np.array_equal(got, want[:, y:y + h, x:x + w]), (case["id"], s, rect)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("bits", [8, 16])
def test_rgba_decode(enc, oracle, bits, device):
    """A multi-tile cut (missing tiles get the model's value for component value 0, alpha is filled as the model fills it) and
    a cut in the middle of a packet of the seven-layer RGBA file."""
    for case in (half_parts("g4"), case_of("r8", "first-3of7")):
        data = cc.cut_bytes(case)
        dec = cc.expected(oracle, case)
        info = api.read_info(data)
        nc, h, w = dec.shape
        planes = rm.rgba(api.rgba_mode(data), list(dec), [info["depth"]] * nc, [(1, 1)] * nc, w, h, bits, bits)
        _, lay = synth.ae_frame(np.zeros((3, h, w), dtype=np.int32), bits, row_pad_bytes=8)
        frame = np.full(h * lay["rowbytes"], 0xA5, dtype=np.uint8)
        want = rm.into_ae_frame(frame, lay, planes)
        got = enc.decode_rgba(data, frame.copy(), lay, w, h, device=device)
        assert np.array_equal(got, want), (case["id"], bits, device)


@pytest.mark.parametrize("group", [0, 1], ids=["grouped", "frame-by-frame"])
def test_sequence_decode(enc, oracle, knobs, group):
    """Every frame of a sequence equals its decode alone: a cut frame's missing tile shows nothing of its neighbours."""
    knobs("decseq_group", group)
    whole = dict(tag="g4", kind="a", label="whole", end=len(cc.load("g4")), eoc=False, twin=None, id="g4-whole")
    a, b = half_parts("g4"), case_of("g4", "last-4of7")
    for frames in ([whole, a, whole], [a, b], [b, whole, a]):
        out = enc.decode_sequence_planar([cc.cut_bytes(c) for c in frames])
        for f, c in enumerate(frames):
            assert np.array_equal(out[f], cc.expected(oracle, c)), (group, [x["id"] for x in frames], f)


def test_compare_against_the_oracles_planes(enc, oracle, golden):
    """j2k_hip_compare on cut files: the sums computed in numpy (compare_model.py) from the source and the ORACLE's decode --
    test_compare.py's model is fed by the decode under test.  The file is lossless, so in the multi-tile cut every difference,
    the first one included, lies inside a missing tile."""
    g, pl, _, cs = golden_case(golden, "g4_300x200_rgb16_53_rct_tile128")
    assert cs == cc.load("g4")
    p = api.make_params(g["width"], g["height"], g["ncomp"], g["prec"], reversible=True, ycc=True, tile_size=128, comment="")
    frame, lay = synth.ae_frame(pl, g["prec"], row_pad_bytes=8)
    w = cc.walk(cs)
    for case in (half_parts("g4"), case_of("g4", "first-3of7"), case_of("g4", "len-2")):
        data = cc.cut_bytes(case)
        want = cm.diffs(list(pl), list(cc.expected(oracle, case)), g["prec"])
        assert enc.compare(data, p, planar=pl) == want, case["id"]
        assert enc.compare_device(data, p, frame=frame, layout=lay) == want, case["id"]
    case = half_parts("g4")
    rects = [cc.tile_rect(w, t) for t in cc.missing_tiles("g4", case)]
    for d in cm.diffs(list(pl), list(cc.expected(oracle, case)), g["prec"]):
        assert d["differing"] > 0 and any(x0 <= d["first_x"] < x1 and y0 <= d["first_y"] < y1 for x0, y0, x1, y1 in rects)
