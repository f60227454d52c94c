"""CPU: the references of the guard-bits cases (tests/guard_cases.py) hold, and host Tier-2 alone refuses an over-range frame.

No device runs here.  The classifier is held to the encoder's own block table (j2k_hip_debug_blocks) and to what the oracle's
Tier-2 reads back from the at_limit files; the oracle's files of both classes are libopenjp2's byte for byte; an at_limit file
round-trips, an `over` file does not (the error recorded in the case table is the measurement, the evidence that such a frame
is to be refused); every `over` block fits the slot its band's Mb gives it, so the failure an encode reports is Tier-2's and
not a Tier-1 capacity error; the two places of tier2.cpp that meet a negative zero-bit-plane count both throw."""
import numpy as np
import pytest

import guard_cases as gc

GUARD_TEXT = "code-block has more bit-planes than its sub-band signals (guard bits exceeded)"
J2K_HIP_ERR_OVERFLOW = 4


@pytest.fixture(scope="module")
def api():
    from j2k_amd import api
    return api


def _ids(c):
    return c.name


def test_case_list_holds_what_it_must():
    over, lim = gc.OVER, gc.AT_LIMIT
    plain = [c for c in over if c.nc == 3 and not c.tile and not c.rates and not c.jp2 and c.mask == "checker"]
    assert {(c.prec, c.numres) for c in plain} >= {(8, 2), (8, 3), (16, 2), (16, 3)}
    assert len([c for c in lim if not c.tile]) >= 4 and {c.prec for c in lim} >= {8, 10, 12, 16}
    assert [c.name for c in over if c.tile] == ["over_tiles_8_k2_r2"] and gc.BY_NAME["over_tiles_8_k2_r2"][3:7] == (2, 128, 64, 64)
    assert len([c for c in over if c.rates == (20.0,)]) == 1 and len([c for c in over if c.nc == 4]) == 1 and len([c for c in over if c.jp2]) == 1
    assert all(max(c.w, c.h) <= 128 for c in gc.CASES) and all(c.rev for c in gc.CASES)
    assert len(over) == 11 and len(lim) == 6


@pytest.mark.parametrize("c", gc.CASES, ids=_ids)
def test_classifier_says_what_the_table_expects(oracle, c):
    rows = gc.classify(oracle, c)
    assert gc.verdict(rows) == c.expect
    if c.pattern_tiles is not None:  # only the pattern's tiles reach the class; the benign tile holds no `over` block
        assert {b["tile"] for b in rows if b["cls"] == c.expect and (c.expect == "over" or b["numbps"] == b["Mb"])} >= set(c.pattern_tiles)
        assert {b["tile"] for b in rows if b["cls"] == "over"} <= set(c.pattern_tiles)
    if c.expect == "over":  # one bit-plane too many, never two: Mb + 1 <= the pass tables' 32 bit-planes
        assert max(b["numbps"] - b["Mb"] for b in rows) == 1
    # the benign frame of the same geometry (the handle's next frame in test_guard_bits.py) is in range
    ben = gc.classify_planes(oracle, gc.benign_frame(c), c.prec, c.rev, c.numres, c.tile, tier1=False)
    assert gc.verdict(ben) != "over"


@pytest.mark.parametrize("c", [c for c in gc.AT_LIMIT if c.amp != (1 << c.prec) - 1], ids=_ids)
def test_at_limit_amplitudes_are_the_largest_in_range(oracle, c):
    assert gc.find_amp(oracle, c) == c.amp


@pytest.mark.parametrize("c", gc.CASES, ids=_ids)
def test_block_table_is_the_encoders(oracle, api, c):
    """tile, component, resolution, band, orientation, position, size and Mb of every block, in the order of the encoder's tables."""
    rows = gc.classify(oracle, c)
    want = np.array([[b[k] for k in api.BLOCK_COLUMNS] for b in rows], np.uint32)
    assert np.array_equal(api.frame_blocks(gc.api_params(api, c)), want)


@pytest.mark.parametrize("c", gc.AT_LIMIT, ids=_ids)
def test_at_limit_classifier_agrees_with_the_files_blocks(oracle, c):
    """What the oracle's Tier-2 reads back from the file: the classifier's numbps, block for block; none above Mb, some at it."""
    rows = {(b["tile"], b["comp"], b["res"], b["orient"], b["tx"], b["ty"], b["w"], b["h"]): b for b in gc.classify(oracle, c)}
    fb = oracle.file_blocks(gc.oracle_file(oracle, c))["blocks"]
    assert len(fb) == len([b for b in rows.values() if b["numbps"]])
    zero = 0
    for f in fb:
        b = rows[(f["tile"], f["comp"], f["res"], f["orient"]) + f["rect"]]
        assert f["numbps"] == b["numbps"] <= b["Mb"]
        zero += f["numbps"] == b["Mb"]
    assert zero >= 2  # (zero-bit-plane count 0 in both chroma components)


@pytest.mark.parametrize("c", gc.AT_LIMIT, ids=_ids)
def test_at_limit_file_round_trips(oracle, c):
    assert np.array_equal(oracle.decode(gc.oracle_file(oracle, c)), gc.frame(c))


@pytest.mark.parametrize("c", [c for c in gc.OVER if not c.rates], ids=_ids)  # (a byte budget: not meant to round-trip)
def test_over_file_does_not_round_trip(oracle, c):
    """libopenjp2's "lossless" file of the frame is not the frame: the largest error is the table's."""
    dec = oracle.decode(gc.oracle_file(oracle, c))
    assert not np.array_equal(dec, gc.frame(c))
    assert gc.round_trip_error(oracle, c) == c.max_err


def _opj_file(opj, c):
    pl = gc.frame(c)
    return opj.encode_ext([pl[i] for i in range(c.nc)], prec=c.prec, reversible=c.rev, mct=True, numres=c.numres,
                          tile=(c.tile, c.tile), rates=list(c.rates) if c.rates else None)


@pytest.mark.parametrize("c", gc.CASES, ids=_ids)
def test_oracle_bytes_equal_libopenjp2(oracle, opj, c):
    """Both classes: libopenjp2 writes the `over` frames too, reports success, and the oracle writes the same bytes."""
    from oracle.oracle import strip_com
    ref = _opj_file(opj, c)
    cs = gc.oracle_file(oracle, c)
    if c.jp2:  # (the wrapper is the oracle's own, test_jp2_wrapper.py: the codestream inside it is what is compared)
        cs = cs[cs.index(b"jp2c") + 4:]
        assert cs == gc.oracle_file(oracle, gc.BY_NAME["over_8_k2_r2"])
    if c.rates:  # (a byte budget also pays for the COM segment: the same text on both sides)
        p = gc.oracle_params(c)
        assert oracle.encode_rates(gc.frame(c), p, list(c.rates), comment=opj.comment) == ref
    else:
        assert cs == strip_com(ref)
    if c.expect == "over" and not c.rates:  # ... and libopenjp2's own decode of its file is as wrong as the oracle's
        assert np.array_equal(opj.decode(ref), oracle.decode(strip_com(ref)))
        assert int(np.abs(opj.decode(ref).astype(np.int64) - gc.frame(c)).max()) == c.max_err


@pytest.mark.parametrize("c", gc.OVER, ids=_ids)
def test_over_blocks_fit_their_slots(oracle, api, c):
    """An Mb + 1 block's decisions and codeword stay inside the slot cblk_capacities gives it at the band's Mb (strictly): the
    modeller's checked stores and the coder's capacity checks are never what stops the frame."""
    over = [b for b in gc.classify(oracle, c, want_symbols=True) if b["cls"] == "over"]
    assert over
    for b in over:
        sym_cap, out_cap = api.cblk_capacities(b["w"] * b["h"], b["Mb"])
        assert len(b["t1"]["symbols"]) < sym_cap, (b["comp"], b["res"], len(b["t1"]["symbols"]), sym_cap)
        assert len(b["t1"]["data"]) < out_cap, (b["comp"], b["res"], len(b["t1"]["data"]), out_cap)
        assert 3 * b["numbps"] - 2 <= 96  # (the per-pass tables: kDevMaxPasses)


def _results(oracle, c):
    rows = gc.classify(oracle, c)
    return ([b["numbps"] for b in rows], [b["t1"]["included"] for b in rows], [b["t1"]["length"] for b in rows])


@pytest.mark.parametrize("pricer", [False, True], ids=["packet_writer", "tile_pricer"])
@pytest.mark.parametrize("c", [c for c in gc.OVER if not c.jp2], ids=_ids)
def test_host_tier2_refuses_over_blocks(oracle, api, c, pricer):
    """plan_codestream's packet writer and TilePricer's constructor, on the oracle's results of the frame's blocks."""
    with pytest.raises(api.J2kHipError) as ei:
        api.host_tier2(gc.api_params(api, c), *_results(oracle, c), pricer=pricer)
    assert ei.value.code == J2K_HIP_ERR_OVERFLOW and GUARD_TEXT in str(ei.value)


@pytest.mark.parametrize("c", gc.AT_LIMIT, ids=_ids)
def test_host_tier2_takes_at_limit_blocks(oracle, api, c):
    """The other side of the edge: zero-bit-plane count 0 plans a codestream of exactly the oracle's length, and prices."""
    assert api.host_tier2(gc.api_params(api, c), *_results(oracle, c)) == len(gc.oracle_file(oracle, c))
    assert api.host_tier2(gc.api_params(api, c), *_results(oracle, c), pricer=True) == 0
    # one bit-plane more on one at_limit block is refused
    nb, npass, ln = _results(oracle, c)
    k = next(i for i, b in enumerate(gc.classify(oracle, c)) if b["cls"] == "at_limit")
    nb[k] += 1
    with pytest.raises(api.J2kHipError, match="guard bits exceeded"):
        api.host_tier2(gc.api_params(api, c), nb, npass, ln)


def test_no_97_frame_of_the_family_goes_over(oracle):
    """The 9/7 / ICT search over gc.SEARCH_97_FAMILY (DESIGN section 8 names it): the irreversible colour transform does not double
    the chroma range, and no block of the 720 frames comes closer to its Mb than one bit-plane."""
    tried, found, margin = gc.search_97(oracle)
    assert tried == 720 and found == [] and margin == 1
