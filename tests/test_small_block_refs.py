"""CPU: the references of the small code-block / small precinct cases (tests/small_block_cases.py) agree with each other.

Every file of the table is written by the oracle's encoder.  libopenjp2's decoder and the oracle's decoder must return the
same samples from it at full and at half size, and the input itself from every reversible file without a byte budget.  The
oracle's bytes are held against libopenjp2's encoder only where that encoder can be asked (cases.safe_for_opj_encoder: style
0, no precinct below 8) -- outside it refuses most cases and crashes on some, so nothing here calls it there.  The table must
still hold what its names claim (1 x 1 code-blocks, a precinct band of more than 64 blocks, more than 1000 packets in a tile, a
frame of at least 8192 blocks), the PCRL / CPRL goldens decode to their committed hashes with both decoders, and the
parameters outside the accepted range are refused on the host (no device work)."""
import hashlib

import numpy as np
import pytest

import small_block_cases as cases
from j2k_amd import api

ALL = cases.CASES + [cases.REGION_EXTRA]
SAFE = [c for c in ALL if cases.safe_for_opj_encoder(c)]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.int32).tobytes()).hexdigest()


def _opj_planes(opj, data, red):
    return np.stack([c["data"] for c in opj.decode_comps(data, red)])


@pytest.mark.parametrize("c", ALL, ids=lambda c: c.name)
def test_libopenjp2_and_the_oracle_decode_the_oracles_file_alike(oracle, opj, c):
    cs = cases.oracle_file(oracle, c)
    for red in (0, 1):
        ours = oracle.decode(cs, red)
        assert ours.shape == (c.nc, -(-c.h >> red), -(-c.w >> red))
        assert np.array_equal(ours, _opj_planes(opj, cs, red)), (c.name, red)
    if c.rev and not c.rates:
        assert np.array_equal(oracle.decode(cs, 0), cases.planes(c))


@pytest.mark.parametrize("c", [c for c in ALL if c.rev and not c.rates], ids=lambda c: c.name)
def test_reversible_files_are_lossless_without_libopenjp2(oracle, c):
    assert np.array_equal(oracle.decode(cases.oracle_file(oracle, c), 0), cases.planes(c))


@pytest.mark.parametrize("c", SAFE, ids=lambda c: c.name)
def test_oracle_bytes_equal_libopenjp2_in_the_safe_subset(oracle, opj, c):
    from oracle.oracle import strip_com
    assert cases.safe_for_opj_encoder(c) and c.style == 0 and all(min(p) >= 8 for p in (c.precincts or ()))
    pl = cases.planes(c)
    ref = opj.encode_ext([pl[i] for i in range(c.nc)], prec=c.prec, reversible=c.rev, mct=c.nc >= 3, numres=c.numres, cblk=c.cblk,
                         tile=(c.tile, c.tile), prog=c.prog, precincts=list(c.precincts) if c.precincts else None,
                         rates=list(c.rates) if c.rates else None)
    if c.rates:  # (a byte budget also pays for the COM segment: the same text on both sides)
        assert cases.oracle_file(oracle, c, comment=opj.comment) == ref
    else:
        assert cases.oracle_file(oracle, c) == strip_com(ref)


def test_safe_subset_never_names_a_case_libopenjp2_cannot_encode():
    assert len(SAFE) >= 60
    for c in ALL:
        if c.style or any(min(p) < 8 for p in (c.precincts or ())):
            assert c not in SAFE, c.name


# -- the table still holds what it claims ----------------------------------------------------------------------------------------
def test_table_has_every_size_pair_spec_style_and_rate_set():
    by_kind = {k: [c for c in cases.CASES if c.kind == k] for k in cases.KINDS}
    sizes = by_kind["size"]
    assert {(c.cblk, c.nc) for c in sizes} == {((a, b), nc) for a in cases.SIDES for b in cases.SIDES for nc in (3, 1)}
    assert all(c.w % 2 and c.h % 2 and c.w % 4 and c.h % 4 and c.numres in (3, 4) and c.precincts is None for c in sizes)
    assert all((c.nc, c.prec, c.rev) in ((3, 8, True), (1, 12, False), (1, 16, False)) for c in sizes)
    assert {c.prec for c in sizes} == {8, 12, 16} and {c.prog for c in sizes} == {0, 1, 2, 3, 4} and {c.numres for c in sizes} == {3, 4}
    prec = by_kind["precinct"]
    assert {(c.precincts, c.cblk) for c in prec} == {(tuple(s), cb) for s, _ in cases.PRECINCT_SPECS.values() for cb in cases.PRECINCT_CBLKS}
    assert {(c.precincts, c.cblk) for c in prec if c.tile == 40 and (c.w, c.h) == (90, 61)} == {(c.precincts, c.cblk) for c in prec}
    assert all(c.prog <= 2 and not c.style and not c.rates for c in prec)
    for c in prec:  # nothing below 2 above the lowest resolution
        assert all(pw >= 2 and ph >= 2 for pw, ph in cases.precinct_sizes(c)[1:]), c.name
    assert {c.precincts: c.numres for c in prec if c.precincts in (((4, 4),), ((2, 2),)) and not c.rev and not c.tile} == {((4, 4),): 3, ((2, 2),): 2}
    sty = by_kind["style"]
    assert {(c.style, c.cblk, c.rev) for c in sty} == {(s, cb, r) for s in cases.STYLES for cb in cases.STYLE_CBLKS for r in (True, False)}
    assert all(not c.rates for c in sty)
    rat = by_kind["rates"]
    assert {c.cblk for c in rat} == set(cases.RATE_CBLKS) and {len(c.rates) for c in rat} == {1, 2, 3}
    assert any(c.rates[-1] == 0 for c in rat) and {(c.w, c.h) for c in rat} == {(150, 100), (97, 131)}
    many = by_kind["many"]
    assert {(c.rev, c.rates) for c in many} == {(r, q) for r in (True, False) for q in (None, tuple(cases.MANY_RATES))}
    assert all((c.w, c.h, c.nc, c.prec, c.cblk) == (300, 200, 3, 8, (4, 4)) for c in many)
    for name in cases.ENTRY_POINT_NAMES + cases.REGION_NAMES:
        assert name in cases.BY_NAME
    assert sum(cases.BY_NAME[n].nc >= 3 for n in cases.ENTRY_POINT_NAMES) >= 4 and len(cases.ENTRY_POINT_NAMES) == 6


def test_table_reaches_one_by_one_blocks_deep_tag_trees_many_packets_and_8192_blocks(oracle):
    """Counted from the oracle's own block list where a block must hold passes (oracle.file_blocks), from the layout of
    T.800 B.5 - B.7 otherwise."""
    c = cases.BY_NAME["prec_p2_4x4_rgb8_53"]
    blocks = oracle.file_blocks(cases.oracle_file(oracle, c))["blocks"]
    assert sum(b["w"] == 1 and b["h"] == 1 for b in blocks) >= 1000 and all(b["w"] * b["h"] == 1 for b in blocks if b["res"] > 0)
    lay = cases.layout(c)
    assert len(lay) == 1 and lay[0]["packets"] > 1000  # packets in one tile
    assert any(t["packets"] > 1000 for cc in cases.CASES if cc.tile for t in cases.layout(cc))  # ... and in a tile of a tiled frame
    for c in cases.MANY:
        fb = oracle.file_blocks(cases.oracle_file(oracle, c))
        assert len(fb["blocks"]) >= 8192, (c.name, len(fb["blocks"]))
        grids = [g for t in cases.layout(c) for g in t["grids"]]
        assert max(a * b for a, b in grids) > 64 and (38, 25) in grids  # one precinct band of 38 x 25 blocks: a tag tree of seven levels
        # (the layout worked out here and the oracle's Tier-2 agree on the blocks' sizes)
        count = {}
        for wh in (bl for t in cases.layout(c) for bl in t["blocks"]):
            count[wh] = count.get(wh, 0) + 1
        for b in fb["blocks"]:
            count[(b["w"], b["h"])] -= 1
        assert min(count.values()) >= 0
    # the rate-controlled small frames leave blocks out of the first layers: precinct bands of more than 64 blocks there too
    assert any(a * b > 64 for c in cases.CASES if c.kind == "rates" for t in cases.layout(c) for a, b in t["grids"])


@pytest.mark.parametrize("c", [c for c in ALL if c.kind in ("precinct", "region")], ids=lambda c: c.name)
def test_layout_agrees_with_the_oracles_block_list(oracle, c):
    fb = oracle.file_blocks(cases.oracle_file(oracle, c))
    lay = cases.layout(c)
    assert fb["ntiles"] == len(lay)
    count = {}
    for wh in (bl for t in lay for bl in t["blocks"]):
        count[wh] = count.get(wh, 0) + 1
    for b in fb["blocks"]:
        assert count.get((b["w"], b["h"]), 0) > 0, (c.name, b["rect"])
        count[(b["w"], b["h"])] -= 1


# -- the PCRL / CPRL goldens -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.EXT_NAMES)
def test_ext_goldens_decode_to_their_hashes_with_the_oracle(oracle, name):
    g, data = cases.ext_entry(name), cases.ext_bytes(name)
    assert len(data) == g["length"] <= 11 * 1024 and hashlib.sha256(data).hexdigest() == g["sha256"]
    assert g["ext"]["prog"] in (3, 4) and min(min(p) for p in g["ext"]["precincts"]) >= 8
    for red in (0, 1):
        dec = oracle.decode(data, red)
        assert [_sha(dec[i]) for i in range(g["ncomp"])] == [d["sha256"] for d in g["decoded_comps"][str(red)]], (name, red)
    assert np.array_equal(oracle.decode(data, 0), cases.ext_planes(name))


@pytest.mark.parametrize("name", cases.EXT_NAMES)
def test_ext_goldens_decode_to_their_hashes_with_libopenjp2(opj, name):
    g, data = cases.ext_entry(name), cases.ext_bytes(name)
    for red in (0, 1):
        comps = opj.decode_comps(data, red)
        assert [_sha(c["data"]) for c in comps] == [d["sha256"] for d in g["decoded_comps"][str(red)]], (name, red)


def test_ext_goldens_come_in_both_orders():
    pairs = {}
    for name in cases.EXT_NAMES:
        kw = cases.ext_entry(name)["ext"]
        pairs.setdefault((tuple(map(tuple, kw["precincts"])), tuple(kw["cblk"])), set()).add(kw["prog"])
    assert pairs == {(((8, 8),), (4, 4)): {3, 4}, (((16, 8),), (8, 4)): {3, 4}, (((32, 32), (8, 8)), (64, 64)): {3, 4}}


# -- refusals (host only) --------------------------------------------------------------------------------------------------------
HALVES_TO_ONE = [((4, 4), 4), ((2, 2), 3), ((4, 16), 4), ((16, 4), 4), ((8, 8), 5), ((1, 8), 2), ((8, 1), 2)]


@pytest.mark.parametrize("size,numres", HALVES_TO_ONE, ids=lambda v: str(v).replace(" ", ""))
def test_precinct_spec_that_halves_to_one_above_the_lowest_resolution_is_refused(size, numres):
    with pytest.raises(api.J2kHipError) as ei:
        api.main_header(api.make_params(67, 45, 3, 8, num_resolutions=numres, cblk=(4, 4), precincts=[size]))
    assert ei.value.code == 1 and "precinct size below 2" in str(ei.value)  # J2K_HIP_ERR_PARAM
    # one resolution fewer keeps 2 above the lowest: accepted
    if min(size) >= 2:
        assert api.main_header(api.make_params(67, 45, 3, 8, num_resolutions=numres - 1, cblk=(4, 4), precincts=[size]))[:2] == b"\xff\x4f"


def test_file_with_a_precinct_of_one_above_the_lowest_resolution_is_rejected_by_read_info(oracle):
    """The oracle's encoder writes such a spec; the header reader refuses the file (no handle, no device)."""
    from oracle.oracle import make_params
    c = cases.BY_NAME["prec_p4_4x4_rgb8_53"]
    pl = cases.planes(c)
    good = oracle.encode(pl, make_params(c.w, c.h, c.nc, c.prec, mct=True, numres=3, cblk=(4, 4), precincts=[(4, 4)]))
    assert api.read_info(good)["num_resolutions"] == 3
    bad = oracle.encode(pl, make_params(c.w, c.h, c.nc, c.prec, mct=True, numres=4, cblk=(4, 4), precincts=[(4, 4)]))
    with pytest.raises(api.J2kHipError) as ei:
        api.read_info(bad)
    assert ei.value.code == 1 and "precinct of size 1 above the lowest resolution" in str(ei.value)


@pytest.mark.parametrize("cblk", [(2, 4), (4, 2), (2, 2), (128, 4), (4, 128), (128, 128)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_code_block_sides_2_and_128_are_refused(cblk):
    with pytest.raises(api.J2kHipError) as ei:
        api.main_header(api.make_params(67, 45, 3, 8, num_resolutions=3, cblk=cblk))
    assert ei.value.code == 1 and "code-block size" in str(ei.value)


@pytest.mark.parametrize("cblk", [(4, 4), (4, 64), (64, 4), (8, 8)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_smallest_code_blocks_are_accepted_and_written_to_the_header(cblk):
    h = api.main_header(api.make_params(67, 45, 3, 8, num_resolutions=3, cblk=cblk, comment=""))
    cod = h.index(b"\xff\x52")
    assert (h[cod + 10], h[cod + 11]) == (cblk[0].bit_length() - 3, cblk[1].bit_length() - 3)
