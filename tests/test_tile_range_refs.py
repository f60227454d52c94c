"""CPU: what the reference of the tile-range sweep (tests/tile_range_cases.py, tests/test_tile_ranges.py) must satisfy.

For every configuration and every kind of samples its views carry: the oracle encodes it, its codestream splits into one
tile-part per tile with SOT indices 0 .. n - 1, the header is the one api.main_header writes (so main header + the ranges'
tile-parts + EOC is the whole file), a lossless configuration decodes back to the samples, and -- where a libopenjp2 is installed
and its encoder may be asked (style 0) -- the bytes are libopenjp2's.  The channel views, read back by numpy through base /
colbytes / rowbytes alone, hold the samples the reference was made from; the range lists reach every kind of working box; the
poisoned copies of a host frame differ from it in every byte outside the rows a range may read."""
import numpy as np
import pytest

import depth_cases
import tile_range_cases as tc
from j2k_amd import api, sharding

KINDS = sorted({(c.name, tc.KIND[v]) for c, v in tc.PAIRS})
LOSSLESS = [(n, k) for n, k in KINDS if tc.BY_NAME[n].rev and not tc.BY_NAME[n].rates]
SAFE = [c for c in tc.CONFIGS if tc.safe_for_opj_encoder(c)]


def test_table_is_the_one_the_sweep_claims():
    assert {g.id: (g.w, g.h, g.nc, g.prec, g.tile, g.numres) for g in tc.GEOS.values()} == {
        "A": (133, 100, 3, 8, 33, 3), "B": (150, 110, 3, 8, 40, 4), "C": (150, 130, 1, 16, 64, 5), "D": (199, 101, 3, 10, 100, 6),
        "E": (130, 129, 3, 8, 128, 6), "F": (135, 102, 4, 16, 33, 3)}
    assert {g.id: tc.grid(g) for g in tc.GEOS.values()} == {"A": (5, 4), "B": (4, 3), "C": (3, 3), "D": (2, 2), "E": (2, 2), "F": (5, 4)}
    assert {(c.geo.id, c.rev, c.mct) for c in tc.BASE} == {("A", True, True), ("B", True, True), ("B", False, True), ("C", False, False),
                                                            ("D", True, False), ("E", False, True), ("F", False, True)}
    assert all(c.geo.id == "B" for c in tc.VARIANTS)
    assert {c.prog for c in tc.VARIANTS if c.layers == 2 and not c.rates} == {0, 1, 2, 3, 4}
    assert any(c.prog == 2 and c.precincts == ((32, 32),) and c.layers == 3 for c in tc.VARIANTS)
    assert any(c.cblk == (16, 16) and c.style == 5 for c in tc.VARIANTS)
    assert any(c.rates == (20.0, 5.0) and not c.rev for c in tc.VARIANTS)
    # every geometry gets the first view, every view at least A and B
    for c in tc.CONFIGS:
        assert (c, "ae") in tc.PAIRS
    for v in tc.VIEWS:
        assert {"A", "B"} <= {c.geo.id for c, vv in tc.PAIRS if vv == v and c in tc.BASE}, v
    # 1-sample edge tiles, edge tiles of 2 and 3 samples
    assert tc.tile_rect(tc.GEOS["A"], 19) == (132, 99, 133, 100) and tc.tile_rect(tc.GEOS["D"], 3) == (100, 100, 199, 101)
    assert tc.tile_rect(tc.GEOS["E"], 3) == (128, 128, 130, 129) and tc.tile_rect(tc.GEOS["F"], 19) == (132, 99, 135, 102)


@pytest.mark.parametrize("name,kind", KINDS, ids=[f"{n}-{k}" for n, k in KINDS])
def test_oracle_file_splits_into_one_tile_part_per_tile(oracle, name, kind):
    c = tc.BY_NAME[name]
    cs, hdr, parts = tc.reference(oracle, c, kind)
    ntx, nty = tc.grid(c.geo)
    assert len(parts) == ntx * nty == tc.ntiles(c.geo)
    assert all(p[:2] == b"\xff\x90" for p in parts)
    assert [int.from_bytes(p[4:6], "big") for p in parts] == list(range(len(parts)))
    assert all(p[10] == 0 and p[11] == 1 for p in parts)  # TPsot 0 of TNsot 1: one tile-part per tile
    p = tc.api_params(api, c, promote=kind == "promote")
    assert api.main_header(p) == hdr
    assert sharding.assemble(p, parts) == cs == sharding.assemble(hdr, parts)
    i = oracle.decode_info(cs)
    assert (i["width"], i["height"], i["ncomp"], i["prec"], i["numres"]) == (c.geo.w, c.geo.h, c.geo.nc, c.geo.prec, c.geo.numres)


@pytest.mark.parametrize("name,kind", LOSSLESS, ids=[f"{n}-{k}" for n, k in LOSSLESS])
def test_lossless_configurations_decode_back_to_the_samples(oracle, name, kind):
    c = tc.BY_NAME[name]
    assert np.array_equal(oracle.decode(tc.oracle_file(oracle, c, kind), 0), tc.samples(c.geo, kind))


def test_sample_kinds_give_different_files(oracle):
    """A view that reached the encoder as another view's samples would not pass by accident."""
    for c in tc.BASE:
        kinds = sorted({tc.KIND[v] for cc, v in tc.PAIRS if cc is c})
        files = [tc.oracle_file(oracle, c, k) for k in kinds]
        assert len(set(files)) == len(files), c.name
        for k in kinds:  # ... nor as the same samples upside down
            assert not np.array_equal(tc.samples(c.geo, k), tc.samples(c.geo, k)[:, ::-1])


@pytest.mark.parametrize("c", SAFE, ids=lambda c: c.name)
def test_oracle_bytes_equal_libopenjp2(oracle, opj, c):
    from oracle.oracle import strip_com
    g = c.geo
    pl = tc.samples(g, "ae")
    ref = opj.encode_ext([pl[i] for i in range(g.nc)], prec=g.prec, reversible=c.rev, mct=c.mct, numres=g.numres, cblk=c.cblk, layers=c.layers,
                         tile=(g.tile, g.tile), prog=c.prog, precincts=list(c.precincts) if c.precincts else None,
                         rates=list(c.rates) if c.rates else None)
    if c.rates:  # (a byte budget also pays for the COM segment: the same text on both sides)
        assert tc.oracle_file(oracle, c, "ae", comment=opj.comment) == ref
    else:
        assert tc.oracle_file(oracle, c) == strip_com(ref)


def test_only_styled_configurations_stay_away_from_libopenjp2s_encoder():
    assert [c.name for c in tc.CONFIGS if c not in SAFE] == ["B_53_rct_cblk16_bypass_termall"]


# -- the channel views -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv", tc.PAIRS, ids=tc.pair_id)
def test_views_hold_the_samples_of_the_reference(cv):
    """numpy's own reading of base / colbytes / rowbytes, then Promote and CopyChannel as depth_cases models them."""
    c, view = cv
    g, src = c.geo, tc.source(c.geo, view)
    st = tc.read_back(g, src)
    if src.promote:
        st = depth_cases.promote(st)
    got = np.stack([depth_cases.convert(st[k], src.chans[k].depth, g.prec) for k in range(g.nc)])
    assert np.array_equal(got, tc.samples(g, tc.KIND[view]))
    assert len(src.chans) == g.nc and src.promote == (view == "promote") and src.knobs == (dict(no_fuse=1) if view == "ae_nofuse" else {})
    for ch in src.chans:
        # every sample of every row lies inside the buffer
        corners = [ch.off + y * ch.rowbytes + x * ch.colbytes for y in (0, g.h - 1) for x in (0, g.w - 1)]
        assert min(corners) >= 0 and max(corners) + ch.sample_bytes <= src.buf.size
        assert abs(ch.rowbytes) > g.w * ch.colbytes  # padded rows
        assert (ch.rowbytes < 0) == view.endswith("bottomup")
        if view.startswith("planar"):
            assert (ch.colbytes, ch.sample_bytes, ch.depth) == (2, 2, 10) and abs(ch.rowbytes) == 2 * g.w + tc.PLANAR_PAD
        else:
            assert ch.colbytes == 4 * ch.sample_bytes and ch.rowbytes % ch.colbytes == 0 and ch.depth == 8 * ch.sample_bytes
    if view == "promote":
        assert st.max() == 65535 and tc.read_back(g, src).max() == 32768


@pytest.mark.parametrize("cv", [cv for cv in tc.PAIRS if cv[0] in tc.BASE], ids=tc.pair_id)
def test_poisoned_frames_keep_the_rows_of_the_box_and_nothing_else(cv):
    c, view = cv
    g, src = c.geo, tc.source(c.geo, view)
    _, nty = tc.grid(g)
    row = min(1, nty - 1)
    y0, y1 = row * g.tile, min((row + 1) * g.tile, g.h)
    p = tc.poisoned(g, src, y0, y1)
    a, b = tc.read_back(g, src), tc.read_back(g, src._replace(buf=p))
    assert np.array_equal(a[:, y0:y1], b[:, y0:y1])
    assert (a[:, :y0] != b[:, :y0]).all() and (a[:, y1:] != b[:, y1:]).all() and y0 > 0
    changed = p != src.buf
    assert ((p ^ src.buf)[changed] == tc.POISON).all() and changed.sum() >= src.buf.size - (y1 - y0) * g.w * g.nc * 2


# -- ranges, boxes, partitions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", list(tc.GEOS.values()), ids=lambda g: g.id)
def test_range_lists_reach_every_kind_of_box(g):
    n, (ntx, nty) = tc.ntiles(g), tc.grid(g)
    r = tc.ranges(g)
    assert len(set(r)) == len(r) and all(c >= 1 and f + c <= n for f, c in r)
    assert {(t, 1) for t in range(n)} <= set(r) and (0, n) in r
    if n <= 12:
        assert len(r) == n * (n + 1) // 2
    else:
        assert {c for _, c in r} == {1, 2, ntx, ntx + 1, n} and all((f, c) in r for c in (2, ntx, ntx + 1) for f in range(n - c + 1))
    kinds = {}
    for f, c in r:
        kinds.setdefault(tc.box_kind(g, f, c), []).append((f, c))
    # (a row of two tiles has no run that is not the whole row)
    assert set(kinds) == {"single", "single_interior", "crosses_row_end", "whole_rows"} | ({"row_run"} if ntx > 2 else set())
    # a box with both origins non-zero, a box that holds a tile nobody asked for
    assert any(tc.box(g, f, c)[0] > 0 and tc.box(g, f, c)[1] > 0 for f, c in r)
    assert any(tc.unrequested(g, f, c) for f, c in r)
    for f, c in kinds["crosses_row_end"]:
        x0, y0, x1, y1 = tc.box(g, f, c)
        assert (x0, x1) == (0, g.w) and tc.unrequested(g, f, c), (f, c)
    for k in ("single", "single_interior", "row_run", "whole_rows"):
        assert not any(tc.unrequested(g, f, c) for f, c in kinds.get(k, [])), k
    for f, c in kinds["single_interior"]:
        assert tc.box(g, f, c)[:2] == tc.tile_rect(g, f)[:2] and min(tc.box(g, f, c)[:2]) >= g.tile
    # one handle sees them in an order of its own, the same in every run
    s = tc.shuffled_ranges(g, 5)
    assert sorted(s) == sorted(r) and s != r and s == tc.shuffled_ranges(g, 5)


def test_b_has_78_ranges_and_the_20_tile_grids_71():
    assert len(tc.ranges(tc.GEOS["B"])) == 78
    assert len(tc.ranges(tc.GEOS["A"])) == len(tc.ranges(tc.GEOS["F"])) == 20 + 1 + 19 + 16 + 15
    # (configuration, view, range) triples of the sweep, each through both entry points
    assert len(tc.PAIRS) == 34 and sum(len(tc.ranges(c.geo)) for c, _ in tc.PAIRS) == 2183 and len(tc.ENTRIES) == 2


@pytest.mark.parametrize("g", list(tc.GEOS.values()), ids=lambda g: g.id)
def test_partitions_cover_the_grid_for_every_world_size(g):
    n = tc.ntiles(g)
    parts = tc.partitions(g)
    assert [w for w, _ in parts] == list(range(1, n + 2))
    for w, shares in parts:
        assert all(c >= 1 for _, c in shares) and len(shares) == min(w, n)
        assert [t for f, c in shares for t in range(f, f + c)] == list(range(n))


def test_partitions_reassemble_the_oracles_file(oracle):
    for c in tc.BASE:
        cs, hdr, parts = tc.reference(oracle, c)
        for w, shares in tc.partitions(c.geo):
            assert sharding.assemble(hdr, [b"".join(parts[f:f + n]) for f, n in shares]) == cs


def test_bad_ranges_are_out_of_bounds():
    for g in tc.GEOS.values():
        n = tc.ntiles(g)
        for what in tc.BAD_RANGES:
            f, c = tc.bad_range(g, what)
            assert 0 <= f <= 0xffffffff and 0 <= c <= 0xffffffff
            assert c == 0 or f >= n or f + c > n
        f, c = tc.bad_range(g, "end_wraps_32_bits")
        assert f < n and 0 < (f + c) & 0xffffffff <= n  # what a 32-bit sum would accept


def test_launch_knob_sets_name_known_knobs():
    assert len(tc.LAUNCH_KNOBS) >= 40
    for kn in tc.LAUNCH_KNOBS:
        assert kn and set(kn) <= set(tc.dv.DEFAULTS)
    assert any(kn.get("no_fuse") for kn in tc.LAUNCH_KNOBS) and any("fused_wpb" in kn for kn in tc.LAUNCH_KNOBS)
    assert {tc.BY_NAME[n].geo.id for n in tc.LAUNCH_CONFIGS} == {"A", "F"}
