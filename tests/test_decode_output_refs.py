"""CPU: the reference of test_decode_output.py on that file's own inputs.

Oracle.decode_output is the tail of the oracle's tile decode, so test_decode_oracle.py and test_oracle_golden.py pin it to
libopenjp2 -- on what files hold: in-range samples of 8 bits and more.  The GPU stage tests feed it what no file here holds
(samples far outside the range, every class of float, precisions down to 1 bit).  These tests anchor it there against an
independent numpy restatement (decode_output_cases.numpy_decode_output), bound the float32 inverse ICT against float64, and
check that the case generators produce what they claim.  No case is left out of any comparison.
"""
import numpy as np
import pytest

import decode_output_cases as oc

GROUPS = {"depth": oc.depth_cases, "clamp": oc.clamp_rev_cases, "float": oc.float_cases, "shape": oc.shape_cases,
          "subsampling": oc.subsampling_cases, "geometry": oc.geometry_cases}


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_oracle_decode_output_matches_the_numpy_restatement(oracle, group):
    cases = GROUPS[group]()
    assert cases
    for case in cases:
        got = oracle.decode_output(case["comps"], case["precs"], case["rev"], case["mct"])
        want = oc.numpy_decode_output(case["comps"], case["precs"], case["rev"], case["mct"])
        assert len(got) == len(want) == len(case["comps"])
        for c, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape == case["comps"][c].shape
            assert np.array_equal(g, w), (case["name"], c, np.flatnonzero(g.ravel() != w.ravel())[:5])


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_expected_buffer_holds_the_restated_samples_and_the_fill(oracle, group):
    """expected() from the oracle's samples equals expected() from the restatement's, and it writes the channels' samples
    only: every byte outside them holds the fill pattern, every channel sample read back through the channel's strides is the
    depth-converted value."""
    for case in GROUPS[group]():
        want = oc.expected(oracle, case)
        planes = oc.numpy_decode_output(case["comps"], case["precs"], case["rev"], case["mct"])
        assert np.array_equal(want, oc.expected(oracle, case, planes)), case["name"]
        touched = np.zeros(case["nbytes"], dtype=bool)
        for c in range(min(len(case["chans"]), len(planes))):
            ch = case["chans"][c]
            cw, chh = min(ch["width"], case["w"]), min(ch["height"], case["h"])
            sb = ch["sample_bits"] // 8
            idx = ch["base"] + np.arange(chh)[:, None] * ch["rowbytes"] + np.arange(cw)[None, :] * ch["colbytes"]
            for k in range(sb):
                assert not touched[idx + k].any(), (case["name"], "channels overlap")
                touched[idx + k] = True
            sx, sy = case["subs"][c]
            full = np.repeat(np.repeat(planes[c], sy, axis=0), sx, axis=1)[:case["h"], :case["w"]][:chh, :cw]
            back = want[idx].astype(np.int64) + (want[idx + 1].astype(np.int64) << 8 if sb == 2 else 0)
            shift = ch["depth"] - case["precs"][c]
            if shift <= 0:  # (the widening branches are test_decode_oracle.py's, against the reference's CopyChannel)
                assert np.array_equal(back, full.astype(np.int64) >> -shift), (case["name"], c)
            else:  # widening replicates the sample's top bits below it: the top `precision` bits are the sample
                assert np.array_equal(back >> shift, full), (case["name"], c)
        assert np.array_equal(want[~touched], oc.fill_pattern(case["nbytes"])[~touched]), case["name"]
        assert touched.any() and not touched.all(), case["name"]


def test_float32_inverse_ict_is_within_one_of_float64(oracle):
    """Where the float64 inverse ICT stays inside the nominal range, the float32 one (the oracle's, the kernel's, libopenjp2's)
    gives the same sample or a neighbour.  The bound is derived, not measured: a component takes at most four rounded float32
    operations and two rounded constants, each off by at most 2^-24 of a magnitude below 2^18, i.e. by at most 2^-6: under
    0.1 in all, so the float32 and float64 values lie less than 0.5 apart and round to the same or to adjacent integers.
    The share of samples that differ is printed, not bounded.  Measured on the planes below (standard_normal x 2^(p-1) x
    0.5 for Y, x 0.25 for U and V; 3 x 2^18 samples per precision): 8 bits 1 of 707440 in-range samples (0.0001%), 10 bits
    10 of 707912 (0.0014%), 12 bits 36 of 707915 (0.0051%), 16 bits 488 of 708478 (0.0689%)."""
    rng = np.random.default_rng(6400)
    for p in (8, 10, 12, 16):
        n = 1 << 18
        y = (rng.standard_normal(n) * (1 << (p - 1)) * 0.5).astype(np.float32)
        u, v = ((rng.standard_normal(n) * (1 << (p - 1)) * 0.25).astype(np.float32) for _ in range(2))
        got = oracle.decode_output([a.reshape(512, 512) for a in (y, u, v)], [p] * 3, False, True)
        y64, u64, v64 = (a.astype(np.float64) for a in (y, u, v))
        rgb = [y64 + 1.402 * v64, y64 - 0.34413 * u64 - 0.71414 * v64, y64 + 1.772 * u64]
        lo, hi = -(1 << (p - 1)), (1 << (p - 1)) - 1
        differ = total = 0
        for g, r in zip(got, rgb):
            inside = (r >= lo) & (r <= hi)
            want = np.rint(r).astype(np.int64) - lo
            d = np.abs(g.ravel().astype(np.int64) - want)[inside]
            assert inside.sum() > n // 2
            assert d.max() <= 1, (p, d.max())
            differ += int((d != 0).sum())
            total += int(inside.sum())
        print(f"precision {p}: {differ} of {total} in-range samples ({100.0 * differ / total:.4f}%) differ by one from the float64 inverse ICT")


# ------------------------------------------------------------------------------------------------ the generators
def test_depth_cases_hold_every_value_of_every_triple():
    seen = set()
    samples = 0
    for case in oc.depth_cases():
        assert case["rev"] and not case["mct"] and len(case["chans"]) == 4
        p = case["precs"][0]
        assert case["precs"] == [p] * 4
        for c, ch in enumerate(case["chans"]):
            values = case["comps"][c].ravel().astype(np.int64) + (1 << (p - 1))
            assert np.array_equal(np.sort(values), np.arange(1 << p)), (p, c)
            assert (ch["width"], ch["height"]) == (case["w"], case["h"])
            triple = (p, ch["sample_bits"], ch["depth"])
            assert triple not in seen
            seen.add(triple)
            samples += values.size
        assert len({ch["sample_bits"] for ch in case["chans"]}) == 2, "8- and 16-bit channels in every call"
    assert seen == set(oc.depth_triples()) and len(seen) == 384
    assert samples == 24 * (2 ** 17 - 2)  # about 3 M


def test_clamp_cases_reach_beyond_both_ends():
    cases = oc.clamp_rev_cases()
    plain = [c for c in cases if not c["mct"]]
    assert sorted(c["precs"][0] for c in plain) == sorted(oc.CLAMP_PRECS)
    for case in plain:
        p = case["precs"][0]
        lo, hi = -(1 << (p - 1)), (1 << (p - 1)) - 1
        for comp in case["comps"]:
            assert {lo - 1, lo, hi, hi + 1, -(1 << 30), 1 << 30} <= set(comp.ravel().tolist()), p
    rct = [c for c in cases if c["mct"]]
    assert rct
    for case in rct:
        p = case["precs"][0]
        lo, hi = -(1 << (p - 1)), (1 << (p - 1)) - 1
        y, u, v = (c.astype(np.int64) for c in case["comps"][:3])
        assert max(np.abs(a).max() for a in (y, u, v)) < 1 << 28  # (no int32 sum of the transform wraps)
        g = y - ((u + v) >> 2)
        rgb = np.stack([v + g, g, u + g])
        below, above = rgb < lo, rgb > hi
        for c in range(3):
            assert below[c].any() and above[c].any(), (p, c)  # beyond each end in each channel
            alone_below = below[c] & ~(below | above)[[i for i in range(3) if i != c]].any(axis=0)
            alone_above = above[c] & ~(below | above)[[i for i in range(3) if i != c]].any(axis=0)
            assert alone_below.any() and alone_above.any(), (p, c)  # ... while the other two stay inside: they clamp independently
        outside = (below | above).sum(axis=0)
        assert {0, 1, 2, 3} <= set(outside.ravel().tolist())
        assert (below.all(axis=0)).any() and (above.all(axis=0)).any() and (below.any(axis=0) & above.any(axis=0)).any()
        s = u + v
        assert ((s < 0) & (s % 4 != 0)).any(), "floor and truncation of (u + w) / 4 differ here"
        assert (((s >> 2) != np.trunc(s / 4.0).astype(np.int64))).any()
        fourth = case["comps"][3].astype(np.int64)
        p4 = case["precs"][3]
        assert p4 != p and (fourth < -(1 << (p4 - 1))).any() and (fourth > (1 << (p4 - 1)) - 1).any()


def test_float_cases_hold_every_listed_class():
    cases = oc.float_cases()
    assert sorted({c["precs"][0] for c in cases}) == sorted(oc.FLOAT_PRECS)
    for case in cases:
        assert not case["rev"]
        p = case["precs"][0]
        if not case["mct"]:
            everything = np.concatenate([c.ravel() for c in case["comps"]])
            missing = [k for k, v in {**oc.float_classes(everything), **oc.clamp_edge_classes(everything, p)}.items() if not v]
            assert not missing, (case["name"], missing)
            # an ordinary plane: standard_normal x 2^(p-1), most of it inside the range, some beyond either end
            normal = case["comps"][1]
            assert 0.5 < (np.abs(normal) < (1 << (p - 1))).mean() < 0.9
        elif "planes" in case["name"]:  # ordinary planes alone: finite, mostly inside the range after the transform
            assert all(np.isfinite(c).all() for c in case["comps"]) and case["comps"][0].size >= 1 << 17
            out = oc.numpy_decode_output(case["comps"], case["precs"], False, True)
            assert all(0.5 < ((o > 0) & (o < (1 << p) - 1)).mean() < 0.999 for o in out)
        else:
            for c in range(3):  # each of Y, U, V holds every class in turn, beside two finite ordinary values
                comp = case["comps"][c].ravel()
                missing = [k for k, v in {**oc.float_classes(comp), **oc.clamp_edge_classes(comp, p)}.items() if not v]
                assert not missing, (case["name"], c, missing)
                k = 3 * oc.float_specials(p).size
                others = [case["comps"][i].ravel()[:k][c::3] for i in range(3) if i != c]
                assert all(np.isfinite(o).all() and (np.abs(o) < 1 << (p + 2)).all() for o in others)
            # the transform's outputs go beyond both ends and to NaN (inf - inf) in every one of R, G, B
            with np.errstate(all="ignore"):
                y, u, v = (c.ravel() for c in case["comps"][:3])
                rgb = [y + v * np.float32(1.402), (y - u * np.float32(0.34413)) - v * np.float32(0.71414), y + u * np.float32(1.772)]
            for r in rgb:
                assert np.isnan(r).any() and (r > 2.0 ** 31).any() and (r < -2.0 ** 31).any()
                assert ((r > (1 << (p - 1))) & (r < 2.0 ** 20)).any() and ((r < -(1 << (p - 1)) - 1) & (r > -2.0 ** 20)).any()
    # random 32-bit patterns: every exponent occurs
    pats = oc.float_cases()[0]["comps"][2].ravel().view(np.uint32)
    assert len(set(((pats >> 23) & 0xff).tolist())) == 256


def test_shape_cases_are_the_listed_ones():
    cases = oc.shape_cases()
    for rev in (True, False):
        mine = [c for c in cases if c["rev"] == rev]
        assert {(c["w"], c["h"]) for c in mine if c["stride"] is None} == {(1, 3), (255, 3), (256, 3), (257, 3), (513, 3), (1000, 3), (3, 70000)}
        assert [(c["w"], c["stride"]) for c in mine if c["stride"] is not None] == [(300, 320)]
        tall = [c for c in mine if c["h"] == 70000][0]
        rows = tall["comps"][0]
        assert not np.array_equal(rows[:70000 - 65535], rows[65535:])  # the rows of the second step are not those of the first
    for case in cases:
        p = case["precs"][0]
        for comp in case["comps"]:
            if comp.size > 100:
                assert (comp < -(1 << (p - 1))).any() and (comp > (1 << (p - 1))).any()


def test_subsampling_cases_are_the_listed_ones():
    cases = oc.subsampling_cases()
    factors = set()
    once = False
    for case in cases:
        w, h = case["w"], case["h"]
        for (sx, sy) in case["subs"]:
            assert 1 <= sx <= 4 and 1 <= sy <= 4
            factors.add(("x", sx))
            factors.add(("y", sy))
            once = once or (sx > 1 and w % sx == 1 and w > sx) or (sy > 1 and h % sy == 1 and h > sy)
    assert factors == {(a, f) for a in "xy" for f in (1, 2, 3, 4)} and once
    general = [c for c in cases if len(c["subs"]) == 4 and not c["mct"]]
    assert general and all(len(set(c["subs"])) == 4 and len(set(c["precs"])) == 4 for c in general)
    assert any(c["w"] % sx or c["h"] % sy for c in general for (sx, sy) in c["subs"])
    for subs in ([(1, 1), (2, 2), (2, 2)], [(1, 1), (2, 1), (2, 1)]):
        for p in (8, 10):
            for rev in (True, False):
                assert any(c["subs"] == subs and c["precs"] == [p] * 3 and c["rev"] == rev for c in cases), (subs, p, rev)


def test_geometry_cases_are_the_listed_ones():
    cases = oc.geometry_cases()
    for rev in (True, False):
        mine = [c for c in cases if c["rev"] == rev]
        w, h = mine[0]["w"], mine[0]["h"]
        ae = [c for c in mine if c["chans"][0]["colbytes"] in (4, 8) and len({ch["colbytes"] for ch in c["chans"]}) == 1 and c["chans"][0]["colbytes"] > c["chans"][0]["sample_bits"] // 8]
        assert {(c["chans"][0]["sample_bits"], len(c["chans"])) for c in ae} >= {(8, 3), (8, 4), (16, 3), (16, 4)}
        assert all(c["chans"][0]["rowbytes"] > w * c["chans"][0]["colbytes"] for c in ae)  # row padding
        assert any(all(ch["rowbytes"] < 0 for ch in c["chans"]) for c in mine)
        assert any(all(ch["colbytes"] == 3 for ch in c["chans"]) for c in mine)
        assert any(len(c["chans"]) < len(c["comps"]) for c in mine) and any(len(c["chans"]) > len(c["comps"]) for c in mine)
        assert any(len({(ch["width"], ch["height"]) for ch in c["chans"]}) > 2 and all(ch["width"] <= w and ch["height"] <= h for ch in c["chans"]) for c in mine)
        assert any(all(ch["width"] > w or ch["height"] > h for ch in c["chans"]) for c in mine)
        assert any({ch["sample_bits"] for ch in c["chans"]} == {8, 16} for c in mine)
        assert any(c["mct"] for c in mine) and any(not c["mct"] for c in mine)
