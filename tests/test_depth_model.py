"""The model of the sample-depth tests against the oracle's C text, on any machine: depth_cases.convert (the numpy
CopyChannel every expectation of test_depth_matrix.py is built from) equals Oracle.copy_channel on every (sample type,
channel depth, file depth) of depth_cases.PAIRS over every legal stored value, no result leaves 0 .. 2^prec - 1, and the
grid points of a float channel quantise back to themselves.  This pins the reference before a device is involved."""
import numpy as np
import pytest

import depth_cases as dc
import dwt_variant_cases as dvc
import float_model as fm


def test_the_tables_hold_every_pair():
    assert len(dc.PAIRS) == 128 + 256 == len(set(dc.PAIRS)) and len(dc.FLOAT_PAIRS) == 256 == len(set(dc.FLOAT_PAIRS))
    assert all(1 <= d <= sb and 1 <= p <= 16 for sb, d, p in dc.PAIRS)
    for prec in dc.PRECS:
        assert len(dc.pairs_of(prec)) == 24
    for sb, groups in dc.GROUPS.items():
        assert sorted(d for g in groups for d in g) == list(dc.depths(sb))


@pytest.mark.parametrize("sample_bits", [8, 16])
def test_ramp_holds_every_legal_stored_value_and_nothing_else(sample_bits):
    rows, cols = dc.shape(sample_bits)
    assert rows * cols == (1 << sample_bits) * (32 if sample_bits == 8 else 1) and rows >= 16
    for d in dc.depths(sample_bits):
        r = dc.ramp(sample_bits, d)
        assert r.shape == (rows, cols) and r.min() == 0 and r.max() == (1 << d) - 1
        assert np.array_equal(np.bincount(r.reshape(-1)), np.full(1 << d, r.size >> d))
        ch = dc.channels(sample_bits, [d] * 4)
        assert ch.shape == (4, rows + 1, cols) and ch.max() == (1 << d) - 1 and ch.min() == 0
        for c in range(4):
            assert np.array_equal(np.roll(ch[c, :rows].reshape(-1), -dc.ROT[c]), r.reshape(-1))
            assert not any(np.array_equal(ch[c], ch[k]) for k in range(c))  # (at d = 1 it is the last row that tells them apart)
        corners = {tuple(int(v) for v in ch[:3, rows, x]) for x in range(cols)}
        assert corners == {(a, b, c) for a in (0, (1 << d) - 1) for b in (0, (1 << d) - 1) for c in (0, (1 << d) - 1)}


@pytest.mark.parametrize("sample_bits", [8, 16])
def test_frames_reach_fast_and_edge_strips(sample_bits):
    """The launch model of dwt.hip (dwt_variant_cases, held to the kernel by test_dwt_variant_refs.py) on the frames of
    test_depth_matrix.py::test_fused_level_1: fuse_frontend takes them (interleaved, 3 or 4 channels of one depth, one DWT
    level), and of their three strips the second is a FAST one (vector loads, paired stores), the others edge strips -- with
    one wave per workgroup and with four.  The model takes the container's bits for the sample depth; neither the fused / unfused
    decision nor a strip's FAST / edge decision depends on a depth."""
    rows, cols = dc.shape(sample_bits)
    for rev, nc in ((True, 3), (False, 4)):
        case = dvc.ae_case(cols, rows + 1, nc, rev, True, sample_bits, sample_bits, False, 0, 1, 0)
        for kn in ({}, dict(fused_wpb=1), dict(fused_wpb=4), dict(fused_generic=1)):
            assert dvc.is_fused(case, kn)
            m = dvc.fused_launch(case, kn)
            assert m["strips"] == [[False, True, False]] and m["fast"] and m["edge"], (sample_bits, nc, kn, m["strips"])
    # (what the first layout of these tests had: 256 columns, where no strip is FAST)
    assert not dvc.fused_launch(dvc.ae_case(256, 257, 3, True, True, 16, 16, False, 0, 1, 0), {})["fast"]


@pytest.mark.parametrize("prec", dc.PRECS)
def test_convert_equals_the_oracles_copy_channel(oracle, prec):
    for sb, d in dc.pairs_of(prec):
        r = dc.ramp(sb, d)
        src = np.ascontiguousarray(r.astype(dc.dtype_of(sb)))
        rows, cols = r.shape
        want = oracle.copy_channel(src.reshape(-1).view(np.uint8), 0, cols, rows, sb // 8, cols * sb // 8, sb // 8, d, prec)
        got = dc.convert(r, d, prec)
        assert np.array_equal(got, want), (sb, d, prec)
        assert got.min() >= 0 and got.max() <= (1 << prec) - 1, (sb, d, prec)
        # the ends of the range stay the ends, and the conversion never reorders two values
        assert got.reshape(-1)[0] == 0 and (prec < d or got.max() == (1 << prec) - 1)
        line = dc.convert(np.arange(1 << d), d, prec)
        assert np.all(np.diff(line) >= 0), (sb, d, prec)


def test_promoted_samples_stay_in_range():
    v = dc.promote(np.arange(65536))
    assert v.min() == 0 and v.max() == 65535
    for prec in dc.PRECS:
        got = dc.convert(v, 16, prec)
        assert got.min() >= 0 and got.max() <= (1 << prec) - 1


def test_float_grid_points_quantise_back_to_themselves():
    for d in range(1, 17):
        x = dc.float_ramp(d)
        assert x.dtype == np.float32 and x.size == 1 << d
        assert np.array_equal(fm.quantise(x, d).reshape(-1), np.arange(1 << d)), d
    v = np.arange(65536)
    assert np.array_equal(fm.quantise(dc.float_ramp(16, True), 16, True).reshape(-1), fm.promote16(fm.demote16(v)))


def test_planes_reach_both_ends_at_every_depth():
    from j2k_amd import synth
    for prec in dc.PRECS:
        pl = dc.planes(70, 45, 4, prec, 11)
        assert pl.shape == (4, 45, 70) and pl.dtype == np.int32
        for c in range(4):
            assert pl[c].min() == 0 and pl[c].max() == (1 << prec) - 1, prec
        if prec >= 8:  # synth.planes' numbers but for the two planted ends
            assert np.count_nonzero(pl != synth.planes(70, 45, 4, prec, 11)) <= 8
