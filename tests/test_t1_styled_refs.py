"""CPU: the references of the styled block-level tests meet the conditions they were built for (t1_styled_families.py:
block lengths per workgroup, terminations behind a drain and crowded in one chunk of decisions, raw segments of no bytes
and the MQ restarts behind them, the raw 0xFF cases, cleanup passes of nothing but segmentation symbols), for every
parametrisation that test_t1_styled_blocks.py runs on the GPU -- so that a seed or an oracle change that loses one of them
is seen without a GPU -- and the oracle's styled block coder keeps what the unstyled one returned."""
import numpy as np
import pytest

import t1_styled_families as fam


@pytest.mark.parametrize("style", fam.MIXED_STYLES_REV)
def test_mixed_family_meets_its_conditions(oracle, style):
    fam.conditions("mixed", style, fam.refs(oracle, "mixed", True, style))


@pytest.mark.parametrize("style", fam.MIXED_STYLES_IRR)
def test_mixed_family_irreversible_meets_its_conditions(oracle, style):
    fam.conditions("mixed", style, fam.refs(oracle, "mixed", False, style))


def test_small_family_meets_its_conditions(oracle):
    assert len(fam.small_blocks()) == 40 and len(fam.SMALL_STYLES) == 31
    shapes = {b.shape for b, _ in fam.small_blocks()}
    assert {(32, 32), (13, 64), (64, 37), (7, 5), (1, 1), (16, 16), (64, 64), (8, 8)} <= shapes  # (h, w)
    for style in fam.SMALL_STYLES:
        try:
            fam.conditions("small", style, fam.refs(oracle, "small", True, style))
        except AssertionError as e:
            raise AssertionError(f"style {style}: {e}") from e


def test_the_searched_block_ends_a_raw_segment_on_ff7f(oracle):
    """FF7F_SEEDS: the search itself is not repeated here (2^20 blocks); what it found is."""
    assert fam.FF7F_SEEDS[0] is None  # bypass without TERMALL: no seed below 2^20 shows it (search_ff7f(oracle, 1, 2))
    data = (fam.integers_block(fam.FF7F_SEEDS[1], 8, 8, 16) << 6).astype(np.int32)
    assert oracle.t1_block(data, 3, style=1 | 4)["events"]["raw_ff7f_dropped"] >= 1
    assert oracle.t1_block(data, 3, style=1 | 4 | 16)["events"]["raw_ff7f_kept"] >= 1
    blocks = fam.small_blocks()
    assert np.array_equal(blocks[-1][0], fam.integers_block(fam.FF7F_SEEDS[1], 8, 8, 16)) and blocks[-1][1] == 3


def test_steered_blocks_quantise_to_all_ones():
    for rev in (True, False):
        vals = fam.all_ones_values(rev)
        assert len(vals) >= 2
        for v in vals:
            m = v if rev else fam._quantised(v)
            assert m >= 0x8000 and m & 0xfff == 0xfff


def test_style_zero_is_the_unstyled_coder(oracle):
    rng = np.random.default_rng(3)
    for w, h in ((64, 64), (5, 7), (1, 1)):
        data = (rng.integers(-4000, 4000, size=(h, w)) << 6).astype(np.int32)
        a = oracle.t1_block(data, 1, want_symbols=True)
        b = oracle.t1_block(data, 1, style=0, want_symbols=True)
        assert "seg_ends" not in a and set(a) == set(b)
        for k in a:
            assert np.array_equal(a[k], b[k]), k
        # a style changes neither the passes nor the decisions outside raw passes
        c = oracle.t1_block(data, 1, style=2 | 32, want_symbols=True)
        assert c["pass_nsym"] == a["pass_nsym"] and np.array_equal(c["symbols"], a["symbols"])
        assert c["seg_ends"] == [False] * (c["npasses"] - 1) + [True] * min(c["npasses"], 1)
