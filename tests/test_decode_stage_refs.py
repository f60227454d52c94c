"""CPU: the oracle's stage-level decode references on the inputs of test_decode_stages.py.

The oracle's inverse DWT and block decoder are pinned to libopenjp2 through whole files only; the GPU stage tests feed
them synthetic inputs no file holds (lines of 1 .. 13 samples at either parity, sparse and truncated blocks).  These
tests anchor the references there, without a GPU: exact inversion of the oracle's own forward stages where that is a
property (5/3, lossless Tier-1), and a float64 restatement of T.800 F.3 for the 9/7 synthesis.
"""
import numpy as np
import pytest

import decode_stage_cases as dc
from t1_families import emission_families, sparse_families


@pytest.mark.parametrize("levels", dc.SWEEP_LEVELS)
def test_idwt53_inverts_dwt53_over_the_sweep(oracle, levels):
    rng = np.random.default_rng(530 + levels)
    for (w, h, x0, y0) in dc.sweep_shapes():
        a = dc.idwt_input(rng, (h, w), True)
        back = oracle.idwt53(oracle.dwt53(a, levels, x0, y0), levels, x0, y0)
        assert np.array_equal(back, a), (w, h, x0, y0, levels)


@pytest.mark.parametrize("family", ["emission", "sparse"])
def test_block_decoder_inverts_block_coder(oracle, family):
    """Reversible blocks of both families, all passes: the decoder's value (one fractional bit, the middle of the
    interval) halved toward zero is the coefficient."""
    rng = np.random.default_rng(97 if family == "emission" else 98)
    for blk, orient in (emission_families(rng) if family == "emission" else sparse_families(rng)):
        c = dc.code_block(oracle, blk, orient, True)
        e = dc.expected_words(oracle, c, True)
        if e is None:
            assert not blk.any(), (blk.shape, orient)
            continue
        assert np.array_equal(e, blk), (blk.shape, orient)


def test_idwt97_matches_float64_restatement(oracle):
    """oracle.idwt97 against the float64 restatement of T.800 F.3 (decode_stage_cases.idwt97_float64) over the sweep,
    standard_normal x 3000 inputs.  Lines of one sample are left as they are by libopenjp2 (no gain applied); the
    restatement does the same, so n == 1 lines are not checked -- the only exclusion.

    The error is measured against the float64 result, in units of 2^-24 of the plane's largest magnitude (of the float64
    result).  Measured over the 5400 cases of the sweep: worst 19.23 units (w = 31, h = 12, origin (1, 0), 5 levels).
    Bound: four times that, 76.92 units; the margin covers other seeds."""
    bound = 4 * 19.23
    worst, at = 0.0, None
    rng = np.random.default_rng(9797)
    for levels in dc.SWEEP_LEVELS:
        for (w, h, x0, y0) in dc.sweep_shapes():
            a = dc.idwt_input(rng, (h, w), False)
            ref = dc.idwt97_float64(a, levels, x0, y0)
            got = oracle.idwt97(a, levels, x0, y0).astype(np.float64)
            err = np.abs(got - ref).max() / np.abs(ref).max() * 2.0 ** 24
            if err > worst:
                worst, at = err, (w, h, x0, y0, levels)
    print(f"idwt97 against float64: worst error {worst:.2f} x 2^-24 of the plane's largest magnitude at {at}")
    assert worst <= bound, (worst, at)


def test_long_stream_and_top_plane_blocks_are_what_they_claim(oracle):
    """The two special blocks of the GPU tests are as described there, and the oracle decodes them back."""
    rng = np.random.default_rng(4242)
    c = dc.code_scaled(oracle, dc.long_stream_block(rng), 0)
    assert c["numbps"] == 16 and c["npasses"] == 46 and len(c["data"]) > 8192
    b = dc.top_planes_block(rng)
    c = dc.code_scaled(oracle, b, 3)
    assert c["numbps"] == 25 and c["npasses"] == 73
    v = oracle.t1_decode_block(c["data"], c["w"], c["h"], 3, 25, 73)
    # 6 fractional bits in, 1 out: the decoded value is the input cut to bit 5 with the half-interval bit below it
    m = np.abs(b.astype(np.int64)) >> 6
    assert np.array_equal(np.abs(v.astype(np.int64)) >> 1, m)
    assert np.array_equal(np.sign(v)[m > 0], np.sign(b)[m > 0])
