"""GPU: the Tier-1 decode kernels on DAMAGED code-block bytes, block by block (run with -m gpu): the wave-per-block kernel
(t1_decode_kernel: mq_bytein behind its 256-byte lane window) and the lane-per-block kernel (t1_dec_lane.h: bytein, the
branch-free first BYTEIN of decode(), the 64-byte ring and its refill) through j2k_hip_stage_t1_decode, against the oracle's
block decoder on the same bytes.  Every comparison is word for word; words outside the rectangles must stay.

The bytes are those of tests/damaged_cases.py: single bit flips, 0xFF + a marker byte (0x90, 0xC3, 0xFF: nothing more is
consumed, the decoder's position stands still while the window or ring is asked for the same byte again), 0xFF 0x8F (the
largest byte that is still data), 0xFF 0xFF 0xFF, 0xFF and 0xFF 0x7F as the last bytes, all 0xFF, all zero, all random --
the placed ones at every position of the block's set (dword edges, the ring's 64 bytes, the window's 256, fractions of
the length, the end), the 0xFF last in one granule and the byte behind it first in the next.  Lengths, pass counts and
bit-plane counts are the clean case's.  test_t1_dec_damaged_refs.py holds what the references must meet for this to mean
anything; the same damage inside MQ-coded segments under code-block styles is the damaged-mq-* family of
t1_dec_styled_cases.py (test_t1_dec_styled_blocks.py, test_t1_lane_styled_host.py)."""
import numpy as np
import pytest

import damaged_cases as dm
import decode_stage_cases as dc

pytestmark = pytest.mark.gpu

KERNELS = ["wave", "lanes"]
TRANSFORMS = [True, False]
both = lambda f: pytest.mark.parametrize("kernel", KERNELS)(pytest.mark.parametrize("rev", TRANSFORMS, ids=["rev", "irr"])(f))


@pytest.fixture(scope="module")
def enc():
    from j2k_amd import api
    e = api.Encoder(0)
    yield e
    e.close()


def _check(enc, oracle, cases, rev, kernel):
    assert 0 < len(cases) <= 400
    got, want, rects = dc.decode_and_expect(enc, oracle, cases, rev, kernel)
    dc.assert_planes_equal(got, want, rects, cases)


@both
@pytest.mark.parametrize("mode", dm.MODES)
def test_t1_decode_damaged_bytes(enc, oracle, mode, rev, kernel):
    """Style 0: the six blocks under one mode, at every position of each block's set."""
    cases = [c for _, _, _, c in dm.mode_cases(oracle, rev, mode)]
    npos = sum(len(dm.positions(len(c["data"]))) for _, c in dm.blocks(oracle, rev))
    assert npos >= 80  # (three bytes do not fit at the set's last position, length - 2: one ff_run less per block)
    assert len(cases) == {"marker": 3 * npos, "flip": npos, "ff8f": npos, "ff_run": npos - 6}.get(mode, 6)
    _check(enc, oracle, cases, rev, kernel)


@both
def test_t1_decode_markers_across_every_window_edge(enc, oracle, rev, kernel):
    """The 9 KB stream with 0xFF as the last byte of each 256-byte window up to 4096 and the marker first in the next."""
    cases = dm.window_edge_cases(oracle)
    assert len(cases) == 16
    _check(enc, oracle, cases, rev, kernel)


@both
def test_t1_decode_damaged_and_cut(enc, oracle, rev, kernel):
    """A marker among the kept bytes with 1, 4 and npasses - 1 passes kept (bytes cut at the pass's rate, and all there); and
    a marker behind the bytes of the kept passes, which must decode like the clean bytes."""
    cut = [bad for _, bad in dm.cut_cases(oracle, rev)]
    _check(enc, oracle, cut, rev, kernel)
    behind = dm.behind_cases(oracle, rev)
    got, want, rects = dc.decode_and_expect(enc, oracle, [bad for _, bad in behind], rev, kernel)
    dc.assert_planes_equal(got, want, rects, [bad for _, bad in behind])
    clean, want_clean, _ = dc.decode_and_expect(enc, oracle, [c for c, _ in behind], rev, kernel)
    assert np.array_equal(want, want_clean) and np.array_equal(got, clean)


@pytest.mark.parametrize("rev", TRANSFORMS, ids=["rev", "irr"])
def test_t1_decode_lanes_stuck_and_advancing_in_one_wave(enc, oracle, rev):
    """One wave of the lane kernel: the long stream in lane 0, clean and damaged copies in turn with markers at different
    depths, a 1 x 1 block in the last lane; then the same blocks with clean and damaged ones swapped round in the wave."""
    cases = dm.unlike_wave(oracle, rev)
    assert len(cases) == 64
    _check(enc, oracle, cases, rev, "lanes")
    _check(enc, oracle, cases[:1] + cases[1:63][::-1] + cases[63:], rev, "lanes")
    _check(enc, oracle, cases, rev, "wave")
