"""GPU: the lane-per-block Tier-1 decode kernel under code-block styles, block by block, through
j2k_hip_stage_t1_decode_styled.  Every group of t1_dec_styled_cases.py: both families of t1_styled_families.py under their
styles, every last pass, codewords and segment tables cut short, damaged raw and MQ-coded segments, every block of the styled files of
libopenjp2 under the file's own style, many bit-planes with and without a region-of-interest shift, orders and group
sizes.  Expected words are the oracle's styled block decoder's on the same bytes and the same segment table, laid into a
plane whose other words must stay as they were.  Bit-exact.  test_t1_lane_styled_host.py runs the same cases through the
kernel's own source on the host; test_t1_dec_styled_refs.py holds the conditions."""
import numpy as np
import pytest

import decode_stage_cases as dsc
import t1_dec_styled_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from j2k_amd import api
    return api


@pytest.fixture(scope="module")
def enc(api):
    e = api.Encoder(0)
    yield e
    e.close()


@pytest.mark.parametrize("name", tc.GROUP_NAMES)
def test_styled_lane_decode_equals_the_styled_oracle(enc, oracle, name):
    batches = tc.group(oracle, name)
    assert batches
    for rev, style, cases in batches:
        got, want, rects = tc.decode_and_expect(enc, oracle, cases, rev, style)
        dsc.assert_planes_equal(got, want, rects, cases)


def test_style_zero_is_the_unstyled_hook(enc, oracle):
    rng = np.random.default_rng(3)
    cases = [dsc.code_block(oracle, blk, o, True) for _, blk, o in dsc.subset_blocks(rng)]
    cases = [dict(c, segs=[]) for c in cases]
    got, want, rects = tc.decode_and_expect(enc, oracle, cases, True, 0)
    dsc.assert_planes_equal(got, want, rects, cases)
    plain, want0, _ = dsc.decode_and_expect(enc, oracle, cases, True, "lanes")
    assert np.array_equal(plain, got) and np.array_equal(want0, want)


def test_refusals(api, enc, oracle):
    rev, style, cases = tc.group(oracle, "small-5")[0]
    cases = cases[:4]
    shape, rects = dsc.lay_out(cases)
    blocks = [dict(c, rect=r) for c, r in zip(cases, rects)]
    plane = dsc.fill_pattern(shape)
    enc.stage_t1_decode_styled(plane, blocks, True, 5)  # (as it should be: accepted)
    total = sum(len(b["segs"]) for b in blocks)
    pairs = [s for b in blocks for s in b["segs"]]
    first = np.cumsum([0] + [len(b["segs"]) for b in blocks[:-1]]).tolist()
    count = [len(b["segs"]) for b in blocks]

    def refused(style_, table=None, blks=blocks):
        with pytest.raises(api.J2kHipError) as ei:
            enc.stage_t1_decode_styled(plane, blks, True, style_, raw_table=table)
        assert ei.value.code == 1  # J2K_HIP_ERR_PARAM

    refused(64)                                                         # style bits above 63
    refused(5 | 128)
    refused(5, (first[:-1] + [total - 1], count, pairs, total))         # a segment range that runs out of the table
    refused(5, (first[:-1] + [total + 1], count, pairs, total))
    refused(2, (first, count, pairs, total))                            # segments under a style without bypass and termall
    refused(0, (first, count, pairs, total))
    refused(5, (first, count, [(1 << 24, 1)] + pairs[1:], total))       # a segment of 2^24 bytes
    refused(5, (first, count, [(pairs[0][0], 256)] + pairs[1:], total)) # a segment of 256 passes
    refused(5, (first, [0] + count[1:], pairs, total))                  # passes, but no segment
    # what a file cut short leaves is accepted: fewer segments than the passes need, lengths summing past cw_len
    enc.stage_t1_decode_styled(plane, blocks, True, 5, raw_table=(first, [1] + count[1:], pairs, total))
    enc.stage_t1_decode_styled(plane, blocks, True, 5, raw_table=(first, count, [(pairs[0][0] + 100000, pairs[0][1])] + pairs[1:], total))
