"""The styled Tier-1 path on the GPU, block by block (run with -m gpu): j2k_hip_stage_t1_styled -- the bypass instantiation
of the modeller, t1_mq_styled_kernel (a lane per block, the codeword staged in LDS and drained in 16-byte units) and
t1_rate_fixup_kernel on the device -- against the CPU oracle's styled block coder, which test_oracle_golden.py ties to
libopenjp2's files and test_t1_mq_styled_host.py to the shared recurrence.  The blocks and what they are built to hit are
t1_styled_families.py's; every parametrisation first asserts those conditions on the oracle's output, then compares
bit-planes, passes, length, bytes and -- at segment ends and the last pass -- the byte counts.  A mismatch names
(workgroup, lane, style)."""
import pytest

import t1_styled_families as fam

pytestmark = pytest.mark.gpu

J2K_HIP_ERR_PARAM = 1


@pytest.fixture(scope="module")
def enc():
    from j2k_amd import api
    e = api.Encoder(0)
    yield e
    e.close()


def _stage(enc, family, rev, style):
    plane, rects, orients, step = fam.plane(family, rev)
    return enc.stage_t1(plane.copy(), rects, orients, [step] * len(rects), rev, style=style)


@pytest.mark.parametrize("style", fam.MIXED_STYLES_REV)
def test_mixed_family_reversible(enc, oracle, style):
    rs = fam.refs(oracle, "mixed", True, style)
    fam.conditions("mixed", style, rs)
    fam.compare(_stage(enc, "mixed", True, style), rs, style)


@pytest.mark.parametrize("style", fam.MIXED_STYLES_IRR)
def test_mixed_family_irreversible(enc, oracle, style):
    rs = fam.refs(oracle, "mixed", False, style)
    fam.conditions("mixed", style, rs)
    fam.compare(_stage(enc, "mixed", False, style), rs, style)


def test_small_family_every_style(enc, oracle):
    for style in fam.SMALL_STYLES:
        rs = fam.refs(oracle, "small", True, style)
        try:
            fam.conditions("small", style, rs)
            fam.compare(_stage(enc, "small", True, style), rs, style)
        except AssertionError as e:
            raise AssertionError(f"style {style}: {e}") from e


def test_refusals_and_style_zero(enc, oracle):
    from j2k_amd import api
    plane, rects, orients, step = fam.plane("small", True)
    six = slice(0, 12, 2)  # six blocks: the steered 3 x 5 one, 32 x 32, 37 x 64, 1 x 1, 64 x 64, 64 x 13
    args = (rects[six], orients[six], [step] * 6, True)
    for style, word in ((8, "vertically causal"), (64, "unknown"), (1 | 8, "vertically causal")):
        with pytest.raises(api.J2kHipError) as ei:
            enc.stage_t1(plane.copy(), *args, style=style)
        assert ei.value.code == J2K_HIP_ERR_PARAM and word in str(ei.value)
    old = enc.stage_t1(plane.copy(), *args, want_passes=True)
    new = enc.stage_t1(plane.copy(), *args, style=0)
    assert any(o["npasses"] > 30 for o in old)
    for i, (o, n) in enumerate(zip(old, new)):
        del o["nmsedec"]
        assert n == o, i
    # and both are the oracle's
    for i, (n, (data, orient)) in enumerate(zip(new, fam.scaled_blocks(oracle, "small", True)[six])):
        r = oracle.t1_block(data, orient)
        assert (n["numbps"], n["npasses"], n["data"], n["rates"]) == (r["numbps"], r["npasses"], r["data"], r["rates"]), i
