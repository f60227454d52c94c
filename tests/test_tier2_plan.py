"""GPU: host Tier-2's real piece layouts through the gather kernel (gather.hip via j2k_hip_stage_gather).  Four of the plans of
tests/test_tier2_plan_refs.py -- untiled with one layer (the blocks go by cblk_dst, blocks of no bytes among them), seven
layers (body pieces at any offset of their block, at any destination alignment; plan_codestream lists no body piece of zero
bytes, so none reaches the kernel on this path: zero lengths are gather_cases.py's), termall, and the tile of 4096 blocks --
are laid out by the kernel from the plan's header pieces and block / body pieces, with the random block bytes as the source; the result must be what api.assemble laid
out on the host (which the CPU tier holds to the oracle's reader), and the bytes around it untouched.

The hook checks every piece against its source and the destination before it launches."""
import numpy as np
import pytest

import tier2_cases as tc

pytestmark = pytest.mark.gpu

MARGIN = 64


@pytest.fixture(scope="module")
def api():
    from j2k_amd import api
    return api


@pytest.fixture(scope="module")
def enc(api):
    e = api.Encoder(0)
    yield e
    e.close()


@pytest.mark.parametrize("name", tc.GATHER_CASES)
def test_gather_lays_out_the_plan(api, enc, name):
    case = tc.case_named(name)
    t = tc.synth_table(api, case)
    with_alloc = case["layers"] > 1
    plan = tc.plan_table(api, t["params"], case["style"], case["layers"], t["numbps"], t["pieces"], with_alloc=with_alloc)
    want = np.frombuffer(api.assemble(plan, t["data"]), np.uint8)
    # the blocks' bytes as a codeword arena has them: every block at a 4-byte aligned offset, other bytes between them
    starts, at = [], 0
    for d in t["data"]:
        starts.append(at)
        at += (len(d) + 3) & ~3
    src = np.full(at + 4, 0xEE, np.uint8)
    for s, d in zip(starts, t["data"]):
        src[s:s + len(d)] = np.frombuffer(d, np.uint8)
    headers = [(int(d) + MARGIN, int(s), int(ln)) for d, s, ln in zip(*plan["headers"])]
    blocks, segments = [], []
    if with_alloc:
        segments = [(int(d) + MARGIN, starts[int(c)] + int(o), int(ln)) for d, c, o, ln in zip(*plan["bodies"])]
        assert any(s[1] & 3 for s in segments) and any(s[0] & 3 for s in segments)
    else:
        blocks = [(int(d) + MARGIN, starts[i], len(t["data"][i])) for i, d in enumerate(plan["cblk_dst"])]
        assert any(b[2] == 0 for b in blocks)
    dst = np.full(plan["total_len"] + 2 * MARGIN, 0xA5, np.uint8)
    got = enc.stage_gather(src, dst, blocks=blocks, headers=headers, segments=segments, blob=plan["blob"])
    assert np.array_equal(got[MARGIN:-MARGIN], want)
    assert np.all(got[:MARGIN] == 0xA5) and np.all(got[-MARGIN:] == 0xA5)
