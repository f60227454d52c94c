"""GPU: rate_curve_kernel alone (rate.hip; j2k_hip_encode_sequence_budget_device) through j2k_hip_stage_rate_curve, which
launches it as the budget search does, against tests/budget_model.py (rate_model.makelayer_plain and rate_model.header_bits on
the grid).  Everything compared is an integer: exact equality throughout.  The inputs are the families of rate_cases.py read as
frames: 1 x 1 block; 21 x 3 (a frame boundary inside a wave); 32 x 2; 13 x 5; 85 x 3; 64 x 4 (boundaries on workgroup edges);
257 x 1; 200 x 5; 125 x 8.

  * candidates: K = 1, 2, 16, 63 and 64, steps of 1, 16 and 256, a base of J2K_HIP_SLOPE_ALL, an interior one and one whose
    tail clamps at J2K_HIP_SLOPE_K_MAX;
  * caps: none; one frame capped inside the candidate range; every frame capped at or above the last candidate, so that all
    columns are equal; the weights wrap per frame (nweights = blocks per frame);
  * what the launch must leave alone: the spare entries behind the sums keep their fill, and the pass tables come back as
    sent, the rows beyond npasses filled with 0xA5 here;
  * the answers are not trivial (on the model alone): for the large families some candidate leaves blocks short of their passes,
    some candidate leaves a block empty, and two adjacent candidates differ in their sums;
  * refusals, after which the handle stages a case correctly.
"""
import numpy as np
import pytest

import budget_model as bm
import rate_cases as rc
import rate_model as rm

FILL64 = 0xA5A5A5A5A5A5A5A5
FILL32 = 0xA5A5A5A5

# family -> the frame counts it is read as
SPLITS = {"mono_1": (1,), "mono_63_one_comp": (3,), "mono_64_comp3": (2,), "real53_65": (5,), "spoiled_65": (5,), "mono_255": (3,),
          "mono_256": (4,), "real97_257": (1,), "big_257": (1,), "mono_1000": (5, 8)}
assert sorted(SPLITS) == sorted(rc.CALL_NAMES)

# (K, step, base): every K, every step, the three kinds of base; the tails of the last three clamp at K_MAX
COMBOS = [(1, 1, bm.ALL), (2, 16, 320), (16, 1, 320), (63, 16, -160), (64, 256, bm.ALL), (64, 1, 2000), (16, 256, bm.ALL), (2, 256, 1900),
          (64, 16, 320), (1, 16, bm.K_MAX), (63, 1, bm.ALL)]
FEW = [(2, 16, 320), (16, 256, bm.ALL), (64, 16, 320), (63, 1, 300), (1, 1, bm.ALL)]  # of the 1000-block family


@pytest.fixture(scope="module")
def api():
    from j2k_amd import api
    return api


@pytest.fixture(scope="module")
def enc(api):
    e = api.Encoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def all_calls(oracle):
    return rc.calls(oracle)


_curves = {}


def curve_of(call):
    if call["name"] not in _curves:
        _curves[call["name"]] = bm.Curve(rc.tables(call))
    return _curves[call["name"]]


def filled(call):
    rate, dist = call["pass_rate"].copy(), call["pass_dist"].copy()
    for b, k in enumerate(call["npasses"]):
        rate[b, int(k):] = FILL32
        dist[b, int(k):] = FILL32 - (1 << 32)
    return rate, dist


def stage(enc, call, nframes, cap, base, step, K, weight=None):
    rate, dist = filled(call)
    out = enc.stage_rate_curve(call["weight"] if weight is None else weight, call["numbps"], call["npasses"], rate, dist, nframes, cap, base, step, K)
    assert out["spare"].size == 64 and (out["spare"] == FILL64).all(), call["name"]
    assert np.array_equal(out["rate_back"], rate) and np.array_equal(out["dist_back"], dist), call["name"]
    return out["sums"]


def cap_variants(nframes, base, step, K):
    cand = bm.candidates(base, step, K)
    none = [bm.ALL] * nframes
    one = list(none)
    one[nframes // 2] = cand[K // 2]
    above = [min(cand[-1] + 5 * f, bm.K_MAX) for f in range(nframes)]
    return none, one, above


pytestmark_gpu = pytest.mark.gpu


@pytestmark_gpu
@pytest.mark.parametrize("name", rc.CALL_NAMES)
def test_device_equals_model(enc, all_calls, name):
    call = all_calls[name]
    curve = curve_of(call)
    for nframes in SPLITS[name]:
        for K, step, base in (FEW if name == "mono_1000" else COMBOS):
            for kind, cap in enumerate(cap_variants(nframes, base, step, K)):
                got = stage(enc, call, nframes, cap, base, step, K)
                want = curve.sums(nframes, cap, base, step, K)
                bad = np.argwhere(got != want)
                assert bad.size == 0, (name, nframes, K, step, base, kind, bad[:4].tolist(), got[tuple(bad[0][:2])].tolist(), want[tuple(bad[0][:2])].tolist())
                if kind == 2:
                    assert (got == got[:, :1, :]).all(), (name, nframes, K, step, base)


@pytestmark_gpu
def test_weights_wrap_per_frame(enc, all_calls):
    """Three frames of 85 blocks: block i takes weight[i % 85]."""
    call = all_calls["mono_255"]
    n1 = 85
    w = np.asarray(call["weight"], dtype=np.float64)[:n1] * np.linspace(0.5, 2.0, n1)
    full = dict(call, weight=np.tile(w, 3), name="mono_255_curve_wrapped")
    curve = bm.Curve(rm.Tables(full["weight"], full["comp"], full["numbps"], full["npasses"], full["pass_rate"], full["pass_dist"]))
    cap = [bm.ALL, 330, bm.ALL]
    want = curve.sums(3, cap, 320, 1, 16)
    assert np.array_equal(stage(enc, full, 3, cap, 320, 1, 16, weight=w), want)
    assert np.array_equal(stage(enc, full, 3, cap, 320, 1, 16), want)
    assert not np.array_equal(want, curve_of(call).sums(3, cap, 320, 1, 16))  # (the weights matter)


def test_the_candidates_cut_blocks_short(all_calls):
    """On the model alone: the comparison is not of trivial answers."""
    for name in ("real97_257", "mono_1000", "spoiled_65"):
        call = all_calls[name]
        tb, curve = rc.tables(call), curve_of(call)
        short = empty = 0
        cands = bm.candidates(320, 16, 64) if name != "mono_1000" else bm.candidates(320, 16, 8)
        for k in cands:
            for b in range(tb.n):
                n = curve.block(b, k)[0]
                short += 0 < n < tb.npasses[b]
                empty += n == 0 and tb.npasses[b] > 0
        sums = [curve.frame(0, tb.n, k) for k in cands]
        assert short and empty and any(a != b for a, b in zip(sums, sums[1:])), (name, short, empty)


@pytestmark_gpu
def test_refusals(api, enc, all_calls):
    call = all_calls["mono_63_one_comp"]

    def refused(nframes=3, cap=None, base=320, step=1, K=16, pending=False):
        cap = [bm.ALL] * max(nframes, 1) if cap is None else cap
        with pytest.raises(api.J2kHipError) as x:
            enc.stage_rate_curve(call["weight"], call["numbps"], call["npasses"], call["pass_rate"], call["pass_dist"], nframes, cap, base, step, K)
        assert x.value.code == 1, str(x.value)  # J2K_HIP_ERR_PARAM
        if pending:
            assert "has not been finished" in str(x.value)

    refused(K=0)
    refused(K=65)
    refused(step=0)
    refused(nframes=2)  # 63 blocks
    refused(nframes=4, cap=[bm.ALL] * 4)
    refused(cap=[bm.ALL, bm.K_MAX + 1, bm.ALL])
    refused(cap=[bm.ALL - 1, bm.ALL, bm.ALL])
    refused(base=bm.ALL - 1)
    refused(base=bm.K_MAX + 1)
    from j2k_amd import synth
    pl = synth.planes(64, 64, 1, 8, 5)
    frame, lay = synth.ae_frame(pl, 8)
    p = api.make_params(64, 64, 1, 8, num_resolutions=3)
    want = enc.encode_host(frame, lay, p)
    enc.encode_begin_host(frame, lay, p)
    refused(pending=True)
    # the refused hook has drained the handle, as every hook does: no frame is pending, and the next one is exact
    with pytest.raises(api.J2kHipError, match="no encode in progress"):
        enc.encode_end()
    assert enc.encode_host(frame, lay, p) == want
    # the handle is as good as before
    cap = [bm.ALL, 322, bm.ALL]
    assert np.array_equal(stage(enc, call, 3, cap, 320, 1, 16), curve_of(call).sums(3, cap, 320, 1, 16))
