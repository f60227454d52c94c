"""GPU: rate_layers_kernel alone (rate.hip; j2k_hip_params.layer_slopes) through j2k_hip_stage_rate_layers, which launches it
as an encode does, against the multi-layer model of tests/slopes_model.py (rate_model.makelayer_plain layer after layer).
Everything compared is an integer: exact equality throughout.  The inputs are the families of test_rate_stage.py -- block
counts 1, 63, 64, 65, 255, 256, 257, 1000: a block range's end inside a wave, on a workgroup's edge and across several -- and
the model is held to the host path on the same inputs in test_slopes_host.py.

  * pass counts and bytes per block and layer equal the model for L = 1, 2, 7 and 100 layers, ordered and unordered lists, with
    thresholds that are negative, 0, 1e-300, just below and at DBL_EPSILON, a run's own slope and one ulp either side, 1e300;
  * what the launch must leave alone still holds the fill: the out arrays' entries behind the last block's (the idle lanes of
    the last wave), and the rows of both pass tables at and beyond npasses, which the caller fills with 0xA5 here;
  * the frames of a sequence share one frame's weights: blocks beyond `nweights` take weight[i % nweights].
"""
import numpy as np
import pytest

import rate_cases as rc
import slopes_model as sm

pytestmark = pytest.mark.gpu

FILL8, FILL32 = 0xA5, 0xA5A5A5A5


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


def filled(call):
    """The call's pass tables with every entry at and beyond npasses set to the fill."""
    rate, dist = call["pass_rate"].copy(), call["pass_dist"].copy()
    for b, k in enumerate(call["npasses"]):
        rate[b, int(k):] = FILL32
        dist[b, int(k):] = FILL32 - (1 << 32)  # (the same bytes as a signed word)
    return rate, dist


def stage(enc, call, slopes, weight=None):
    rate, dist = filled(call)
    out = enc.stage_rate_layers(call["weight"] if weight is None else weight, call["numbps"], call["npasses"], rate, dist, slopes)
    # left alone: the spare entries of both out arrays, and the pass tables whole (their rows beyond npasses with them)
    assert (out["spare_passes"] == FILL8).all() and (out["spare_bytes"] == FILL32).all(), call["name"]
    assert np.array_equal(out["rate_back"], rate) and np.array_equal(out["dist_back"], dist), call["name"]
    return out


@pytest.mark.parametrize("name", rc.CALL_NAMES)
def test_device_equals_model(enc, all_calls, name):
    call = all_calls[name]
    want = sm.model(call)
    assert sorted(set(len(sl) for sl, _, _ in want)) == list(sm.LAYER_COUNTS)
    for k, (sl, passes, nbytes) in enumerate(want):
        out = stage(enc, call, sl)
        assert out["passes"].shape == passes.shape
        bad = np.argwhere(out["passes"] != passes)
        assert bad.size == 0, (name, k, sl[:8], bad[:4].tolist())
        bad = np.argwhere(out["bytes"] != nbytes)
        assert bad.size == 0, (name, k, sl[:8], bad[:4].tolist())


def test_the_lists_cut_blocks_short(all_calls):
    """The comparison is not of trivial answers: on the large families some list leaves blocks short of their passes in its last
    layer, some layer adds passes to a block that has some already, and some block gets nothing at all."""
    for name in ("real97_257", "mono_1000", "spoiled_65"):
        call = all_calls[name]
        total = np.asarray(call["npasses"])
        short = grown = empty = 0
        for sl, passes, _ in sm.model(call):
            short += int(((passes[:, -1] < total)).sum())
            empty += int(((passes[:, -1] == 0) & (total > 0)).sum())
            if passes.shape[1] > 1:
                d = np.diff(passes.astype(int), axis=1)
                grown += int(((d > 0) & (passes[:, :-1] > 0)).sum())
        assert short and grown and empty, (name, short, grown, empty)


def test_weights_wrap_as_the_frames_of_a_sequence(enc, all_calls):
    """Three "frames" of 85 blocks in one table of 255: block i takes weight[i % 85]."""
    call = all_calls["mono_255"]
    n1 = 85
    w = np.asarray(call["weight"], dtype=np.float64)[:n1] * np.linspace(0.5, 2.0, n1)
    full = dict(call, weight=np.tile(w, 3), name="mono_255_wrapped")
    tb = rc.tables(full)
    sl = sm.threshold_lists(tb)[10]
    assert len(sl) == 7
    got = stage(enc, full, sl, weight=w)
    for b in range(tb.n):
        p, q = sm.layers_plain(tb.rate[b], tb.disto[b], sl)
        assert got["passes"][b].tolist() == p and got["bytes"][b].tolist() == q, b
    whole = stage(enc, full, sl)
    assert np.array_equal(whole["passes"], got["passes"]) and np.array_equal(whole["bytes"], got["bytes"])


def test_refusals(api, enc, all_calls):
    call = all_calls["mono_63_one_comp"]
    tb = rc.tables(call)

    def refused(slopes=(1.0,), change=None, weight=None):
        c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in call.items()}
        if change:
            change(c)
        with pytest.raises(api.J2kHipError) as x:
            enc.stage_rate_layers(c["weight"] if weight is None else weight, c["numbps"], c["npasses"], c["pass_rate"], c["pass_dist"], list(slopes))
        assert x.value.code == 1  # J2K_HIP_ERR_PARAM

    def set_(key, i, v):
        def change(c):
            c[key][i] = v
        return change

    b = next(i for i in range(tb.n) if tb.npasses[i] >= 2)
    refused(slopes=[])
    refused(slopes=[1.0] * 101)
    refused(slopes=[1.0, float("nan")])
    refused(slopes=[float("inf")])
    refused(change=set_("npasses", b, 3 * int(call["numbps"][b]) - 1))
    refused(change=set_("numbps", b, 32))
    refused(weight=np.ones(tb.n + 1))
    # the handle is as good as before
    sl, passes, nbytes = sm.model(call)[11]
    out = stage(enc, call, sl)
    assert np.array_equal(out["passes"], passes) and np.array_equal(out["bytes"], nbytes)
