"""GPU: the rate control's kernels alone (rate.hip: rate_prepare_kernel, rate_ahead_kernel, rate_scan_kernel) through
j2k_hip_stage_rate, which drives them with the objects of an encode (rate_args, RcLayout, HipRateDevice), against the
plain-Python model of tests/rate_model.py.  Everything compared is an integer or a bit pattern: exact equality throughout.
The inputs are those of test_rate_model.py, where the model is held to the code on the host and the inputs are proven fit.

  * prepare: disto as uint64, reach as uint32 and bounds equal the model; entries of a row at and beyond npasses still
    hold the hook's fill (the kernel leaves them alone);
  * scans: taken.lo / hi / n, bytes and sums equal the model at every threshold, through scan and through scan_sums + fetch
    in each of the three slots; a fetch put off until other slots were scanned still returns its own scan;
  * ahead: body equals the model, for the bisection's own list, a list of exactly 128 thresholds and a single one;
  * properties of the device's own outputs against the plain makelayer (rate_cases.check_properties): the shortcut never
    changes a pass count, reach and the ahead walk are bounds (monotone tables), the sums are those of the blocks.

Block counts 1 .. 1000 and the ranges (0, n), (1, 64), (37, 300), (n - 1, 1) put a range's end inside a wave, on a
workgroup's edge (64 for the scan and the prepare kernel, 256 for the walk) and across several workgroups.
"""
import numpy as np
import pytest

import rate_cases as rc
import rate_model as rm

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


@pytest.fixture(scope="module")
def all_calls(oracle):
    return rc.calls(oracle)


def stage(enc, call, **kw):
    return enc.stage_rate(call["weight"], call["comp"], call["numbps"], call["npasses"], call["pass_rate"], call["pass_dist"], **kw)


def scan_modes(api, k):
    """Scan k of a list goes through scan, or through scan_sums + fetch in slot 0, 1 or 2."""
    return [(api.RATE_SCAN, 0), (api.RATE_SUMS_FETCH, 0), (api.RATE_SUMS_FETCH, 1), (api.RATE_SUMS_FETCH, 2)][k % 4]


def device_rows(out, k, count):
    t, b = out["taken"][k], out["bytes"][k]
    return [(int(t["n"][i]), int(t["lo"][i]), int(t["hi"][i]), int(b[i])) for i in range(count)]


def check_prepare(call, tb, out):
    n = tb.n
    fill64, fill32 = 0xA5A5A5A5A5A5A5A5, 0xA5A5A5A5
    d, r = out["disto"].view(np.uint64), out["reach"].view(np.uint32)
    for b in range(n):
        k = tb.npasses[b]
        assert [int(v) for v in d[b, :k]] == [rm.bits64(v) for v in tb.disto[b]], (call["name"], b)
        assert [int(v) for v in r[b, :k]] == [rm.bits32(v) for v in tb.reach[b]], (call["name"], b)
        assert np.all(d[b, k:] == fill64) and np.all(r[b, k:] == fill32), (call["name"], b)  # left alone
    want = [[rm.bits64(v) for v in col] for col in (tb.bmin, tb.bmax, tb.steepest)]
    assert [[int(v) for v in row] for row in out["bounds"].view(np.uint64)] == want, call["name"]


@pytest.mark.parametrize("name", rc.CALL_NAMES)
def test_device_equals_model_and_properties_hold(api, enc, all_calls, name):
    call = all_calls[name]
    tb = rc.tables(call)
    for v, (first, count, done, ahead_name) in enumerate(rc.variants(call, tb)):
        ahead = rc.ahead_lists(tb, first, count)[ahead_name]
        thresholds = rc.variant_thresholds(tb, first, count)
        scans = [(t,) + scan_modes(api, k + v) for k, t in enumerate(thresholds)]
        out = stage(enc, call, first=first, count=count, done=done, ahead=ahead, scans=scans)
        check_prepare(call, tb, out)
        body = [[int(x) for x in row] for row in out["body"]]
        assert body == rm.ahead_range(tb, first, count, done, ahead), (name, v, ahead_name)
        got = []
        for k, t in enumerate(thresholds):
            rows, sums = rm.scan_range(tb, first, count, done, t)
            dev = device_rows(out, k, count)
            assert dev == rows, (name, v, t, scans[k])
            assert [int(x) for x in out["sums"][k]] == sums, (name, v, t, scans[k])
            got.append((dev, [int(x) for x in out["sums"][k]]))
        rc.check_properties(tb, call, first, count, done, thresholds, got, ahead, body)


def test_sums_and_walk_pass_32_bits(all_calls):
    """big_257 is what its name says: a scan's body bytes and the walk's bound exceed 2^32 (the device's sums are compared
    with these in test_device_equals_model_and_properties_hold)."""
    call = all_calls["big_257"]
    tb = rc.tables(call)
    _, sums = rm.scan_range(tb, 0, tb.n, None, -1.0)
    assert all(sums[2 * c] > 1 << 32 for c in range(4))
    body = rm.ahead_range(tb, 0, tb.n, None, rc.ahead_lists(tb, 0, tb.n)["bisection"])
    assert all(body[c][-1] > 1 << 32 for c in range(4))


def test_a_fetch_after_other_slots_were_scanned(api, enc, all_calls):
    """Three scans whose fetches are put off to the end, one per slot, in every order of the slots; then scans into two slots
    with a plain scan (slot 0) last: each fetch returns its own scan's blocks."""
    call = all_calls["mono_255"]
    tb = rc.tables(call)
    first, count = 1, 254
    done = rc.done_values(call, first, count, 5)
    grid = rc.thresholds(tb, first, count)[-9:-1]
    orders = [(0, 1, 2), (2, 1, 0), (1, 2, 0)]
    for o, slots in enumerate(orders):
        ts = [grid[o], grid[o + 3], grid[o + 5]]
        out = stage(enc, call, first=first, count=count, done=done, scans=[(t, api.RATE_SUMS_FETCH_LAST, s) for t, s in zip(ts, slots)])
        for k, t in enumerate(ts):
            rows, sums = rm.scan_range(tb, first, count, done, t)
            assert device_rows(out, k, count) == rows and [int(x) for x in out["sums"][k]] == sums, (slots, k)
    ts = [grid[1], grid[6], grid[3]]
    assert len({tuple(r[0] for r in rm.scan_range(tb, first, count, done, t)[0]) for t in ts}) == 3  # three different candidates
    out = stage(enc, call, first=first, count=count, done=done,
                scans=[(ts[0], api.RATE_SUMS_FETCH_LAST, 1), (ts[1], api.RATE_SUMS_FETCH_LAST, 2), (ts[2], api.RATE_SCAN, 0)])
    for k, t in enumerate(ts):
        rows, sums = rm.scan_range(tb, first, count, done, t)
        assert device_rows(out, k, count) == rows and [int(x) for x in out["sums"][k]] == sums, k


def test_prepare_alone_and_refusals(api, enc, all_calls):
    call = all_calls["mono_63_one_comp"]
    tb = rc.tables(call)
    check_prepare(call, tb, stage(enc, call))
    n = tb.n

    def refused(change=None, **kw):
        c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in call.items()}
        if change:
            change(c)
        with pytest.raises(api.J2kHipError) as x:
            stage(enc, c, **kw)
        assert x.value.code == 1  # J2K_HIP_ERR_PARAM

    def set_(key, i, v):
        def change(c):
            c[key][i] = v
        return change

    b = next(i for i in range(n) if tb.npasses[i] >= 2)
    refused(set_("npasses", b, 3 * int(call["numbps"][b]) - 1))  # more than 3 numbps - 2
    refused(lambda c: (set_("numbps", b, 40)(c), set_("npasses", b, 97)(c)))  # more than 96
    refused(set_("numbps", b, 32))
    refused(set_("comp", b, 4))
    refused(first=0, count=n + 1, scans=[(1.0, api.RATE_SCAN, 0)])
    refused(first=n, count=1, scans=[(1.0, api.RATE_SCAN, 0)])
    refused(first=0, count=0, scans=[(1.0, api.RATE_SCAN, 0)])
    refused(first=0, count=n, ahead=[float(200 - k) for k in range(129)])
    refused(first=0, count=n, ahead=[1.0, 2.0])
    refused(first=0, count=n, scans=[(1.0, api.RATE_SUMS_FETCH, 3)])
    refused(first=0, count=n, scans=[(1.0, 3, 0)])
    refused(first=0, count=n, scans=[(1.0, api.RATE_SUMS_FETCH_LAST, 0), (2.0, api.RATE_SCAN, 0)])
    refused(first=b, count=1, done=[int(call["npasses"][b]) + 1], scans=[(1.0, api.RATE_SCAN, 0)])
    # the handle is as good as before: no encode pending, the same answers
    check_prepare(call, tb, stage(enc, call))
