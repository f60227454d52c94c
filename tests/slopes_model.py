"""Layers at given slope thresholds (j2k_hip_params.layer_slopes) in plain Python: the multi-layer driver over
rate_model.makelayer_plain, the threshold lists the tests use, and the case files of tests/native/slopes_host.cpp.  Plain
helpers: no fixtures, no tests.  Shared by test_slopes_host.py (CPU) and test_rate_layers_stage.py (GPU); what the model says of
a call is computed once per process and never changed.

Layer l of a block is opj_tcd_makelayer at slopes[l] on top of the passes of the layers before -- nothing skipped, no
`steepest`, no shortcut -- so the model is independent of rate_block_choose; the distortions are rate_model.disto's, which
test_rate_model.py holds to the library bit for bit.
"""
import struct

import numpy as np

import rate_cases as rc
import rate_model as rm

EPS = rm.DBL_EPSILON
LAYER_COUNTS = (1, 2, 7, 100)


def layers_plain(rate, dis, slopes):
    """(passes in layers 0..l, bytes up to the last of them) for every l."""
    done, passes, nbytes = 0, [], []
    for t in slopes:
        done = rm.makelayer_plain(rate, dis, done, t)
        passes.append(done)
        nbytes.append(rate[done - 1] if done else 0)
    return passes, nbytes


def run_slopes(rate, dis, most=3):
    """Slopes dd / dr of runs the scan really tests, exactly as it forms them: from an empty block, the first step with bytes
    (behind whatever byte-less passes the scan takes on the way); then, with that run taken, the next one; and so on."""
    out, n = [], 0
    for p in range(len(rate)):
        dr = rm.u32(rate[p] - (rate[n - 1] if n else 0))
        dd = dis[p] - (dis[n - 1] if n else 0.0)
        if not dr:
            if dd != 0:
                n = p + 1
            continue
        out.append(dd / dr)
        n = p + 1
        if len(out) == most:
            break
    return out


def edge_values(tb):
    """The thresholds of the issue's list for a call: negative, 0, 1e-300, just below and at DBL_EPSILON, runs' slopes of a few
    blocks with one ulp either side (the thresh - slope < DBL_EPSILON edge), 1e300."""
    vals = [-1.0, 0.0, 1e-300, float(np.nextafter(EPS, 0.0)), EPS, 1e300]
    picked = 0
    for b in range(tb.n):
        if picked == 3:
            break
        s = [v for v in run_slopes(tb.rate[b], tb.disto[b]) if 0 < v < rm.INF]
        if not s:
            continue
        picked += 1
        for v in s:
            vals += [float(np.nextafter(v, -np.inf)), v, float(np.nextafter(v, np.inf))]
    return vals


def threshold_lists(tb):
    """Per layer count of LAYER_COUNTS a few lists, ordered (descending, "everything left" last) and unordered."""
    vals = edge_values(tb)
    slopes = [v for v in vals[6:]] or [1.0, 2.0, 3.0]
    hi = max([tb.bmax[b] for b in range(tb.n) if 0 < tb.bmax[b] < rm.INF] or [1.0])
    lo = min([tb.bmin[b] for b in range(tb.n) if 0 < tb.bmin[b] < rm.DBL_MAX] or [hi * 1e-9])
    lo = min(lo, hi * 1e-3)
    grid = [float(np.exp(np.log(lo) + (np.log(hi) - np.log(lo)) * k / 79)) for k in range(80)]
    rng = np.random.default_rng(len(vals) * 1000 + tb.n)
    desc = lambda v: sorted(v, key=lambda x: (x < 0, -x))  # descending, negative entries last
    lists = [[-1.0], [0.0], [EPS], [slopes[1 % len(slopes)]], [1e300]]
    lists += [[float(np.nextafter(slopes[1 % len(slopes)], np.inf)), float(np.nextafter(slopes[1 % len(slopes)], -np.inf))], [1e300, -1.0], [0.0, 1e-300],
              [float(np.nextafter(EPS, 0.0)), EPS], [slopes[0], slopes[0]]]
    seven = desc([1e300, grid[60], slopes[0], slopes[-1], EPS, 1e-300, -1.0])
    lists += [seven, [seven[i] for i in rng.permutation(7)], [grid[70], -1.0, grid[10], 0.0, slopes[0], grid[40], grid[5]]]
    hundred = desc((vals + slopes + grid)[:100] if len(vals) + len(slopes) + len(grid) >= 100 else (vals + slopes + grid + grid)[:100])
    assert len(hundred) == 100
    lists += [hundred, [hundred[i] for i in rng.permutation(100)]]
    assert sorted(set(len(v) for v in lists)) == list(LAYER_COUNTS)
    return lists


_model = {}


def model(call):
    """[(slopes, passes (n, L) uint8, bytes (n, L) uint32)] for every list of the call."""
    if call["name"] not in _model:
        tb = rc.tables(call)
        out = []
        for sl in threshold_lists(tb):
            p = np.zeros((tb.n, len(sl)), np.uint8)
            q = np.zeros((tb.n, len(sl)), np.uint32)
            for b in range(tb.n):
                p[b], q[b] = layers_plain(tb.rate[b], tb.disto[b], sl)
            out.append((sl, p, q))
        _model[call["name"]] = out
    return _model[call["name"]]


def write_case(path, call, lists):
    """A case file of tests/native/slopes_host.cpp: the call's tables and the threshold lists."""
    with open(path, "wb") as f:
        n = len(call["npasses"])
        f.write(b"RLH1" + struct.pack("<I", n))
        for i in range(n):
            k = int(call["npasses"][i])
            f.write(struct.pack("<dII", float(call["weight"][i]), int(call["numbps"][i]), k))
            f.write(call["pass_rate"][i, :k].astype("<u4").tobytes() + call["pass_dist"][i, :k].astype("<i4").tobytes())
        f.write(struct.pack("<I", len(lists)))
        for sl in lists:
            f.write(struct.pack(f"<I{len(sl)}d", len(sl), *sl))


def read_output(text, n, lists):
    """The program's lines -> [(passes (n, L), bytes (n, L))] per list."""
    out = [(np.zeros((n, len(sl)), np.uint8), np.zeros((n, len(sl)), np.uint32)) for sl in lists]
    seen = 0
    for line in text.splitlines():
        w = line.split()
        if not w or w[0] != "P":
            continue
        k, b, bar = int(w[1]), int(w[2]), w.index("|")
        out[k][0][b] = [int(v) for v in w[3:bar]]
        out[k][1][b] = [int(v) for v in w[bar + 1:]]
        seen += 1
    assert seen == n * len(lists)
    return out
