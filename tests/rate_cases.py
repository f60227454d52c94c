"""Inputs of the rate stage (j2k_hip_stage_rate) and of its host anchor (tests/native/rate_block_host.cpp), shared by
test_rate_model.py and test_rate_stage.py.  Plain helpers: no fixtures, no tests.  Everything comes from seeded numpy
generators; the Tier-1 tables of the `real` families are the CPU oracle's results for the blocks of t1_families.py --
inputs only, never expectations.

A call = dict(name, weight, comp, numbps, npasses, pass_rate (n, 96) uint32, pass_dist (n, 96) int32, monotone: every
block's table is, so the bound properties are claimed).  Block counts 1, 63, 64, 65, 255, 256, 257 and 1000 are the edges
of the kernels' two workgroup sizes (64 and 256) and several workgroups.
"""
import json
import math
import os

import numpy as np

import rate_model as rm
import t1_families as fam

MP = rm.PASSES
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden.json")

# L2 norms of the synthesis basis functions [orient][level] and of the colour transforms, as OpenJPEG tabulates them
NORMS_53 = [[1.000, 1.500, 2.750, 5.375, 10.68, 21.34, 42.67, 85.33, 170.7, 341.3],
            [1.038, 1.592, 2.919, 5.703, 11.33, 22.64, 45.25, 90.48, 180.9, 0],
            [1.038, 1.592, 2.919, 5.703, 11.33, 22.64, 45.25, 90.48, 180.9, 0],
            [.7186, .9218, 1.586, 3.043, 6.019, 12.01, 24.00, 47.97, 95.93, 0]]
NORMS_97 = [[1.000, 1.965, 4.177, 8.403, 16.90, 33.84, 67.69, 135.3, 270.6, 540.9],
            [2.022, 3.989, 8.355, 17.04, 34.27, 68.63, 137.3, 274.6, 549.0, 0],
            [2.022, 3.989, 8.355, 17.04, 34.27, 68.63, 137.3, 274.6, 549.0, 0],
            [2.080, 3.865, 8.307, 17.18, 34.71, 69.59, 139.3, 278.6, 557.2, 0]]
MCT_REV, MCT_REAL = [1.732, .8292, .8292], [1.732, 1.805, 1.573]


def golden_weights(oracle, name):
    """block_weight (rate_control.cpp) of every (component 0..3, resolution, orientation) of a golden case's geometry:
    MCT norm x band norm x step size in that order; component 3 is an alpha channel outside the colour transform."""
    with open(GOLDEN) as f:
        g = json.load(f)[name]
    p = g["params"]
    rev, mct, numres, prec = p.get("reversible", True), p.get("mct", False), p.get("numres", 6), g["prec"]
    out = {}
    for comp in range(4):
        w1 = (MCT_REV if rev else MCT_REAL)[comp] if mct and comp < 3 else 1.0
        for res in range(numres):
            for orient in ([0] if res == 0 else [1, 2, 3]):
                level = numres - 1 - res
                w2 = (NORMS_53 if rev else NORMS_97)[orient][level]
                step = float(np.float32(oracle.band_quant(prec, rev, numres, 0 if res == 0 else 3 * (res - 1) + orient)[3]))
                if not rev:
                    step /= float(1 << (0 if orient == 0 else 2 if orient == 3 else 1))
                out[(comp, res, orient)] = w1 * w2 * step
    return out, numres


_real = {}


def real_tables(oracle):
    """(numbps, rates, nmsedec) of every block of t1_families.py, by the CPU oracle (once per process)."""
    if "t" not in _real:
        rng = np.random.default_rng(20240611)
        blocks = fam.emission_families(rng) + fam.sparse_families(rng)
        out = []
        for blk, o in blocks:
            r = oracle.t1_block((blk.astype(np.int64) << 6).astype(np.int32), o)
            out.append((r["numbps"], r["rates"], r["nmsedec"], o))
        _real["t"] = out
    return _real["t"]


def _pack(name, rows, monotone):
    n = len(rows)
    c = dict(name=name, monotone=monotone, weight=np.zeros(n), comp=np.zeros(n, np.uint8), numbps=np.zeros(n, np.uint32),
             npasses=np.zeros(n, np.uint32), pass_rate=np.zeros((n, MP), np.uint32), pass_dist=np.zeros((n, MP), np.int32))
    for i, (w, comp, nbp, rates, dist) in enumerate(rows):
        assert len(rates) == len(dist) <= MP and (not rates or len(rates) <= 3 * nbp - 2) and nbp <= 31
        c["weight"][i], c["comp"][i], c["numbps"][i], c["npasses"][i] = w, comp, nbp, len(rates)
        c["pass_rate"][i, :len(rates)] = rates
        c["pass_dist"][i, :len(dist)] = dist
    return c


def real_call(oracle, name, golden, n, seed, ncomp=4):
    rng = np.random.default_rng(seed)
    weights, numres = golden_weights(oracle, golden)
    tabs = real_tables(oracle)
    rows = []
    for i in range(n):
        if rng.random() < 0.08:
            rows.append((1.0, int(rng.integers(0, ncomp)), int(rng.integers(0, 12)), [], []))  # an empty block
            continue
        nbp, rates, nms, o = tabs[int(rng.integers(0, len(tabs)))]
        res = 0 if o == 0 else int(rng.integers(1, numres))  # (the LL band is the lowest resolution's alone)
        comp = int(rng.integers(0, ncomp))
        rows.append((weights[(comp, res, o)], comp, nbp, list(rates), list(nms)))
    return _pack(name, rows, True)


def _increments(rng, n, big):
    """n rate increments: about a third 0, else 1, small, or up to 2^20 (big: up to 2^28)."""
    kind = rng.integers(0, 6, size=n)
    top = 1 << (28 if big else 20)
    inc = np.where(kind < 2, 0, np.where(kind == 2, 1, np.where(kind < 5, rng.integers(2, 40, size=n), rng.integers(40, top, size=n))))
    return inc.astype(np.int64)


def _dists(rng, n):
    kind = rng.integers(0, 5, size=n)
    return np.where(kind == 0, 0, np.where(kind == 1, 1, np.where(kind < 4, rng.integers(2, 500, size=n),
                                                                  rng.integers(500, (1 << 31) - 1, size=n, endpoint=True)))).astype(np.int64)


def synthetic_block(rng, shape):
    """One monotone block.  shape picks the pass count ({1, 2, 3 numbps - 2, random}) and where the byte-less runs lie."""
    nbp = int(rng.integers(1, 32))
    most = min(3 * nbp - 2, MP)
    n = [1, 2, most, int(rng.integers(1, most + 1))][shape % 4]
    n = min(n, most)
    inc, dist = _increments(rng, n, False), _dists(rng, n)
    where = (shape // 4) % 5
    run = max(1, n // 4)
    if where == 0:
        inc[:run] = 0  # byte-less passes at the front
    elif where == 1:
        inc[n // 2:n // 2 + run] = 0  # in the middle
    elif where == 2:
        inc[n - run:] = 0  # at the end
    elif where == 3 and shape % 7 == 3:
        inc[:] = 0  # every rate zero
    # byte-less passes with zero and with non-zero distortion
    zero = np.flatnonzero(inc == 0)
    if zero.size:
        dist[zero[::2]] = 0
        dist[zero[1::2]] = rng.integers(1, 1000, size=zero[1::2].size)
    return nbp, [int(v) for v in np.cumsum(inc)], [int(v) for v in dist]


def synthetic_call(name, n, seed, comps=(0, 1, 2, 3), spoil=False):
    """Monotone tables; spoil: every third block gets one rate that steps backwards or one negative distortion sum."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        comp = comps[int(rng.integers(0, len(comps)))]
        w = float(rng.uniform(128.0, 1024.0))  # every non-zero slope of a single pass lies above 1e-6 (2^20 bytes, nmsedec 1, plane 0)
        if rng.random() < 0.1 and n > 1:
            rows.append((w, comp, int(rng.integers(0, 32)), [], []))
            continue
        nbp, rates, dist = synthetic_block(rng, i)
        if spoil and i % 3 == 0 and len(rates) >= 2:
            p = int(rng.integers(1, len(rates)))
            if i % 2 == 0 and rates[p - 1] > 0:
                rates[p] = rates[p - 1] - 1 - int(rng.integers(0, rates[p - 1]))
            else:
                dist[p] = -int(rng.integers(1, 1 << 20))
        rows.append((w, comp, nbp, rates, dist))
    return _pack(name, rows, not spoil)


def big_sum_call(name, n, seed):
    """Rates near 2^31: the body-byte sums of a scan and of the ahead walk pass 2^32 after a few blocks."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        nbp = int(rng.integers(25, 32))
        k = int(rng.integers(1, 6))
        inc = rng.integers(1, 1 << 10, size=k).astype(np.int64)
        inc[0] = (1 << 31) - 1 - int(rng.integers(0, 1 << 12))
        if k > 2:
            inc[1] = (1 << 30) + int(rng.integers(0, 1 << 20))
        rows.append((float(rng.uniform(128.0, 1024.0)), int(rng.integers(0, 4)), nbp, [int(v) for v in np.cumsum(inc)],
                     [int(v) for v in rng.integers(1, 1 << 20, size=k)]))
    return _pack(name, rows, True)


def calls(oracle):
    """Every call of the suite, by name."""
    cs = [real_call(oracle, "real97_257", "c2_4096_rgb8_97", 257, 1),
          real_call(oracle, "real53_65", "c1_512_grey_53", 65, 2),
          synthetic_call("mono_1", 1, 3),
          synthetic_call("mono_63_one_comp", 63, 4, comps=(0,)),
          synthetic_call("mono_64_comp3", 64, 5, comps=(3,)),
          synthetic_call("mono_255", 255, 6),
          synthetic_call("mono_256", 256, 7),
          synthetic_call("mono_1000", 1000, 8),
          synthetic_call("spoiled_65", 65, 9, spoil=True),
          big_sum_call("big_257", 257, 10)]
    return {c["name"]: c for c in cs}


CALL_NAMES = ["real97_257", "real53_65", "mono_1", "mono_63_one_comp", "mono_64_comp3", "mono_255", "mono_256", "mono_1000",
              "spoiled_65", "big_257"]


_tables = {}


def tables(call):
    """The model's tables of a call (rate_model.Tables), made once per process and never changed."""
    if call["name"] not in _tables:
        _tables[call["name"]] = rm.Tables(call["weight"], call["comp"], call["numbps"], call["npasses"], call["pass_rate"], call["pass_dist"])
    return _tables[call["name"]]


def ranges(n):
    """(first, count) of a call with n blocks: the whole call, (1, 64), (37, 300) and the last block, where they fit."""
    out = [(0, n)]
    for r in ((1, 64), (37, 300), (n - 1, 1)):
        if r[0] + r[1] <= n and r not in out:
            out.append(r)
    return out


def done_values(call, first, count, seed):
    """Passes in earlier layers: random in 0..npasses, every fifth block with all of its passes."""
    rng = np.random.default_rng(seed)
    npz = call["npasses"][first:first + count].astype(np.int64)
    d = (rng.random(count) * (npz + 1)).astype(np.int64)
    d[::5] = npz[::5]
    return np.minimum(d, npz).astype(np.uint8)


def thresholds(tb, first, count, grid=8, blocks=4, slopes=6):
    """Scan thresholds of a block range: a negative one, 0, single-pass slopes of a few blocks with both neighbours, a
    geometric grid across the range's [smallest positive bmin, max bmax], one above every
    finite steepest."""
    out = [-1.0, 0.0]
    picked = 0
    for b in range(first, first + count):
        if picked == blocks:
            break
        if tb.npasses[b] < 2 or not tb.monotone(b):
            continue
        picked += 1
        r, d, k = tb.rate[b], tb.disto[b], 0
        for p in range(len(r)):
            dr = r[p] - (r[p - 1] if p else 0)
            if dr > 0 and k < slopes:
                s = (d[p] - (d[p - 1] if p else 0.0)) / dr
                out += [float(np.nextafter(s, -np.inf)), s, float(np.nextafter(s, np.inf))]
                k += 1
    hi = max([tb.bmax[b] for b in range(first, first + count) if tb.bmax[b] > 0] or [1.0])
    lo = min([tb.bmin[b] for b in range(first, first + count) if 0 < tb.bmin[b] < rm.DBL_MAX] or [hi * 1e-9])
    lo = min(lo, hi * 1e-3)
    out += [math.exp(math.log(lo) + (math.log(hi) - math.log(lo)) * k / (grid - 1)) for k in range(grid)]
    steep = [tb.steepest[b] for b in range(first, first + count) if tb.steepest[b] != rm.INF]
    out.append((max(steep) if steep and max(steep) > 0 else 1.0) * 2.0)
    return out


def ahead_lists(tb, first, count):
    """The list the bisection builds from the range's own bounds, an explicit list of exactly 128 descending values, K = 1."""
    rng = range(first, first + count)
    live = [b for b in rng if tb.bmax[b] > 0]
    lo = min([tb.bmin[b] for b in live] or [0.0])
    hi = max([tb.bmax[b] for b in live] or [1.0])
    top = hi if hi > 0 else 1.0
    bottom = max(lo, top * 1e-12)
    explicit = [top * 1.5 * (bottom / (top * 1.5)) ** (k / 127) for k in range(128)]
    assert all(a > b for a, b in zip(explicit, explicit[1:]))
    return dict(bisection=rm.bisection_ahead(lo, hi), explicit128=explicit, one=[(lo + hi) / 2])


# ---- what both test modules do with a call
def bound_threshold(t):
    """Where the two bound properties are asserted: at every threshold.  (The families' weights keep every non-zero slope of
    a single pass above 1e-6, where rate_block_choose's absolute term, thresh - slope < DBL_EPSILON, cannot matter; the
    thresholds around a slope of 0 and the tail of the bisection's list lie below it, and reach carries the term for them:
    test_thresholds_below_the_absolute_term.)"""
    return True


def check_properties(tb, call, first, count, done, thresholds, scans, ahead, body):
    """The properties that test_rate_model.py's docstring lists, on `scans` = per threshold (rows of (n, lo, hi, bytes), sums) and on the ahead
    walk's `body`, whichever side computed them."""
    dn = [0] * count if done is None else [int(v) for v in done]
    for t, (rows, sums) in zip(thresholds, scans):
        want = [0] * 8
        for i in range(count):
            b = first + i
            n = rows[i][0]
            plain = rm.makelayer_plain(tb.rate[b], tb.disto[b], dn[i], t)
            assert n == plain, (call["name"], t, b, n, plain)  # the shortcut never changes a result
            assert rows[i][3] == (tb.rate[b][n - 1] if n else 0)
            lb = rm.layer_bytes(tb.rate[b], dn[i], n)
            want[2 * tb.comp[b]] += lb
            want[2 * tb.comp[b] + 1] += rm.header_bits(n - dn[i], lb)
            if call["monotone"] and bound_threshold(t) and lb:
                assert t <= float(tb.reach[b][n - 1]), (call["name"], t, b, n)  # reach is a bound
        assert list(sums) == want, (call["name"], t)
    if call["monotone"] and ahead:
        for k, t in enumerate(ahead):
            if not bound_threshold(t):
                continue
            plain = [0] * 4
            for i in range(count):
                b = first + i
                plain[tb.comp[b]] += rm.layer_bytes(tb.rate[b], dn[i], rm.makelayer_plain(tb.rate[b], tb.disto[b], dn[i], t))
            for c in range(4):
                assert body[c][k] >= plain[c], (call["name"], "ahead", k, t, c)


def variants(call, tb):
    """(first, count, done, ahead name) of a call: every range without and with passes done, the ahead lists in turn."""
    n = len(call["npasses"])
    out, names = [], ["bisection", "explicit128", "one"]
    for k, (first, count) in enumerate(ranges(n)):
        out.append((first, count, None, names[k % 3]))
        out.append((first, count, done_values(call, first, count, 100 + k), names[(k + 1) % 3]))
    return out


def variant_thresholds(tb, first, count):
    return thresholds(tb, first, count, grid=8, blocks=4, slopes=6) if count <= 300 else thresholds(tb, first, count, grid=6, blocks=2, slopes=3)
