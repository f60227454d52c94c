"""Inputs and references of the decode output stage's tests (test_decode_output.py on the GPU, test_decode_output_refs.py on
the CPU).  Plain helpers, no fixtures: `oracle` is oracle.oracle.Oracle, `enc` is j2k_amd.api.Encoder.

A case is a dict: rev, mct, w, h (the image), comps (one 2-D int32 / float32 plane per component, of ceil(h / sub_y) x
ceil(w / sub_x) samples), precs, subs [(sub_x, sub_y)], chans (dicts like api.Encoder.stage_decode_output takes them: base
is a byte offset), nbytes (the channel buffer's size), stride (words, or None) and a name.

The reference of a case is expected(): Oracle.decode_output (the tail of the oracle's tile decode, which the whole-file tests
pin to libopenjp2), replication by np.repeat(...)[:h, :w], Oracle.copy_channel_out for the depth conversion, scattered into
the fill pattern by plain index arithmetic.  numpy_decode_output() restates the first of these independently.
"""
import itertools

import numpy as np

F32 = np.float32


def fill_pattern(n):
    """What the channel buffer holds before the kernel runs: no byte value repeats at a distance of a sample or a pixel."""
    return ((np.arange(n, dtype=np.int64) * 131 + 89) % 251).astype(np.uint8)


def cdiv(a, b):
    return -(-a // b)


def make_case(name, rev, mct, w, h, comps, precs, subs, chans, nbytes, stride=None):
    dt = np.int32 if rev else np.float32
    comps = [np.ascontiguousarray(c, dtype=dt) for c in comps]
    assert len(comps) == len(precs) == len(subs)
    for c, (sx, sy) in zip(comps, subs):
        assert c.shape == (cdiv(h, sy), cdiv(w, sx)), (name, c.shape, w, h, sx, sy)
    return dict(name=name, rev=rev, mct=mct, w=w, h=h, comps=comps, precs=list(precs), subs=list(subs), chans=chans, nbytes=nbytes,
                stride=stride)


def chan(base, colbytes, rowbytes, bits, depth, width, height):
    return dict(base=base, colbytes=colbytes, rowbytes=rowbytes, sample_bits=bits, depth=depth, width=width, height=height)


def planar(w, h, specs, rowpad=3, gap=5):
    """One padded planar channel per (sample_bits, depth) of specs, one behind the other with `gap` bytes between them."""
    chans, pos = [], gap
    for bits, depth in specs:
        sb = bits // 8
        pos += pos % sb
        rb = (w + rowpad) * sb
        chans.append(chan(pos, sb, rb, bits, depth, w, h))
        pos += rb * h + gap
    return chans, pos


def interleaved(w, h, bits, depth, offsets, pixel, rowpad):
    """Samples of interleaved pixels of `pixel` bytes: channel c at byte offsets[c] of every pixel."""
    rb = w * pixel + rowpad
    return [chan(o, pixel, rb, bits, depth, w, h) for o in offsets], rb * h


# ------------------------------------------------------------------------------------------------ running and references
def run(enc, case):
    return enc.stage_decode_output(case["comps"], case["precs"], case["subs"], case["w"], case["h"], case["rev"], case["mct"],
                                   case["chans"], fill_pattern(case["nbytes"]), stride=case["stride"])


def scatter(buf, ch, dense):
    """dense: (rows, cols) uint8 / uint16 samples -> the bytes of channel `ch` in buf (little-endian, like the device)."""
    rows, cols = dense.shape
    sb = dense.itemsize
    idx = ch["base"] + np.arange(rows, dtype=np.int64)[:, None] * ch["rowbytes"] + np.arange(cols, dtype=np.int64)[None, :] * ch["colbytes"]
    assert idx.min() >= 0 and idx.max() + sb <= buf.size, "the case's own channel leaves its buffer"
    by = dense.reshape(rows, cols, 1).view(np.uint8) if sb == 1 else dense.astype("<u2").reshape(rows, cols, 1).view(np.uint8)
    for k in range(sb):
        buf[idx + k] = by[:, :, k]


def expected(oracle, case, planes=None):
    """The whole channel buffer as the kernel must leave it.  planes: the samples per component (default: the oracle's)."""
    w, h = case["w"], case["h"]
    if planes is None:
        planes = oracle.decode_output(case["comps"], case["precs"], case["rev"], case["mct"])
    buf = fill_pattern(case["nbytes"])
    for c in range(min(len(case["chans"]), len(planes))):
        ch = case["chans"][c]
        sx, sy = case["subs"][c]
        full = np.repeat(np.repeat(planes[c], sy, axis=0), sx, axis=1)[:h, :w]
        cw, chh = min(ch["width"], w), min(ch["height"], h)
        if cw <= 0 or chh <= 0:
            continue
        sb = ch["sample_bits"] // 8
        dense = oracle.copy_channel_out(full[:chh, :cw], case["precs"][c], sb, ch["depth"], sb, cw * sb, cw, chh)
        scatter(buf, ch, dense.view(np.uint8 if sb == 1 else np.uint16).reshape(chh, cw))
    return buf


def assert_buffers_equal(got, want, case):
    if np.array_equal(got, want):
        return
    bad = np.flatnonzero(got != want)
    raise AssertionError(f"{case['name']}: {bad.size} of {want.size} bytes differ, first at byte {bad[0]} "
                         f"(got {got[bad[0]]}, want {want[bad[0]]}, fill {fill_pattern(int(bad[0]) + 1)[-1]}); "
                         f"precs {case['precs']} subs {case['subs']} chans {case['chans']}")


def numpy_decode_output(comps, precs, rev, mct):
    """Independent restatement of Oracle.decode_output.  Reversible: int64 throughout.  Irreversible: np.float32 operation by
    operation in libopenjp2's order, the explicit limits (above 2^31 - 1 as a float the highest value, below -2^31 and NaN the
    lowest), np.rint (to nearest even), int64 add, clip."""
    out = []
    if rev:
        s = [np.asarray(c).astype(np.int64) for c in comps]
        if mct:
            y, u, v = s[:3]
            g = y - ((u + v) >> 2)
            s[:3] = [v + g, g, u + g]
        for c, p in zip(s, precs):
            out.append(np.clip(c + (1 << (p - 1)), 0, (1 << p) - 1).astype(np.int32))
        return out
    f = [np.asarray(c, dtype=F32) for c in comps]
    with np.errstate(all="ignore"):
        if mct:
            y, u, v = f[:3]
            r = y + v * F32(1.402)
            g = (y - u * F32(0.34413)) - v * F32(0.71414)
            b = y + u * F32(1.772)
            assert r.dtype == g.dtype == b.dtype == F32
            f[:3] = [r, g, b]
        for c, p in zip(f, precs):
            nan, hi, lo = np.isnan(c), c > F32(2147483647.0), c < F32(-2147483648.0)
            t = np.rint(np.where(nan | hi | lo, F32(0), c)).astype(np.int64) + (1 << (p - 1))
            t = np.clip(t, 0, (1 << p) - 1)
            t[hi] = (1 << p) - 1
            t[lo | nan] = 0
            out.append(t.astype(np.int32))
    return out


# ------------------------------------------------------------------------------------------------ depth conversion
def depth_triples():
    """Every (cprec, sample_bits, depth): 16 x (8 + 16) = 384."""
    return [(p, bits, d) for p in range(1, 17) for bits in (8, 16) for d in range(1, bits + 1)]


def depth_cases():
    """All 384 triples, four to a call (one precision per call, 8- and 16-bit channels mixed), every sample value 0 ..
    2^cprec - 1 in each channel: reversible, no MCT, input word = value - 2^(cprec - 1).  Channel c holds the values rotated
    by 37 c places, so that a channel that took another's samples shows."""
    cases = []
    for p in range(1, 17):
        mine = [(bits, d) for (q, bits, d) in depth_triples() if q == p]
        n = 1 << p
        w = min(n, 256)
        h = n // w
        for g in range(6):
            specs = mine[g::6]
            assert len(specs) == 4
            comps = [(np.roll(np.arange(n, dtype=np.int64), 37 * c) - (n >> 1)).reshape(h, w) for c in range(4)]
            chans, nbytes = planar(w, h, specs)
            cases.append(make_case(f"depth p{p} {specs}", True, False, w, h, comps, [p] * 4, [(1, 1)] * 4, chans, nbytes))
    return cases


# ------------------------------------------------------------------------------------------------ clamp, reversible
CLAMP_PRECS = (1, 7, 8, 12, 16)


def clamp_values(p):
    lo, hi = -(1 << (p - 1)), (1 << (p - 1)) - 1
    return [lo - 2, lo - 1, lo, lo + 1, -1, 0, 1, hi - 1, hi, hi + 1, hi + 2, -(1 << 30), 1 << 30, -(1 << 30) + 1, (1 << 30) - 1, lo - 1000, hi + 1000]


def rct_forward(r, g, b):
    """T.800 G.2.1 on int64 (exactly undone by G.2.2 whatever the values)."""
    return (r + 2 * g + b) >> 2, b - g, r - g


def clamp_rev_cases():
    cases = []
    for p in CLAMP_PRECS:  # without MCT: two components, the second holds the values in reverse
        v = np.array(clamp_values(p), dtype=np.int64)
        comps = [np.stack([v, -v]), np.stack([v[::-1], v])]
        w, h = v.size, 2
        chans, nbytes = planar(w, h, [(8, min(p, 8)), (16, p)])
        cases.append(make_case(f"clamp rev p{p}", True, False, w, h, comps, [p, p], [(1, 1)] * 2, chans, nbytes))
    for p, p4 in ((8, 12), (12, 16), (16, 7), (1, 8), (7, 1)):  # with MCT: target (R, G, B) triples through the forward RCT
        lo, hi = -(1 << (p - 1)), (1 << (p - 1)) - 1
        per = [lo - 1000, lo - 1, lo, -1, 0, hi, hi + 1, hi + 1000]
        rgb = np.array(list(itertools.product(per, repeat=3)), dtype=np.int64)  # 512 triples
        y, u, v = rct_forward(rgb[:, 0], rgb[:, 1], rgb[:, 2])
        w, h = 64, 8
        fourth = np.resize(np.array(clamp_values(p4), dtype=np.int64), w * h)
        comps = [a.reshape(h, w) for a in (y, u, v, fourth)]
        chans, nbytes = planar(w, h, [(16, p), (16, p), (16, p), (16, p4)])
        cases.append(make_case(f"clamp rct p{p}", True, True, w, h, comps, [p, p, p, p4], [(1, 1)] * 4, chans, nbytes))
    return cases


# ------------------------------------------------------------------------------------------------ float conversion
FLOAT_PRECS = (8, 12, 16)


def bits_to_f32(bits):
    return np.array(bits, dtype=np.uint32).view(F32)


def float_specials(p):
    lo, hi = -float(1 << (p - 1)), float((1 << (p - 1)) - 1)
    ties = [k + 0.5 for k in range(-6, 6)] + [126.5, 127.5, -127.5, -128.5, 2047.5, -2048.5, 32766.5, 32767.5, -32768.5, -32769.5]
    edge = [lo, lo - 0.49, lo - 0.5, lo - 0.51, lo - 1, lo + 0.49, lo + 0.5, hi, hi + 0.49, hi + 0.5, hi + 0.51, hi + 1, hi - 0.5]
    far = [2.0 ** 31 - 128, -(2.0 ** 31 - 128), 2.0 ** 31, -(2.0 ** 31), 3e9, -3e9, 1e30, -1e30]
    v = np.array(ties + edge + far + [0.0, -0.0], dtype=F32)
    v = np.concatenate([v, np.nextafter(F32([lo - 0.5, lo - 0.5, hi + 0.5, hi + 0.5, 2.0 ** 31, -(2.0 ** 31), -(2.0 ** 31)]),
                                        F32([-np.inf, np.inf, -np.inf, np.inf, np.inf, -np.inf, np.inf]))])
    raw = bits_to_f32([0x00000001, 0x80000001, 0x007fffff, 0x807fffff,       # denormals
                       0x7f7fffff, 0xff7fffff, 0x7f800000, 0xff800000,       # +-FLT_MAX, +-inf
                       0x7fc00000, 0xffc00000, 0x7f800001, 0xffbfffff])      # NaNs: quiet, negative, signalling
    return np.concatenate([v, raw])


def float_classes(a):
    """Which of the listed classes of floats an array holds."""
    a = np.asarray(a, dtype=F32).ravel()
    bits = a.view(np.uint32)
    fin = np.isfinite(a)
    small = fin & (np.abs(np.where(fin, a, 0)) < 2.0 ** 22)
    k = np.floor(np.where(small, a, 0).astype(np.float64))
    tie = small & (np.where(small, a, 0).astype(np.float64) - k == 0.5)
    two31 = F32(2.0 ** 31)
    return {
        "tie above an even integer, positive": bool((tie & (k % 2 == 0) & (a > 0)).any()),
        "tie above an odd integer, positive": bool((tie & (k % 2 == 1) & (a > 0)).any()),
        "tie above an even integer, negative": bool((tie & (k % 2 == 0) & (a < 0)).any()),
        "tie above an odd integer, negative": bool((tie & (k % 2 == 1) & (a < 0)).any()),
        "+0": bool((bits == 0).any()), "-0": bool((bits == 0x80000000).any()),
        "denormal, positive": bool(((bits > 0) & (bits < 0x00800000)).any()),
        "denormal, negative": bool(((bits > 0x80000000) & (bits < 0x80800000)).any()),
        "2^31 - 128": bool((a == F32(2.0 ** 31 - 128)).any()), "-(2^31 - 128)": bool((a == -F32(2.0 ** 31 - 128)).any()),
        "2^31": bool((a == two31).any()), "-2^31": bool((a == -two31).any()),
        "just above 2^31": bool((a == np.nextafter(two31, F32(np.inf))).any()),
        "just below -2^31": bool((a == np.nextafter(-two31, F32(-np.inf))).any()),
        "3e9": bool((a == F32(3e9)).any()), "-3e9": bool((a == F32(-3e9)).any()),
        "1e30": bool((a == F32(1e30)).any()), "-1e30": bool((a == F32(-1e30)).any()),
        "FLT_MAX": bool((bits == 0x7f7fffff).any()), "-FLT_MAX": bool((bits == 0xff7fffff).any()),
        "+inf": bool((bits == 0x7f800000).any()), "-inf": bool((bits == 0xff800000).any()),
        "NaN": bool(np.isnan(a).any()),
    }


def clamp_edge_classes(a, p):
    """Values just inside and just outside either end of the clamp of precision p (after rounding)."""
    a = np.asarray(a, dtype=F32).ravel()
    lo, hi = -float(1 << (p - 1)), float((1 << (p - 1)) - 1)
    fin = np.isfinite(a)
    r = np.rint(np.where(fin, a, 0).astype(np.float64))
    frac = fin & (np.where(fin, a, 0) != r)
    return {"inside the low end": bool((frac & (r == lo)).any()), "outside the low end": bool((frac & (r == lo - 1)).any()),
            "inside the high end": bool((frac & (r == hi)).any()), "outside the high end": bool((frac & (r == hi + 1)).any())}


def float_cases():
    """Irreversible planes of 128 x 32.  Without MCT: the special values, random 32-bit patterns and standard_normal x
    2^(p-1) planes, each in some component.  With MCT: the special values in each of Y, U and V in turn beside two ordinary
    values, then random patterns and ordinary values in all three; the fourth component rides along."""
    cases = []
    w, h = 128, 32
    n = w * h
    for p in FLOAT_PRECS:
        rng = np.random.default_rng(3100 + p)
        sp = float_specials(p)
        patterns = lambda: rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(F32)
        normal = lambda scale=1.0: (rng.standard_normal(n) * (1 << (p - 1)) * scale).astype(F32)
        a = patterns()
        a[:sp.size] = sp
        d = normal()
        d[:sp.size] = sp[::-1]
        comps = [x.reshape(h, w) for x in (a, normal(), patterns(), d)]
        chans, nbytes = planar(w, h, [(16, p), (16, p), (8, 8), (16, 16)])
        cases.append(make_case(f"float p{p}", False, False, w, h, comps, [p] * 4, [(1, 1)] * 4, chans, nbytes))
        yuv = [normal(0.5), normal(0.25), normal(0.25)]
        for i in range(3 * sp.size):  # special value i // 3 in component i % 3
            yuv[i % 3][i] = sp[i // 3]
        k = 3 * sp.size
        pats = [patterns() for _ in range(3)]
        for c in range(3):
            yuv[c][k:k + 1024] = pats[c][:1024]
        comps = [x.reshape(h, w) for x in yuv + [a[::-1].copy()]]
        chans, nbytes = planar(w, h, [(16, p), (8, min(p, 8)), (16, 16), (16, p)])
        cases.append(make_case(f"float ict p{p}", False, True, w, h, comps, [p] * 4, [(1, 1)] * 4, chans, nbytes))
        # ordinary planes alone, many samples: where the order of the transform's operations shows in the last bit
        W, H = 512, 256
        big = [(rng.standard_normal((H, W)) * (1 << (p - 1)) * s).astype(F32) for s in (0.5, 0.25, 0.25)]
        chans, nbytes = planar(W, H, [(16, p)] * 3, rowpad=0)
        cases.append(make_case(f"float ict planes p{p}", False, True, W, H, big, [p] * 3, [(1, 1)] * 3, chans, nbytes))
    return cases


# ------------------------------------------------------------------------------------------------ launch shape
SHAPES = [(1, 3), (255, 3), (256, 3), (257, 3), (513, 3), (1000, 3), (3, 70000)]


def _noisy(rng, shape, p, rev):
    """Values over twice the nominal range of precision p: every row and column unlike its neighbours, both clamp ends reached."""
    v = rng.integers(-(1 << p), 1 << p, shape)
    return v if rev else (v + rng.integers(0, 4, shape) * 0.25).astype(F32)


def shape_cases():
    cases = []
    rng = np.random.default_rng(7100)
    for rev in (True, False):
        for (w, h) in SHAPES:
            comps = [_noisy(rng, (h, w), 8, rev) for _ in range(3)]
            chans, nbytes = planar(w, h, [(8, 8)] * 3, rowpad=1)
            cases.append(make_case(f"shape {w}x{h} {'rev' if rev else 'irr'}", rev, True, w, h, comps, [8] * 3, [(1, 1)] * 3, chans, nbytes))
        w, h = 300, 5  # a stride larger than the width (the words between hold NaN bit patterns: api.stage_decode_output)
        comps = [_noisy(rng, (h, w), 8, rev) for _ in range(3)]
        chans, nbytes = planar(w, h, [(8, 8)] * 3)
        cases.append(make_case(f"stride 320 {'rev' if rev else 'irr'}", rev, False, w, h, comps, [8] * 3, [(1, 1)] * 3, chans, nbytes, stride=320))
    return cases


# ------------------------------------------------------------------------------------------------ sub-sampling
def _sub_comps(rng, w, h, precs, subs, rev):
    return [_noisy(rng, (cdiv(h, sy), cdiv(w, sx)), p, rev) for p, (sx, sy) in zip(precs, subs)]


def subsampling_cases():
    cases = []
    rng = np.random.default_rng(4200)
    mixes = [[(1, 1), (2, 3), (4, 1), (3, 4)], [(3, 2), (1, 4), (2, 2), (4, 3)], [(4, 4), (3, 1), (1, 2), (2, 1)]]
    precs = [8, 5, 12, 16]
    # 13 = 6 x 2 + 1 = 4 x 3 + 1 = 3 x 4 + 1 and 9 = 4 x 2 + 1 = 2 x 4 + 1: the last sample of a component is replicated once
    for (w, h) in [(13, 9), (12, 10), (10, 7), (1, 1)]:
        for subs in mixes:
            for rev in (True, False):
                comps = _sub_comps(rng, w, h, precs, subs, rev)
                chans, nbytes = planar(w, h, [(8, 8), (8, 5), (16, 12), (16, 16)])
                cases.append(make_case(f"sub {w}x{h} {subs} {'rev' if rev else 'irr'}", rev, False, w, h, comps, precs, subs, chans, nbytes))
    for name, subs in (("4:2:0", [(1, 1), (2, 2), (2, 2)]), ("4:2:2", [(1, 1), (2, 1), (2, 1)])):
        for p in (8, 10):
            for rev in (True, False):
                w, h = 35, 21
                comps = _sub_comps(rng, w, h, [p] * 3, subs, rev)
                chans, nbytes = planar(w, h, [(8 if p == 8 else 16, p)] * 3)
                cases.append(make_case(f"sub {name} {p} bits {'rev' if rev else 'irr'}", rev, False, w, h, comps, [p] * 3, subs, chans, nbytes))
    for rev in (True, False):  # the colour transform on three components sub-sampled alike, a fourth on the full grid
        w, h, subs, precs4 = 21, 13, [(2, 2)] * 3 + [(1, 1)], [8, 8, 8, 11]
        comps = _sub_comps(rng, w, h, precs4, subs, rev)
        chans, nbytes = planar(w, h, [(8, 8)] * 3 + [(16, 11)])
        cases.append(make_case(f"sub mct {'rev' if rev else 'irr'}", rev, True, w, h, comps, precs4, subs, chans, nbytes))
    return cases


# ------------------------------------------------------------------------------------------------ destination geometry
def geometry_cases():
    cases = []
    rng = np.random.default_rng(5300)
    w, h = 19, 7

    def add(name, rev, mct, precs, chans, nbytes, ncomp=None):
        ncomp = ncomp or len(precs)
        comps = [_noisy(rng, (h, w), p, rev) for p in precs[:ncomp]]
        cases.append(make_case(f"geometry {name} {'rev' if rev else 'irr'}", rev, mct, w, h, comps, precs[:ncomp], [(1, 1)] * ncomp, chans, nbytes))

    for rev in (True, False):
        for nch in (3, 4):  # After Effects frames: A R G B samples, codec channels R, G, B[, A]
            chans, nbytes = interleaved(w, h, 8, 8, [1, 2, 3, 0][:nch], 4, 12)
            add(f"ARGB32 {nch} channels", rev, True, [8] * nch, chans, nbytes)
            chans, nbytes = interleaved(w, h, 16, 16, [2, 4, 6, 0][:nch], 8, 16)
            add(f"ARGB64 {nch} channels", rev, True, [16] * nch, chans, nbytes)
        chans, nbytes = interleaved(w, h, 16, 16, [2, 4, 6, 0], 8, 16)  # ARGB64 of 15-bit + 1 samples from a 12-bit file
        for ch in chans:
            ch["depth"] = 15
        add("ARGB64 depth 15", rev, True, [12] * 4, chans, nbytes)
        chans, nbytes = planar(w, h, [(8, 8), (16, 10), (8, 8)], rowpad=7, gap=11)
        add("planar padded", rev, False, [8, 10, 8], chans, nbytes)
        chans, nbytes = planar(w, h, [(8, 8), (16, 12), (8, 8)], rowpad=2)
        for ch in chans:  # bottom-up rows: base is the last row of the region, rowbytes negative
            ch["base"] += (h - 1) * ch["rowbytes"]
            ch["rowbytes"] = -ch["rowbytes"]
        add("bottom-up", rev, False, [8, 12, 8], chans, nbytes)
        chans, nbytes = interleaved(w, h, 8, 8, [0, 1, 2], 3, 1)
        add("3-byte pixels", rev, True, [8] * 3, chans, nbytes)
        chans, nbytes = planar(w, h, [(8, 8), (8, 8)])
        add("two channels of four components", rev, True, [8] * 4, chans, nbytes)
        chans, nbytes = planar(w, h, [(8, 8), (16, 9), (8, 8)])
        add("three channels of two components", rev, False, [8, 9, 8], chans, nbytes, ncomp=2)
        chans, nbytes = planar(w, h, [(8, 8), (16, 16), (8, 6), (16, 11)])
        for ch, (cw, chh) in zip(chans, [(w - 3, h), (w, h - 2), (1, 1), (w - 1, h - 1)]):
            ch["width"], ch["height"] = cw, chh
        add("smaller destinations", rev, False, [8, 16, 8, 11], chans, nbytes)
        chans, nbytes = planar(w, h, [(8, 8), (16, 16), (8, 8)])
        for ch, (cw, chh) in zip(chans, [(w + 5, h + 3), (w + 1, h), (w, 1 << 20)]):
            ch["width"], ch["height"] = cw, chh
        add("larger destinations", rev, True, [8, 8, 8], chans, nbytes)
        chans, nbytes = planar(w, h, [(8, 8), (16, 12), (8, 3), (16, 16)])
        add("mixed sample types", rev, False, [12, 12, 12, 12], chans, nbytes)
    return cases


def all_cases():
    return depth_cases() + clamp_rev_cases() + float_cases() + shape_cases() + subsampling_cases() + geometry_cases()
