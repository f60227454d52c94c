"""GPU: decoding into 32-bit float samples (After Effects 32-bpc worlds, sample_bits 32).

A float destination receives the integer of depth d that an integer destination receives, divided by 2^d - 1 (demoted:
Demote's value divided by 32768) -- float_model.py.  So every test runs the same call twice, into integers and into floats,
and compares the floats bit for bit (as uint32) with the model of the integers; the integer side is what the existing decode
tests pin to libopenjp2.  Whole buffers are compared: every byte that is no written float keeps its fill."""
import numpy as np
import pytest

import float_model as fm
import rgba_cases as rc
from conftest import GOLDEN_DIR
from j2k_amd import synth

pytestmark = pytest.mark.gpu

F32 = np.float32
RGB, GREY, PALETTE, SYCC = 1, 2, 3, 4


@pytest.fixture(scope="module")
def api():
    from j2k_amd import api
    return api


@pytest.fixture(scope="module")
def enc(api):
    e = api.Encoder(0)
    yield e
    e.close()


def fill_pattern(n):
    """No byte value repeats at a sample's or a pixel's distance; every seventh 16-byte block holds NaN patterns."""
    b = ((np.arange(n, dtype=np.int64) * 131 + 89) % 251).astype(np.uint8)
    blocks = b[:n - n % 16].reshape(-1, 16)
    blocks[::7] = 0xff
    return b


def chan(base, colbytes, rowbytes, bits, depth, w, h):
    return dict(base=base, colbytes=colbytes, rowbytes=rowbytes, sample_bits=bits, depth=depth, width=w, height=h)


def planar(w, h, bits, n, rowpad=3, gap=8):
    sb, chans, pos = bits // 8, [], gap
    for _ in range(n):
        chans.append((pos, sb, (w + rowpad) * sb))
        pos += (w + rowpad) * sb * h + gap
    return chans, pos


def interleaved(w, h, bits, slots, rowpad_pixels=1):
    """R, G, B, A at slots (samples) of one 4-sample pixel."""
    sb = bits // 8
    rb = (w + rowpad_pixels) * 4 * sb
    return [(s * sb, 4 * sb, rb) for s in slots], rb * h


def gather(buf, geom, sb, w, h):
    base, cb, rb = geom
    idx = base + np.arange(h, dtype=np.int64)[:, None] * rb + np.arange(w, dtype=np.int64)[None, :] * cb
    by = np.stack([buf[idx + k] for k in range(sb)], axis=-1)
    return np.ascontiguousarray(by).view({1: np.uint8, 2: "<u2", 4: "<u4"}[sb]).reshape(h, w)


def scatter(buf, geom, values_u32, w, h):
    base, cb, rb = geom
    idx = base + np.arange(h, dtype=np.int64)[:, None] * rb + np.arange(w, dtype=np.int64)[None, :] * cb
    by = np.ascontiguousarray(values_u32.astype("<u4")).reshape(h, w, 1).view(np.uint8)
    for k in range(4):
        buf[idx + k] = by[:, :, k]


def check_pair(run, int_geoms, int_bits, int_bytes, flt_geoms, flt_bytes, d, w, h, demote=False, what=""):
    """run(geoms, bits, nbytes) -> the buffer after the hook; geoms[c] None: channel absent."""
    ibuf = run(int_geoms, int_bits, int_bytes)
    fbuf = run(flt_geoms, 32, flt_bytes)
    want = fill_pattern(flt_bytes)
    for gi, gf in zip(int_geoms, flt_geoms):
        if gi is None:
            continue
        ints = gather(ibuf, gi, int_bits // 8, w, h).astype(np.int64)
        scatter(want, gf, fm.bits(fm.to_float(ints, d, demoted=demote)), w, h)
    if not np.array_equal(fbuf, want):
        bad = np.flatnonzero(fbuf != want)
        raise AssertionError(f"{what}: {bad.size} of {want.size} bytes differ, first at byte {bad[0]}")


# ------------------------------------------------------------------------------------------------ the plain output stage
def _values(prec, rev, k):
    """Every value of the precision with values beyond both ends around them, as the component words the stage reads."""
    n = (1 << prec) + 16
    v = np.roll(np.arange(-8, n - 8, dtype=np.int64), 37 * k) - (1 << (prec - 1))
    w = 256
    h = -(-n // w)
    v = np.resize(v, w * h).reshape(h, w)
    return (v if rev else (v.astype(np.float64) + (0.25 * k)).astype(F32)), w, h


@pytest.mark.parametrize("prec", [8, 10, 12, 16])
@pytest.mark.parametrize("rev", [True, False], ids=["53", "97"])
def test_output_stage_float_channels_equal_the_model_of_the_integer_ones(enc, rev, prec):
    comps = []
    for k in range(3):
        v, w, h = _values(prec, rev, k)
        comps.append(v)
    for mct in (False, True):
        for d in (8, 16, prec, 5):
            ibits = 8 if d <= 8 else 16

            def run(geoms, bits, nbytes):
                chans = [chan(g[0], g[1], g[2], bits, d, w, h) for g in geoms]
                return enc.stage_decode_output(comps, [prec] * 3, [(1, 1)] * 3, w, h, rev, mct, chans, fill_pattern(nbytes))
            ig, ib = planar(w, h, ibits, 3)
            fg, fb = planar(w, h, 32, 3)
            check_pair(run, ig, ibits, ib, fg, fb, d, w, h, what=f"planar prec {prec} d {d} mct {mct}")
            ig, ib = interleaved(w, h, ibits, (1, 2, 3))
            fg, fb = interleaved(w, h, 32, (1, 2, 3))
            check_pair(run, ig, ibits, ib, fg, fb, d, w, h, what=f"interleaved prec {prec} d {d} mct {mct}")


def test_output_stage_mixed_float_and_integer_channels_and_subsampled_chroma(enc):
    w, h, prec = 67, 9, 10
    rng = np.random.default_rng(3)
    subs = [(1, 1), (2, 2), (2, 1)]
    for rev in (True, False):
        comps = [rng.integers(-600, 600, size=(-(-h // sy), -(-w // sx))).astype(np.int32 if rev else F32) for sx, sy in subs]
        # channel 1 is 16-bit in both runs, channels 0 and 2 are 16-bit in one and float in the other
        g16, n16 = planar(w, h, 16, 3)
        gf = [(8, 4, (w + 3) * 4)]
        pos = 8 + (w + 3) * 4 * h + 8
        gf.append((pos, 2, (w + 3) * 2))
        pos += (w + 3) * 2 * h + 8
        pos += (-pos) % 4
        gf.append((pos, 4, (w + 3) * 4))
        nf = pos + (w + 3) * 4 * h + 8
        ibuf = enc.stage_decode_output(comps, [prec] * 3, subs, w, h, rev, False, [chan(*g, 16, 16, w, h) for g in g16], fill_pattern(n16))
        fbuf = enc.stage_decode_output(comps, [prec] * 3, subs, w, h, rev, False,
                                       [chan(*gf[0], 32, 16, w, h), chan(*gf[1], 16, 16, w, h), chan(*gf[2], 32, 16, w, h)], fill_pattern(nf))
        want = fill_pattern(nf)
        for c in (0, 2):
            scatter(want, gf[c], fm.bits(fm.to_float(gather(ibuf, g16[c], 2, w, h), 16)), w, h)
        mid = gather(ibuf, g16[1], 2, w, h)
        base, cb, rb = gf[1]
        idx = base + np.arange(h)[:, None] * rb + np.arange(w)[None, :] * cb
        want[idx], want[idx + 1] = (mid & 0xff).astype(np.uint8), (mid >> 8).astype(np.uint8)
        assert np.array_equal(fbuf, want), rev


def test_output_stage_refuses_bad_float_channels(api, enc):
    w, h = 6, 4
    comps = [np.zeros((h, w), np.int32)]

    def refused(**kw):
        c = chan(8, 4, 4 * w, 32, 16, w, h)
        c.update(kw)
        with pytest.raises(api.J2kHipError) as e:
            enc.stage_decode_output(comps, [8], [(1, 1)], w, h, True, False, [c], fill_pattern(256))
        assert e.value.code == 1
    for kw in (dict(depth=17), dict(depth=0), dict(base=6), dict(rowbytes=4 * w + 2), dict(colbytes=6), dict(sample_bits=24)):
        refused(**kw)


# ------------------------------------------------------------------------------------------------ the RGBA output stage
def _rgba_comps(rng, mode, ncomp, precs, subs, w, h, org, rev):
    out = []
    for c in range(ncomp):
        sx, sy = subs[c]
        shape = (-(-(org[1] + h) // sy), -(-(org[0] + w) // sx))
        top = 1 << precs[c]
        if mode == PALETTE:
            v = rng.integers(-top // 2 - 2, top // 2 + 2, size=shape)
        else:
            v = rng.integers(-top // 2 - 40, top // 2 + 40, size=shape)
            v.reshape(-1)[:6] = [-top // 2, top // 2 - 1, -top // 2 - 1, top // 2, 0, -1][:v.size]
        out.append(v.astype(np.int32) if rev else (v + rng.uniform(-0.5, 0.5, size=shape)).astype(F32))
    return out


#             mode     ncomp precs             subs                              mct   org
RGBA_CASES = [(RGB, 3, [8, 8, 8], [(1, 1)] * 3, True, (0, 0)),
              (RGB, 4, [16, 16, 16, 16], [(1, 1)] * 4, True, (0, 0)),
              (RGB, 4, [10, 10, 10, 8], [(1, 1)] * 4, False, (3, 1)),
              (GREY, 1, [12], [(1, 1)], False, (0, 0)),
              (GREY, 2, [8, 16], [(1, 1)] * 2, False, (0, 0)),
              (PALETTE, 1, [8], [(1, 1)], False, (0, 0)),
              (SYCC, 3, [8, 8, 8], [(1, 1), (2, 2), (2, 2)], False, (1, 1)),
              (SYCC, 3, [10, 10, 10], [(1, 1), (2, 1), (2, 1)], False, (3, 0)),
              (SYCC, 3, [16, 16, 16], [(1, 1)] * 3, False, (0, 0))]


@pytest.mark.parametrize("case", RGBA_CASES, ids=lambda c: f"mode{c[0]}-{c[1]}comp-p{c[2][0]}-org{c[5][0]}{c[5][1]}")
@pytest.mark.parametrize("rev", [True, False], ids=["53", "97"])
def test_rgba_stage_float_destinations_equal_the_model_of_the_integer_ones(enc, rev, case):
    mode, ncomp, precs, subs, mct, org = case
    w, h = 67, 9
    rng = np.random.default_rng(17 * mode + ncomp + precs[0])
    comps = _rgba_comps(rng, mode, ncomp, precs, subs, w, h, org, rev)
    lut = rng.integers(0, 256, size=(200, 3)).astype(np.uint8) if mode == PALETTE else None
    for d, demote in ((8, False), (16, False), (16, True)):
        ibits = 8 if d == 8 else 16
        for alpha in (True, False):
            for form in ("argb", "rgba", "planar"):
                def run(geoms, bits, nbytes):
                    chans = [None if g is None else chan(g[0], g[1], g[2], bits, d, w, h) for g in geoms]
                    return enc.stage_rgba_output(comps, precs, subs, w, h, rev, mct, mode, chans, fill_pattern(nbytes), demote=demote,
                                                 lut=lut, lut_rgb=(1, 2, 0), org=org)
                if form == "planar":
                    ig, ib = planar(w, h, ibits, 4)
                    fg, fb = planar(w, h, 32, 4)
                else:
                    slots = (1, 2, 3, 0) if form == "argb" else (0, 1, 2, 3)
                    ig, ib = interleaved(w, h, ibits, slots)
                    fg, fb = interleaved(w, h, 32, slots)
                if not alpha:
                    ig[3], fg[3] = None, None
                check_pair(run, ig, ibits, ib, fg, fb, d, w, h, demote=demote, what=f"{form} d {d} demote {demote} alpha {alpha}")


def test_opaque_alpha_fill_is_exactly_one(enc):
    w, h = 5, 3
    comps = [np.zeros((h, w), np.int32)] * 3
    for d, demote in ((8, False), (16, False), (16, True), (11, False)):
        fg, fb = interleaved(w, h, 32, (1, 2, 3, 0))
        chans = [chan(g[0], g[1], g[2], 32, d, w, h) for g in fg]
        buf = enc.stage_rgba_output(comps, [8] * 3, [(1, 1)] * 3, w, h, True, False, RGB, chans, fill_pattern(fb), demote=demote)
        assert np.all(gather(buf, fg[3], 4, w, h) == fm.bits(F32(1.0)))


# ------------------------------------------------------------------------------------------------ whole files
def _load(name):
    import os
    with open(os.path.join(GOLDEN_DIR, name), "rb") as f:
        return f.read()


FILES = {"rgb16_53": lambda: _load("g4_300x200_rgb16_53_rct_tile128.j2k"),
         "rgba8_97_jp2_alpha": lambda: _load("jr1_300x200_rgba8_jp2_srgb_alpha_r30_8.jp2"),
         "palette": lambda: rc.load("pal")}


def _frames(w, h, pad_pixels=1):
    """(ARGB64 frame, layout), (ARGB128 frame, layout), both filled with the pattern."""
    out = []
    for sb in (2, 4):
        rb = (w + pad_pixels) * 4 * sb
        lay = dict(sample_bytes=sb, colbytes=4 * sb, rowbytes=rb, channel_offsets=(0, sb, 2 * sb, 3 * sb))
        if sb == 4:
            lay["depth"] = 16
        out.append((fill_pattern(rb * h), lay))
    return out


def _expect_frame(iframe, ilay, flay, w, h, demote, alpha):
    want = fill_pattern(flay["rowbytes"] * h)
    for k in range(4):  # A, R, G, B
        if k == 0 and not alpha:
            continue
        ints = gather(iframe, (ilay["channel_offsets"][k], 8, ilay["rowbytes"]), 2, w, h)
        scatter(want, (flay["channel_offsets"][k], 16, flay["rowbytes"]), fm.bits(fm.to_float(ints, 16, demoted=demote)), w, h)
    return want


@pytest.mark.parametrize("name", sorted(FILES))
def test_whole_files_into_float_destinations(api, enc, name):
    data = FILES[name]()
    info = api.read_info(data)
    w, h, nc = info["width"], info["height"], info["channels"]
    # decode_channels: padded float arrays against padded 16-bit arrays
    ints = np.zeros((nc, h, w + 3), np.uint16)
    flts = np.full((nc, h, w + 3), np.nan, F32)
    before = flts.copy()
    enc.decode_channels(data, [ints[c, :, :w] for c in range(nc)], depth=16)
    enc.decode_channels(data, [flts[c, :, :w] for c in range(nc)], depth=16)
    assert np.array_equal(fm.bits(flts[:, :, :w]), fm.bits(fm.to_float(ints[:, :, :w], 16)))
    assert np.array_equal(fm.bits(flts[:, :, w:]), fm.bits(before[:, :, w:]))
    # decode_rgba into an ARGB128 frame: host and device destinations, Demote, with and without the alpha destination
    for demote, alpha, device in ((False, True, False), (True, True, True), (False, False, False), (True, False, True)):
        (iframe, ilay), (fframe, flay) = _frames(w, h)
        enc.decode_rgba(data, iframe, ilay, w, h, depth=16, demote=demote, alpha=alpha, device=device)
        enc.decode_rgba(data, fframe, flay, w, h, depth=16, demote=demote, alpha=alpha, device=device)
        assert np.array_equal(fframe, _expect_frame(iframe, ilay, flay, w, h, demote, alpha)), (demote, alpha, device)
    # an odd window, planar
    rect = (7, 3, 45, 21)
    a = enc.decode_region_planar(data, rect, sample_bits=16, depth=16)
    b = enc.decode_region_planar(data, rect, sample_bits=32, depth=16)
    assert b.dtype == F32 and np.array_equal(fm.bits(b), fm.bits(fm.to_float(a, 16)))
    # half size
    a = enc.decode_planar(data, subsample=2, sample_bits=16, depth=16)
    b = enc.decode_planar(data, subsample=2, sample_bits=32, depth=16)
    assert np.array_equal(fm.bits(b), fm.bits(fm.to_float(a, 16)))
    # three frames in one call
    for device in (False, True):
        (i1, ilay), (f1, flay) = _frames(w, h)
        iframes = np.ascontiguousarray(np.stack([i1] * 3))
        fframes = np.ascontiguousarray(np.stack([f1] * 3))
        enc.decode_rgba_sequence([data] * 3, iframes, ilay, w, h, depth=16, demote=True, device=device)
        enc.decode_rgba_sequence([data] * 3, fframes, flay, w, h, depth=16, demote=True, device=device)
        for f in range(3):
            assert np.array_equal(fframes[f], _expect_frame(iframes[f], ilay, flay, w, h, True, True)), (f, device)


def test_sub_sampled_file_and_the_sequence_of_planar_floats(api, enc):
    data = rc.load("k2")  # 65 x 33, sYCC 4:2:2, 10 bits, 9/7
    info = api.read_info(data)
    w, h, nc = info["width"], info["height"], info["channels"]
    a = enc.decode_planar(data, sample_bits=16, depth=16)
    b = enc.decode_planar(data, sample_bits=32, depth=16)
    assert np.array_equal(fm.bits(b), fm.bits(fm.to_float(a, 16)))
    a = enc.decode_planar(data, sample_bits=16)  # the file's own depth: floats of depth 10
    b = enc.decode_planar(data, sample_bits=32)
    assert np.array_equal(fm.bits(b), fm.bits(fm.to_float(a, 10)))
    for device in (False, True):
        s16 = enc.decode_sequence_planar([data] * 3, sample_bits=16, depth=16, device=device)
        s32 = enc.decode_sequence_planar([data] * 3, sample_bits=32, depth=16, device=device)
        assert np.array_equal(fm.bits(s32), fm.bits(fm.to_float(s16, 16)))
    for sub in (1, 2):
        (iframe, ilay), (fframe, flay) = _frames(-(-w // sub), -(-h // sub))
        enc.decode_rgba(data, iframe, ilay, -(-w // sub), -(-h // sub), depth=16, subsample=sub)
        enc.decode_rgba(data, fframe, flay, -(-w // sub), -(-h // sub), depth=16, subsample=sub)
        assert np.array_equal(fframe, _expect_frame(iframe, ilay, flay, -(-w // sub), -(-h // sub), False, True))


def test_refused_float_destinations_are_untouched(api, enc):
    data = FILES["rgb16_53"]()
    w, h = 300, 200
    (_, _), (fframe, flay) = _frames(w, h)
    before = fframe.copy()
    for kw in (dict(depth=17), dict(depth=12, demote=True)):
        with pytest.raises(api.J2kHipError) as e:
            enc.decode_rgba(data, fframe, flay, w, h, **kw)
        assert e.value.code == 1
    bad = dict(flay, rowbytes=flay["rowbytes"] - 2)
    with pytest.raises(api.J2kHipError) as e:
        enc.decode_rgba(data, fframe, bad, w, h, depth=16)
    assert e.value.code == 1 and np.array_equal(fframe, before)


# ------------------------------------------------------------------------------------------------ round trip
@pytest.mark.parametrize("promote", [False, True], ids=["plain", "ae16"])
def test_float_frame_on_the_16_bit_grid_survives_a_lossless_round_trip(api, enc, promote):
    w, h = 131, 67
    pl = synth.planes(w, h, 4, 16, 5)
    if promote:
        pl = fm.promote16(fm.demote16(pl)).astype(np.int32)
    frame, lay = synth.ae_frame_float(pl, 16, row_pad_bytes=16, promote=promote)
    p = api.make_params(w, h, 4, 16, reversible=True, ycc=True, num_resolutions=4, promote=promote, jp2=True, color_space=1, alpha_channel=3)
    cs = enc.encode_host(frame, lay, p)
    back = np.full(frame.size, 0xff, np.uint8)
    enc.decode_rgba(cs, back, lay, w, h, depth=16, demote=promote)
    idx = (np.arange(h)[:, None] * lay["rowbytes"] + np.arange(16 * w)[None, :]).reshape(-1)
    assert np.array_equal(back[idx], frame[idx])
    assert np.all(np.delete(back, idx) == 0xff)
