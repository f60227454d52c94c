"""GPU: the fused RGBA output stage alone (j2k_hip_stage_rgba_output -> decode_rgba_kernel) against the numpy model
(rgba_model.py), exact equality everywhere.  In every case the WHOLE channel buffer is compared: every byte that is not a
sample of a given destination channel must still hold the fill pattern.

The component samples the model starts from come from decode_output_cases.numpy_decode_output (DC shift, clamp, inverse
component transform), the restatement the plain output stage's tests already pin to the oracle."""
import itertools

import numpy as np
import pytest

import decode_output_cases as doc
import rgba_model as rm
from j2k_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def enc():
    e = api.Encoder(0)
    yield e
    e.close()


def frame(w, h, bits, depth, order="ARGB", rowpad=0, shift=0, alpha=True, cw=None, ch=None):
    """The four samples of interleaved pixels in `order`, `shift` bytes into the buffer: ([R, G, B, A] channels, bytes)."""
    sb = bits // 8
    rb = w * 4 * sb + rowpad
    chans = [doc.chan(shift + order.index(k) * sb, 4 * sb, rb, bits, depth, cw or w, ch or h) for k in "RGBA"]
    if not alpha:
        chans[3] = None
    return chans, shift + rb * h


def planar(w, h, bits, depth, rowpad=3, gap=6, alpha=True, bottom_up=False):
    chans, n = doc.planar(w, h, [(bits, depth)] * 4, rowpad, gap)
    if bottom_up:  # the base is the LAST row of the channel's block, rows go upwards
        for c in chans:
            c["base"] += (h - 1) * c["rowbytes"]
            c["rowbytes"] = -c["rowbytes"]
    if not alpha:
        chans[3] = None
    return chans, n


def expect(chans, nbytes, planes, w, h):
    buf = doc.fill_pattern(nbytes)
    for ch, p in zip(chans, planes):
        if ch is None:
            continue
        cw, chh = min(ch["width"], w), min(ch["height"], h)
        if cw > 0 and chh > 0:
            doc.scatter(buf, ch, np.ascontiguousarray(p[:chh, :cw]).astype(np.uint8 if ch["sample_bits"] == 8 else np.uint16))
    return buf


def check(enc, mode, comps, precs, subs, w, h, rev, chans, nbytes, mct=False, demote=False, lut=None, lut_rgb=(0, 1, 2), org=(0, 0), what="", nmodel=None):
    """nmodel: the components the model is given (sYCC reads three of four)."""
    bits, depth = chans[0]["sample_bits"], chans[0]["depth"]
    m = nmodel or len(comps)
    unsigned = doc.numpy_decode_output(comps[:m], precs[:m], rev, mct)
    planes = rm.rgba(mode, unsigned, precs[:m], subs[:m], w, h, depth, bits, org, lut, lut_rgb, demote)
    want = expect(chans, nbytes, planes, w, h)
    got = enc.stage_rgba_output(comps, precs, subs, w, h, rev, mct, mode, chans, doc.fill_pattern(nbytes), demote=demote, lut=lut,
                                lut_rgb=lut_rgb, org=org)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {bad.size} of {want.size} bytes differ, first at byte {bad[0]} (got {got[bad[0]]}, want {want[bad[0]]}); "
                             f"mode {mode} {w}x{h} precs {precs} subs {subs} org {org} chans {chans}")
    return planes


def signed(rng, prec, shape, rev):
    """Components as the inverse DWT leaves them: around zero, a little beyond the precision's range on both sides."""
    half = 1 << (prec - 1)
    v = rng.integers(-half - 3, half + 3, size=shape)
    return v.astype(np.int32) if rev else (v + rng.uniform(-0.5, 0.5, size=shape)).astype(np.float32)


def comps_for(rng, mode, w, h, prec, rev, subs, org=(0, 0)):
    return [signed(rng, prec, (doc.cdiv(org[1] + h, sy), doc.cdiv(org[0] + w, sx)), rev) for sx, sy in subs]


NCOMP = {rm.RGB: 4, rm.GREY: 2, rm.PALETTE: 1, rm.SYCC: 3}


# ------------------------------------------------------------------------------------------------ sYCC, 8 bit, every triple
_exhaustive = {}


def _all_triples():
    if not _exhaustive:
        v = np.arange(1 << 24, dtype=np.int64).reshape(4096, 4096)
        y, cb, cr = v & 255, (v >> 8) & 255, v >> 16
        _exhaustive["comps"] = [(c - 128).astype(np.int32) for c in (y, cb, cr)]
        _exhaustive["planes"] = rm.rgba(rm.SYCC, [y, cb, cr], [8] * 3, [(1, 1)] * 3, 4096, 4096, 8, 8)
    return _exhaustive


@pytest.mark.parametrize("form", ["packed", "planar"])
def test_sycc_8bit_every_triple(enc, form):
    """A 4096 x 4096 image whose pixels enumerate every (Y, Cb, Cr): 237 of them change when the arithmetic is done exactly
    instead of in float in the stated order, so this pins the order of the operations and the absence of contraction."""
    t = _all_triples()
    chans, n = frame(4096, 4096, 8, 8, "RGBA") if form == "packed" else planar(4096, 4096, 8, 8, rowpad=0, gap=0)
    got = enc.stage_rgba_output(t["comps"], [8] * 3, [(1, 1)] * 3, 4096, 4096, True, False, rm.SYCC, chans, np.full(n, 0x5A, dtype=np.uint8))
    if form == "packed":
        want = np.stack([p.astype(np.uint8) for p in t["planes"]], axis=-1).reshape(-1)
    else:
        want = np.concatenate([p.astype(np.uint8).reshape(-1) for p in t["planes"]])
    assert got.size == want.size
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


# ------------------------------------------------------------------------------------------------ sYCC, 16 bit
@pytest.mark.parametrize("demote", [False, True], ids=["plain", "demote"])
@pytest.mark.parametrize("rev", [True, False], ids=["int", "float"])
@pytest.mark.parametrize("prec", [8, 10, 12, 16])
def test_sycc_16bit_edges_and_random_triples(enc, prec, rev, demote):
    """D = 16 from every precision (the replication comes before the conversion): the edge values {0, 1, h-1, h, h+1, max-1, max}
    crossed on a 257 x 3 image, and 64 K random triples; integer and float components (irreversible, no component transform)."""
    half, top = 1 << (prec - 1), (1 << prec) - 1
    edge = np.array([0, 1, half - 1, half, half + 1, top - 1, top], dtype=np.int64)
    tri = np.array(list(itertools.product(edge, repeat=3)), dtype=np.int64)  # 343 triples
    tri = tri[np.arange(257 * 3) % len(tri)]
    dt = np.int32 if rev else np.float32
    comps = [(tri[:, k] - half).reshape(3, 257).astype(dt) for k in range(3)]
    for form in (frame(257, 3, 16, 16, "ARGB"), planar(257, 3, 16, 16)):
        check(enc, rm.SYCC, comps, [prec] * 3, [(1, 1)] * 3, 257, 3, rev, *form, demote=demote, what="edges")
    rng = np.random.default_rng(prec * 4 + rev * 2 + demote)
    comps = [signed(rng, prec, (256, 256), rev) for _ in range(3)]
    check(enc, rm.SYCC, comps, [prec] * 3, [(1, 1)] * 3, 256, 256, rev, *frame(256, 256, 16, 16, "ARGB"), demote=demote, what="random")


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("mode", [rm.RGB, rm.GREY, rm.PALETTE, rm.SYCC], ids=["rgb", "grey", "palette", "sycc"])
def test_wavefront_and_workgroup_edges_of_both_store_forms(enc, mode):
    rng = np.random.default_rng(mode)
    lut = rng.integers(0, 256, size=(256, 3)).astype(np.uint8) if mode == rm.PALETTE else None
    n = NCOMP[mode]
    for w, h in itertools.product((1, 63, 64, 65, 255, 256, 257), (1, 2, 3)):
        comps = comps_for(rng, mode, w, h, 8, True, [(1, 1)] * n)
        for form in (frame(w, h, 8, 8, "ARGB"), planar(w, h, 8, 8), frame(w, h, 16, 16, "RGBA")):
            check(enc, mode, comps, [8] * n, [(1, 1)] * n, w, h, True, *form, lut=lut, what="shape")


# ------------------------------------------------------------------------------------------------ sub-sampling
@pytest.mark.parametrize("sub", [(2, 2), (2, 1)], ids=["420", "422"])
def test_subsampled_chroma_and_the_replication_phase_of_a_window(enc, sub):
    """Odd widths and heights (the last column and row are replicated from a chroma sample of their own) and every origin
    phase of a window; sYCC, and RGB mode on the same components (a raw 4:2:0 file without a colour space)."""
    rng = np.random.default_rng(sub[1])
    subs = [(1, 1), sub, sub]
    for (w, h), (ox, oy) in itertools.product(((37, 21), (65, 3), (1, 1)), itertools.product(range(4), repeat=2)):
        for mode, rev in ((rm.SYCC, True), (rm.RGB, False)):
            comps = comps_for(rng, mode, w, h, 8, rev, subs, (ox, oy))
            form = frame(w, h, 8, 8, "ARGB") if (ox + oy) % 2 else planar(w, h, 16, 12)
            check(enc, mode, comps, [8] * 3, subs, w, h, rev, *form, org=(ox, oy), what="subsampled")
    # components of unlike precision, and the component transform in front of the conversion
    comps = [signed(rng, p, (doc.cdiv(21, sy), doc.cdiv(37, sx)), True) for p, (sx, sy) in zip((10, 8, 8), subs)]
    check(enc, rm.SYCC, comps, [10, 8, 8], subs, 37, 21, True, *frame(37, 21, 16, 16), what="unlike precisions")
    for rev in (True, False):
        comps = comps_for(rng, rm.SYCC, 65, 5, 8, rev, [(1, 1)] * 3)
        check(enc, rm.SYCC, comps, [8] * 3, [(1, 1)] * 3, 65, 5, rev, *frame(65, 5, 8, 8), mct=True, what="mct")
        comps = comps_for(rng, rm.RGB, 65, 5, 12, rev, [(1, 1)] * 4)
        check(enc, rm.RGB, comps, [12] * 4, [(1, 1)] * 4, 65, 5, rev, *frame(65, 5, 16, 16), mct=True, demote=True, what="mct rgba")


# ------------------------------------------------------------------------------------------------ palette
@pytest.mark.parametrize("entries", [256, 200, 1])
def test_palette(enc, entries):
    """Indices at and above lut_size give 0; the column maps; 8- and 16-bit samples; the entry's value does not depend on D."""
    rng = np.random.default_rng(entries)
    lut = rng.integers(1, 256, size=(entries, 3)).astype(np.uint8)  # (no entry is 0: a miss shows)
    w, h = 65, 4
    idx = rng.integers(0, 256, size=(h, w))
    idx[0, :4] = [0, entries - 1, min(entries, 255), 255]
    comps = [(idx - 128).astype(np.int32)]
    seen = {}
    for cols, (bits, depth) in itertools.product(((0, 1, 2), (2, 1, 0), (1, 2, 0)), ((8, 8), (16, 8), (16, 12), (16, 16))):
        for form in (frame(w, h, bits, depth, "ARGB"), planar(w, h, bits, depth)):
            planes = check(enc, rm.PALETTE, comps, [8], [(1, 1)], w, h, True, *form, lut=lut, lut_rgb=cols, what="palette")
        seen.setdefault((cols, bits), planes[0])
        assert np.array_equal(seen[(cols, bits)], planes[0])  # whatever D
        if entries < 256:
            assert (planes[0][idx >= entries] == 0).all() and (planes[0][idx < entries] != 0).all()
        assert (planes[3] == (1 << depth) - 1).all()
    # indices of 10 bits: most lie beyond the table; a fourth column is ignored
    idx = rng.integers(0, 1024, size=(h, w))
    lut4 = np.concatenate([lut, rng.integers(0, 256, size=(entries, 1)).astype(np.uint8)], axis=1)
    check(enc, rm.PALETTE, [(idx - 512).astype(np.int32)], [10], [(1, 1)], w, h, True, *frame(w, h, 16, 16), lut=lut4, lut_rgb=(2, 0, 1), demote=True,
          what="wide indices")


# ------------------------------------------------------------------------------------------------ destinations
def test_destinations(enc):
    rng = np.random.default_rng(5)
    w, h = 70, 5
    for bits, depth in ((8, 8), (16, 16), (16, 10)):
        sb = bits // 8
        comps4, comps3 = comps_for(rng, rm.RGB, w, h, 8, True, [(1, 1)] * 4), comps_for(rng, rm.SYCC, w, h, 8, True, [(1, 1)] * 3)
        forms = {
            "ARGB": frame(w, h, bits, depth, "ARGB"), "RGBA": frame(w, h, bits, depth, "RGBA"), "BGRA": frame(w, h, bits, depth, "BGRA"),
            "padded rows": frame(w, h, bits, depth, "ARGB", rowpad=4 * sb * 3),
            "rows that are no multiple of the record": frame(w, h, bits, depth, "ARGB", rowpad=sb),
            "record misaligned by one sample": frame(w, h, bits, depth, "ARGB", shift=sb),
            "no alpha": frame(w, h, bits, depth, "ARGB", alpha=False),
            "narrower and shorter": frame(w, h, bits, depth, "ARGB", cw=w - 7, ch=h - 2),
            "planar": planar(w, h, bits, depth), "planar bottom-up": planar(w, h, bits, depth, bottom_up=True),
            "planar without alpha": planar(w, h, bits, depth, alpha=False),
        }
        one_narrow = frame(w, h, bits, depth, "ARGB")
        one_narrow[0][1]["width"] = w - 1  # G alone is narrower: no record stores
        forms["one channel narrower"] = one_narrow
        wider = frame(w + 9, h + 2, bits, depth, "ARGB")  # channels larger than the image: its top-left part is written
        forms["larger than the image"] = wider
        for what, form in forms.items():
            check(enc, rm.RGB, comps4, [8] * 4, [(1, 1)] * 4, w, h, True, *form, what=what)
            check(enc, rm.SYCC, comps3, [8] * 3, [(1, 1)] * 3, w, h, True, *form, demote=depth == 16, what=what)
    # a bottom-up packed frame
    chans, n = frame(w, h, 16, 16, "ARGB", rowpad=16)
    for c in chans:
        c["base"] += (h - 1) * c["rowbytes"]
        c["rowbytes"] = -c["rowbytes"]
    check(enc, rm.RGB, comps4, [8] * 4, [(1, 1)] * 4, w, h, True, chans, n, what="bottom-up records")


@pytest.mark.parametrize("bits,depth", [(8, 8), (16, 10), (16, 16)])
def test_alpha_fill(enc, bits, depth):
    rng = np.random.default_rng(depth)
    w, h = 66, 2
    for mode, n in ((rm.RGB, 3), (rm.GREY, 1), (rm.SYCC, 3), (rm.SYCC, 4)):
        comps = comps_for(rng, mode, w, h, 8, True, [(1, 1)] * n)
        planes = check(enc, mode, comps, [8] * n, [(1, 1)] * n, w, h, True, *frame(w, h, bits, depth), what="fill", nmodel=min(n, 3))
        assert (planes[3] == (1 << depth) - 1).all()
        if depth == 16:
            planes = check(enc, mode, comps, [8] * n, [(1, 1)] * n, w, h, True, *planar(w, h, bits, depth), demote=True, what="fill", nmodel=min(n, 3))
            assert (planes[3] == 32768).all()


def test_refusals_leave_the_buffer_untouched(enc):
    rng = np.random.default_rng(9)
    w, h = 20, 3
    comps = comps_for(rng, rm.RGB, w, h, 8, True, [(1, 1)] * 3)
    ok, n = frame(w, h, 16, 16)

    def refused(chans, nbytes=n, mode=rm.RGB, cs=comps, **kw):
        with pytest.raises(api.J2kHipError) as ei:
            enc.stage_rgba_output(cs, [8] * len(cs), [(1, 1)] * len(cs), w, h, True, False, mode, chans, doc.fill_pattern(nbytes), **kw)
        assert ei.value.code == 1  # J2K_HIP_ERR_PARAM

    mixed = [dict(c) for c in ok]
    mixed[1]["depth"] = 12
    refused(mixed)
    refused(frame(w, h, 8, 8)[0], demote=True)
    refused(frame(w, h, 16, 12)[0], demote=True)
    refused(ok, nbytes=n - 1)                      # the last record leaves the buffer
    refused(frame(w, h, 16, 16, shift=1)[0], nbytes=n + 1)  # 16-bit samples at odd addresses
    refused(ok, mode=rm.GREY)                      # three components are no grey file
    refused(ok, mode=rm.PALETTE, cs=comps[:1], lut=np.zeros((4, 3), np.uint8), lut_rgb=(0, 1, 3))
    refused(ok, mode=7)
    check(enc, rm.RGB, comps, [8] * 3, [(1, 1)] * 3, w, h, True, ok, n, what="and the handle still works")
