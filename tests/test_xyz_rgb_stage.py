"""GPU: the X'Y'Z' -> R'G'B' variants of the RGBA output kernel through j2k_hip_stage_rgba_output_xyz against the numpy model
(xyz_inverse_model.py) fed with the library's own tables (api.xyz_inverse_tables): exact equality, and the WHOLE channel
buffer is compared -- every byte that is no sample of a given channel keeps its fill.

The component samples the model starts from come from decode_output_cases.numpy_decode_output (DC shift, clamp, inverse
component transform), the restatement the plain output stage's tests pin to the oracle.  Shapes are the smallest at which the
indexing can go wrong: one lane, one lane short of / exactly / one lane past a workgroup's 256 columns; one row, two rows, 70
rows, and (a test of its own, three columns wide) more rows than the LDS variants' grid has workgroups.  (P, D) = (8, 8), (12, 8), (10, 10): both tables in
LDS; (12, 16), (16, 16): both in global memory."""
import itertools

import numpy as np
import pytest

import decode_output_cases as doc
import float_model as fm
import rgba_model as rm
import xyz_inverse_model as xim
from j2k_amd import api

pytestmark = pytest.mark.gpu

J2K_HIP_ERR_PARAM = 1


@pytest.fixture(scope="module")
def enc():
    e = api.Encoder(0)
    yield e
    e.close()


_tables = {}


def tables(target, comp_depth, dst_depth):
    key = (target, comp_depth, dst_depth)
    if key not in _tables:
        _tables[key] = api.xyz_inverse_tables(target, comp_depth, dst_depth)
    return _tables[key]


def frame(w, h, bits, depth, order="ARGB", rowpad=0, alpha=True):
    """The four samples of interleaved pixels in `order` (the packed form: ARGB32 / ARGB64 / ARGB128)."""
    sb = bits // 8
    rb = w * 4 * sb + rowpad
    chans = [doc.chan(order.index(k) * sb, 4 * sb, rb, bits, depth, w, h) for k in "RGBA"]
    if not alpha:
        chans[3] = None
    return chans, rb * h


def planar(w, h, bits, depth, alpha=True, bottom_up=False):
    """Four padded planes one behind the other (the general strided form); float samples on the 4-byte grid."""
    sb = bits // 8
    chans, pos = [], 8
    for _ in range(4):
        rb = (w + 3) * sb
        chans.append(doc.chan(pos, sb, rb, bits, depth, w, h))
        pos += rb * h + 8
    if bottom_up:
        for c in chans:
            c["base"] += (h - 1) * c["rowbytes"]
            c["rowbytes"] = -c["rowbytes"]
    if not alpha:
        chans[3] = None
    return chans, pos


def scatter(buf, ch, values, sb):
    rows, cols = values.shape
    idx = ch["base"] + np.arange(rows, dtype=np.int64)[:, None] * ch["rowbytes"] + np.arange(cols, dtype=np.int64)[None, :] * ch["colbytes"]
    assert idx.min() >= 0 and idx.max() + sb <= buf.size
    by = np.ascontiguousarray(values.astype({1: np.uint8, 2: "<u2", 4: "<u4"}[sb])).reshape(rows, cols, 1).view(np.uint8)
    for k in range(sb):
        buf[idx + k] = by[:, :, k]


def expect(chans, nbytes, planes, w, h, demote):
    buf = doc.fill_pattern(nbytes)
    for ch, p in zip(chans, planes):
        if ch is None:
            continue
        cw, chh = min(ch["width"], w), min(ch["height"], h)
        if cw <= 0 or chh <= 0:
            continue
        v = p[:chh, :cw]
        if ch["sample_bits"] == 32:
            scatter(buf, ch, fm.bits(fm.to_float(v, ch["depth"], demoted=demote)), 4)
        else:
            scatter(buf, ch, v, ch["sample_bits"] // 8)
    return buf


def check(enc, target, comps, precs, subs, w, h, rev, chans, nbytes, mct=False, demote=False, org=(0, 0), what=""):
    bits, depth = chans[0]["sample_bits"], chans[0]["depth"]
    unsigned = doc.numpy_decode_output(comps, precs, rev, mct)
    planes = xim.rgba(unsigned, precs, subs, w, h, depth, bits, target, org, demote, tables=tables(target, precs[0], depth))
    want = expect(chans, nbytes, planes, w, h, demote)
    got = enc.stage_rgba_output(comps, precs, subs, w, h, rev, mct, rm.RGB, chans, doc.fill_pattern(nbytes), demote=demote, org=org,
                                xyz_to_rgb=target)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {bad.size} of {want.size} bytes differ, first at byte {bad[0]} (got {got[bad[0]]}, want {want[bad[0]]}); "
                             f"target {target} {w}x{h} precs {precs} subs {subs} org {org} rev {rev} chans {chans}")
    return planes


def xyz_comps(rng, prec, w, h, rev, ncomp=3, subs=None, org=(0, 0), anchors=True):
    """Components as the inverse DWT leaves them: around zero, a little beyond the precision's range on both sides.  The first
    pixels hold black, the top code in all three, and the three saturated primaries (top, 0, 0), (0, top, 0), (0, 0, top),
    which lie outside the Rec.709 gamut: a negative linear value, and one above the last threshold."""
    half, top = 1 << (prec - 1), (1 << prec) - 1
    subs = subs or [(1, 1)] * ncomp
    out = []
    for c, (sx, sy) in enumerate(subs):
        shape = (doc.cdiv(org[1] + h, sy), doc.cdiv(org[0] + w, sx))
        v = rng.integers(-half - 3, half + 3, size=shape)
        if anchors and c < 3:
            a = np.array([0, top, top if c == 0 else 0, top if c == 1 else 0, top if c == 2 else 0]) - half
            v.reshape(-1)[:min(5, v.size)] = a[:min(5, v.size)]
        out.append(v.astype(np.int32) if rev else (v + rng.uniform(-0.4, 0.4, size=shape)).astype(np.float32))
    return out


def forms(w, h, depth, alpha):
    """Packed records of integer samples (ARGB32 for D <= 8, ARGB64), packed ARGB128 floats, and the general strided form."""
    bits = 8 if depth <= 8 else 16
    return {"packed": frame(w, h, bits, depth, "ARGB", alpha=True),  # (the packed form needs all four channels)
            "packed float": frame(w, h, 32, depth, "ARGB", alpha=True),
            "strided": planar(w, h, bits, depth, alpha=alpha),
            "strided float": planar(w, h, 32, depth, alpha=alpha)}


# ------------------------------------------------------------------------------------------------ shapes, depths, targets, forms
@pytest.mark.parametrize("prec,depth", [(8, 8), (12, 8), (12, 16), (16, 16), (10, 10)], ids=lambda v: str(v))
@pytest.mark.parametrize("rev", [True, False], ids=["int32", "float32"])
def test_shapes_depths_targets_and_store_forms(enc, rev, prec, depth):
    rng = np.random.default_rng(prec * 100 + depth + rev)
    k = 0
    for (w, h), target in itertools.product(itertools.product((1, 255, 256, 257), (1, 2, 70)), (1, 2, 3)):
        ncomp = 3 + (k % 2)  # with and without a fourth component ...
        comps = xyz_comps(rng, prec, w, h, rev, ncomp)
        for what, form in forms(w, h, depth, alpha=k % 3 != 0).items():  # ... with and without an alpha destination
            planes = check(enc, target, comps, [prec] * ncomp, [(1, 1)] * ncomp, w, h, rev, *form, what=what)
            if ncomp == 3:  # ... whose absence fills A with the top
                assert (planes[3] == (1 << depth) - 1).all()
        k += 1


@pytest.mark.parametrize("target", [1, 2, 3])
def test_every_code_on_the_grey_axis_and_a_lattice_of_codes(enc, target):
    """Every 12-bit code in all three components at once (D65-ish greys: monotone in every channel), and a 17^3 lattice of
    codes, most of it outside the target's gamut; D = 8 and D = 16."""
    v = np.arange(4096, dtype=np.int64).reshape(16, 256)
    k = np.round(np.linspace(0, 4095, 17)).astype(np.int64)
    x, y, z = np.meshgrid(k, k, k, indexing="ij")
    for depth in (8, 16):
        comps = [(v - 2048).astype(np.int32)] * 3
        planes = check(enc, target, comps, [12] * 3, [(1, 1)] * 3, 256, 16, True, *frame(256, 16, 16 if depth == 16 else 8, depth), what="grey axis")
        assert all(np.all(np.diff(p.reshape(-1)) >= 0) and p[0, 0] == 0 for p in planes[:3])
        comps = [(c.reshape(17, 289) - 2048).astype(np.int32) for c in (x, y, z)]
        planes = check(enc, target, comps, [12] * 3, [(1, 1)] * 3, 289, 17, True, *planar(289, 17, 16 if depth == 16 else 8, depth), what="lattice")
        assert min(p.min() for p in planes[:3]) == 0 and max(p.max() for p in planes[:3]) == (1 << depth) - 1


def test_more_rows_than_the_lds_grid_has_workgroups(enc):
    """The LDS variants launch at most 2048 workgroups, each striding over its rows: at 3 columns that is 2048 rows per pass, so
    rows 2048.. are a workgroup's second.  The global-memory variant keeps a workgroup per row (up to 65535)."""
    rng = np.random.default_rng(4)
    w, h = 3, 2100
    for rev, (prec, depth) in itertools.product((True, False), ((12, 8), (12, 16))):
        comps = xyz_comps(rng, prec, w, h, rev, 3)
        check(enc, 1, comps, [prec] * 3, [(1, 1)] * 3, w, h, rev, *frame(w, h, 8 if depth == 8 else 16, depth), what="tall")
        check(enc, 2, comps, [prec] * 3, [(1, 1)] * 3, w, h, rev, *planar(w, h, 32, depth), what="tall, strided floats")


# ------------------------------------------------------------------------------------------------ demote, windows, sub-sampling
@pytest.mark.parametrize("prec", [12, 16])
def test_demote_ae16(enc, prec):
    rng = np.random.default_rng(prec)
    w, h = 70, 5
    for rev, target in itertools.product((True, False), (1, 2, 3)):
        comps = xyz_comps(rng, prec, w, h, rev, 4)
        for what, form in (("ARGB64", frame(w, h, 16, 16)), ("ARGB128", frame(w, h, 32, 16)), ("strided", planar(w, h, 16, 16)),
                           ("strided, no alpha", planar(w, h, 32, 16, alpha=False))):
            planes = check(enc, target, comps, [prec] * 4, [(1, 1)] * 4, w, h, rev, *form, demote=True, what=what)
            assert max(p.max() for p in planes) <= 32768
        planes = check(enc, target, comps[:3], [prec] * 3, [(1, 1)] * 3, w, h, rev, *frame(w, h, 16, 16), demote=True, what="filled alpha")
        assert (planes[3] == 32768).all()


@pytest.mark.parametrize("sub", [(1, 1), (2, 2), (2, 1)], ids=["444", "420", "422"])
def test_window_origins_and_subsampled_components(enc, sub):
    """A non-zero org_x / org_y in every replication phase, components 1 and 2 on a coarser grid (chroma-style), odd sizes."""
    rng = np.random.default_rng(sub[0] * 2 + sub[1])
    subs = [(1, 1), sub, sub]
    k = 0
    for (w, h), (ox, oy) in itertools.product(((37, 21), (257, 3), (1, 1)), itertools.product((0, 1, 2, 3), (0, 1, 5))):
        for prec, depth, rev in ((12, 8, True), (12, 16, False), (10, 10, k % 2 == 0)):
            target = 1 + k % 3
            comps = xyz_comps(rng, prec, w, h, rev, 3, subs, (ox, oy))
            form = (frame(w, h, 8 if depth == 8 else 16, depth), planar(w, h, 16, depth, bottom_up=True), frame(w, h, 32, depth, "RGBA", rowpad=32))[k % 3]
            check(enc, target, comps, [prec] * 3, subs, w, h, rev, *form, org=(ox, oy), what="window")
            k += 1
    # a fourth component on the full grid and of another precision: A goes through the depth conversion
    comps = xyz_comps(rng, 12, 65, 7, True, 3, subs, (3, 1)) + xyz_comps(rng, 8, 65, 7, True, 1, [(1, 1)], (3, 1), anchors=False)
    check(enc, 1, comps, [12, 12, 12, 8], subs + [(1, 1)], 65, 7, True, *frame(65, 7, 16, 16), org=(3, 1), what="alpha of another precision")


@pytest.mark.parametrize("rev", [True, False], ids=["rct", "ict"])
def test_component_transform_in_front_of_the_conversion(enc, rev):
    rng = np.random.default_rng(3 + rev)
    for prec, depth, target in ((12, 8, 1), (12, 16, 2), (16, 16, 3)):
        comps = xyz_comps(rng, prec, 131, 9, rev, 4, anchors=False)
        check(enc, target, comps, [prec] * 4, [(1, 1)] * 4, 131, 9, rev, *frame(131, 9, 8 if depth == 8 else 16, depth), mct=True, what="mct")


def test_destination_variants(enc):
    rng = np.random.default_rng(8)
    w, h = 70, 5
    comps = xyz_comps(rng, 12, w, h, True, 4)
    for bits, depth in ((8, 8), (16, 12), (16, 16), (32, 12)):
        variants = {"RGBA": frame(w, h, bits, depth, "RGBA"), "BGRA": frame(w, h, bits, depth, "BGRA"),
                    "padded rows": frame(w, h, bits, depth, "ARGB", rowpad=4 * (bits // 8) * 3),
                    "no alpha destination": frame(w, h, bits, depth, "ARGB", alpha=False),
                    "bottom-up planes": planar(w, h, bits, depth, bottom_up=True)}
        narrow = frame(w, h, bits, depth)
        for c in narrow[0]:
            c["width"], c["height"] = w - 7, h - 2
        variants["narrower and shorter"] = narrow
        for what, form in variants.items():
            check(enc, 1, comps, [12] * 4, [(1, 1)] * 4, w, h, True, *form, what=what)


# ------------------------------------------------------------------------------------------------ off, and the refusals
def test_value_0_is_the_plain_stage(enc):
    rng = np.random.default_rng(1)
    w, h = 67, 4
    comps = xyz_comps(rng, 12, w, h, True, 4)
    chans, n = frame(w, h, 16, 16)
    args = (comps, [12] * 4, [(1, 1)] * 4, w, h, True, False, rm.RGB, chans, doc.fill_pattern(n))
    plain = enc.stage_rgba_output(*args)
    assert np.array_equal(enc.stage_rgba_output(*args, xyz_to_rgb=0), plain)
    assert not np.array_equal(enc.stage_rgba_output(*args, xyz_to_rgb=1), plain)
    for mode, cs in ((rm.GREY, comps[:2]), (rm.SYCC, comps[:3])):  # 0 leaves the other modes alone too
        a = (cs, [12] * len(cs), [(1, 1)] * len(cs), w, h, True, False, mode, chans, doc.fill_pattern(n))
        assert np.array_equal(enc.stage_rgba_output(*a, xyz_to_rgb=0), enc.stage_rgba_output(*a))


def test_refusals_name_the_setting(enc):
    rng = np.random.default_rng(2)
    w, h = 20, 3
    comps = xyz_comps(rng, 12, w, h, True, 3)
    chans, n = frame(w, h, 16, 16)

    def refused(cs, precs, mode, value, **kw):
        with pytest.raises(api.J2kHipError) as ei:
            enc.stage_rgba_output(cs, precs, [(1, 1)] * len(cs), w, h, True, False, mode, chans, doc.fill_pattern(n), xyz_to_rgb=value, **kw)
        assert ei.value.code == J2K_HIP_ERR_PARAM and "xyz_to_rgb" in str(ei.value), str(ei.value)

    refused(comps, [12] * 3, rm.RGB, 4)
    refused(comps[:1], [12], rm.GREY, 1)
    refused(comps[:2], [12] * 2, rm.GREY, 2)
    refused(comps, [12] * 3, rm.SYCC, 1)
    refused(comps[:1], [8], rm.PALETTE, 3, lut=np.zeros((4, 3), np.uint8))
    refused(comps, [12, 12, 10], rm.RGB, 1)
    refused(comps, [12, 10, 12], rm.RGB, 1)
    check(enc, 1, comps, [12] * 3, [(1, 1)] * 3, w, h, True, chans, n, what="and the handle still works")
