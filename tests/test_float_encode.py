"""GPU: encoding from 32-bit float samples (After Effects 32-bpc worlds, sample_bits 32).

The front end against the numpy model of the definition (float_model.py) word for word; whole files against the committed
libopenjp2 goldens byte for byte, the float frame built from the integers the 16-bit frame of the same golden holds
(test_float_model.py shows that the definition returns them); every entry point; what is refused."""
import ctypes as C

import numpy as np
import pytest

import float_model as fm
import rgba_model
import subsample_cases as sub_cases
import sycc_model
from conftest import golden_case
from j2k_amd import synth

pytestmark = pytest.mark.gpu

J2K_HIP_ERR_PARAM = 1
F32 = np.float32


@pytest.fixture(scope="module")
def api():
    from j2k_amd import api
    return api


@pytest.fixture(scope="module")
def enc(api):
    e = api.Encoder(0)
    yield e
    e.close()


def _argb128(chans, row_pad=0):
    """[R, G, B, A] float32 planes -> (buffer, layout) of an ARGB128 frame; the padding holds NaN patterns."""
    h, w = chans[0].shape
    rowbytes = 16 * w + row_pad
    buf = np.full(h * rowbytes, 0xff, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(buf.view(F32), shape=(h, w, 4), strides=(rowbytes, 16, 4), writeable=True)
    for slot, c in zip((1, 2, 3, 0), chans):
        view[:, :, slot] = c
    return buf, dict(sample_bytes=4, colbytes=16, rowbytes=rowbytes, channel_offsets=(0, 4, 8, 12), depth=16)


def _argb64(chans, row_pad=0):
    """[R, G, B, A] integer planes (16-bit values) -> (buffer, layout) of an ARGB64 frame."""
    h, w = chans[0].shape
    rowbytes = 8 * w + row_pad
    buf = np.zeros(h * rowbytes, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(buf.view(np.uint16), shape=(h, w, 4), strides=(rowbytes, 8, 2), writeable=True)
    for slot, c in zip((1, 2, 3, 0), chans):
        view[:, :, slot] = np.asarray(c).astype(np.uint16)
    return buf, dict(sample_bytes=2, colbytes=8, rowbytes=rowbytes, channel_offsets=(0, 2, 4, 6))


SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, 5e-39, 1.0, 1.0000001, 2.0, -1e-30, 0.5, 0.49999997, 3e38], dtype=F32)


def _floats(rng, shape):
    """Off-grid floats around 0..1 with the special values sprinkled in."""
    x = rng.uniform(-0.05, 1.05, size=shape).astype(F32)
    flat = x.reshape(-1)
    idx = rng.permutation(flat.size)[:min(flat.size, SPECIALS.size)]
    flat[idx] = SPECIALS[:idx.size]
    return x


def _frontend_model(oracle, ints, prec, rev, mct):
    """Integer samples of depth `prec` -> the front end's words (DC shift + RCT / ICT by the oracle), as uint32."""
    ref = np.ascontiguousarray(np.stack(ints).astype(np.int32))
    nc = ref.shape[0]
    ptrs = (C.POINTER(C.c_int32) * nc)(*[ref[c].ctypes.data_as(C.POINTER(C.c_int32)) for c in range(nc)])
    oracle.L.j2ko_dc_mct.argtypes = [C.POINTER(C.POINTER(C.c_int32)), C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int]
    oracle.L.j2ko_dc_mct(ptrs, nc, ref[0].size, prec, int(rev), int(mct))
    return ref.view(np.uint32)


def _model_ints(x, d, prec, promote):
    return rgba_model.depth_convert(fm.quantise(x, d, promote), d, prec, 32)


#       d  prec promote
FORMS = [(16, 16, False), (16, 12, False), (8, 8, False), (8, 12, False), (16, 16, True), (10, 10, False)]


@pytest.mark.parametrize("size", [(1, 1), (3, 5), (67, 9)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("rev", [True, False], ids=["53", "97"])
@pytest.mark.parametrize("mct", [False, True], ids=["plain", "mct"])
def test_frontend_equals_the_model(api, enc, oracle, size, rev, mct):
    """ARGB128 frames (one 16-byte load per pixel; padded rows) and planar float arrays with padded rows."""
    w, h = size
    for k, (d, prec, promote) in enumerate(FORMS):
        for nc in (3, 4):
            rng = np.random.default_rng(100 * k + nc + w)
            x = _floats(rng, (4, h, w))
            p = api.make_params(w, h, nc, prec, reversible=rev, ycc=mct, promote=promote, num_resolutions=1)
            want = _frontend_model(oracle, [_model_ints(x[c], d, prec, promote) for c in range(nc)], prec, rev, mct)
            # interleaved
            buf, lay = _argb128(list(x), row_pad=16 * (k % 2))
            lay["depth"] = d
            got = enc.stage_frontend(buf, lay, p)
            assert np.array_equal(got.view(np.uint32), want), ("argb128", d, prec, promote, nc)
            # an ARGB128 frame whose rows are no multiple of the pixel: the strided 4-byte loads
            buf, lay = _argb128(list(x), row_pad=4)
            lay["depth"] = d
            got = enc.stage_frontend(buf, lay, p)
            assert np.array_equal(got.view(np.uint32), want), ("argb128 odd rows", d, prec, promote, nc)
            # planar, padded rows
            store = np.full((nc, h, w + 3), np.nan, dtype=F32)
            store[:, :, :w] = x[:nc]
            views = [store[c, :, :w] for c in range(nc)]
            planes = lambda dev: api.planes_from_arrays(views, d, base_of=lambda c: dev + (views[c].ctypes.data - store.ctypes.data))
            got = enc.stage_frontend_planes(store, planes, p)
            assert np.array_equal(np.asarray(got).view(np.uint32), want), ("planar", d, prec, promote, nc)


def _neighbourhood(d, promote):
    """Every grid point of the form, its float32 neighbours, and the midpoints to the next grid point with theirs."""
    scale = F32(32768) if promote else F32((1 << d) - 1)
    n = 32769 if promote else (1 << d)
    k = np.arange(n, dtype=np.int64)
    grid = (k.astype(F32) / scale).astype(F32)
    mid = ((k.astype(np.float64) + 0.5) / float(scale)).astype(F32)
    out = []
    for v in (grid, mid):
        out += [v, np.nextafter(v, F32(-1)), np.nextafter(v, F32(2))]
    return out


@pytest.mark.parametrize("form", [(16, False), (8, False), (16, True)], ids=["d16", "d8", "promote"])
def test_frontend_every_grid_point_and_midpoint(api, enc, oracle, form):
    d, promote = form
    six = _neighbourhood(d, promote)
    w = h = 256
    tiles = [np.resize(v, w * h).reshape(h, w) for v in six]
    p4 = api.make_params(w, h, 4, d, reversible=True, promote=promote, num_resolutions=1)
    p3 = api.make_params(w, h, 3, d, reversible=True, promote=promote, num_resolutions=1)
    # A, R, G, B of one ARGB128 frame: grid, grid - ulp, grid + ulp, midpoint (channels R, G, B, A = 1, 2, 3, 0)
    chans = [tiles[1], tiles[2], tiles[3], tiles[0]]
    buf, lay = _argb128(chans)
    lay["depth"] = d
    want = _frontend_model(oracle, [fm.quantise(c, d, promote) for c in chans], d, True, False)
    assert np.array_equal(enc.stage_frontend(buf, lay, p4).view(np.uint32), want)
    # planar: midpoint, midpoint - ulp, midpoint + ulp
    store = np.ascontiguousarray(np.stack(tiles[3:6]))
    views = [store[c] for c in range(3)]
    planes = lambda dev: api.planes_from_arrays(views, d, base_of=lambda c: dev + (views[c].ctypes.data - store.ctypes.data))
    want = _frontend_model(oracle, [fm.quantise(c, d, promote) for c in views], d, True, False)
    assert np.array_equal(np.asarray(enc.stage_frontend_planes(store, planes, p3)).view(np.uint32), want)
    # and the grid points come back as themselves
    n = 32769 if promote else (1 << d)
    back = fm.quantise(six[0], d, promote)
    assert np.array_equal(back, fm.promote16(np.arange(n)) if promote else np.arange(n))


@pytest.mark.parametrize("rev", [True, False], ids=["53", "97"])
def test_frontend_mixed_float_and_16_bit_channels(api, enc, oracle, rev):
    w, h = 67, 9
    rng = np.random.default_rng(5)
    xf = _floats(rng, (2, h, w))
    xi = rng.integers(0, 65536, size=(2, h, w)).astype(np.uint16)
    # one buffer: float plane, 16-bit plane, float plane, 16-bit plane (each 16-byte aligned)
    fb, ib = xf[0].nbytes, -(-xi[0].nbytes // 16) * 16
    store = np.zeros(2 * fb + 2 * ib, np.uint8)
    offs = [0, fb, fb + ib, 2 * fb + ib]
    views = [store[offs[0]:offs[0] + fb].view(F32).reshape(h, w), store[offs[1]:offs[1] + xi[0].nbytes].view(np.uint16).reshape(h, w),
             store[offs[2]:offs[2] + fb].view(F32).reshape(h, w), store[offs[3]:offs[3] + xi[1].nbytes].view(np.uint16).reshape(h, w)]
    views[0][...], views[1][...], views[2][...], views[3][...] = xf[0], xi[0], xf[1], xi[1]
    for prec, mct in ((16, True), (12, False)):
        p = api.make_params(w, h, 4, prec, reversible=rev, ycc=mct, num_resolutions=1)
        planes = lambda dev: api.planes_from_arrays(views, 16, base_of=lambda c: dev + offs[c])
        ints = [_model_ints(xf[0], 16, prec, False), rgba_model.depth_convert(xi[0], 16, prec, 32),
                _model_ints(xf[1], 16, prec, False), rgba_model.depth_convert(xi[1], 16, prec, 32)]
        want = _frontend_model(oracle, ints, prec, rev, mct)
        assert np.array_equal(np.asarray(enc.stage_frontend_planes(store, planes, p)).view(np.uint32), want)


@pytest.mark.parametrize("size", [(5, 3), (66, 34)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_ycc_front_end_420_equals_the_model(api, enc, size):
    w, h = size
    sub = (2, 2)
    for k, (d, prec, nc, rev, promote) in enumerate([(16, 16, 3, True, False), (16, 12, 4, False, False), (8, 8, 4, True, False), (16, 16, 4, False, True)]):
        x = _floats(np.random.default_rng(31 * k + w), (4, h, w))
        buf, lay = _argb128(list(x), row_pad=16 * (k % 2))
        lay["depth"] = d
        p = api.make_params(w, h, nc, prec, reversible=rev, promote=promote, num_resolutions=1,
                            sub=[(1, 1), sub, sub] + [(1, 1)] * (nc - 3), rgb_to_sycc=True)
        got = enc.stage_frontend(buf, lay, p)
        want = sycc_model.frontend_planes([_model_ints(x[c], d, prec, promote) for c in range(nc)], prec, sub)
        assert len(got) == nc
        for c in range(nc):
            g, wnt = np.asarray(got[c]), np.asarray(want[c])
            assert g.shape == wnt.shape
            assert np.array_equal(g, wnt) if rev else np.array_equal(g.view(np.uint32), wnt.astype(F32).view(np.uint32)), (k, c)


# ------------------------------------------------------------------------------------------------ bytes
def _params_from_golden(api, g, **kw):
    q = g["params"]
    return api.make_params(g["width"], g["height"], g["ncomp"], g["prec"], reversible=q.get("reversible", True),
                           ycc=q.get("mct", False), layers=q.get("layers", 1), tile_size=q.get("tile", 0),
                           num_resolutions=q.get("numres", 6), cblk=tuple(q.get("cblk", (64, 64))), comment="", **kw)


GOLDENS = ["g4_300x200_rgb16_53_rct_tile128", "g6_300x200_rgb16_97_ict", "g7_300x200_rgb10_53", "g9_300x200_rgba8_53_rct"]


def _float_frame_of_golden(g, pl, row_pad=16):
    """The floats of the integers synth.ae_frame stores for the golden: 8-bit worlds as depth 8, deeper ones left-justified
    to 16 bits."""
    d = 8 if g["prec"] <= 8 else 16
    return synth.ae_frame_float(pl, d, row_pad_bytes=row_pad, prec=g["prec"])


@pytest.mark.parametrize("name", GOLDENS)
def test_float_frame_encodes_to_the_golden(api, enc, golden, name):
    g, pl, _, cs = golden_case(golden, name)
    frame, lay = _float_frame_of_golden(g, pl)
    p = _params_from_golden(api, g)
    ours = enc.encode_host(frame, lay, p)
    assert len(ours) == g["length"]
    assert ours == cs
    assert enc.stats()["bands"] == 0


def test_promoted_float_frame_encodes_to_the_golden(api, enc, golden):
    """The 15+1-bit world as floats (Demote(sample) / 32768) under promote_ae16.  Promote(Demote(s)) = s needs an s that Promote
    produces: the golden's samples are brought there first, and the reference bytes come from the 16-bit frame of those."""
    g, pl, _, _ = golden_case(golden, "g6_300x200_rgb16_97_ict")
    pl = fm.promote16(fm.demote16(pl)).astype(np.int32)
    frame, lay = synth.ae_frame_float(pl, 16, row_pad_bytes=16, promote=True)
    iframe, ilay = synth.ae_frame(pl, 16)
    assert enc.encode_host(frame, lay, _params_from_golden(api, g, promote=True)) == enc.encode_host(iframe, ilay, _params_from_golden(api, g))


def test_float_components_encode_to_the_subsampled_golden(api, enc):
    name = sub_cases.by_prefix("q2")  # 97 x 61, 4:2:0, 10 bits, 9/7, 4 resolutions
    g = sub_cases.entry(name)
    p = sub_cases.params(api, name)
    comps = sub_cases.components(name)
    bufs = [np.ascontiguousarray(fm.to_float(c, g["prec"])) for c in comps]
    planes = api.planes_from_arrays(bufs, g["prec"])
    ours = sub_cases.strip_com(enc._encode_planes_host(planes, sum(b.nbytes for b in bufs), p, False))
    assert ours == sub_cases.golden_bytes(name)
    assert enc.stats()["bands"] == 0


def test_every_entry_point_writes_the_golden(api, enc, golden):
    L = enc.L
    g, pl, _, cs = golden_case(golden, "g4_300x200_rgb16_53_rct_tile128")
    frame, lay = _float_frame_of_golden(g, pl)
    pl2 = synth.planes(g["width"], g["height"], g["ncomp"], g["prec"], g["seed"] + 1, g["dist"])
    frame2, _ = _float_frame_of_golden(g, pl2)
    iframe2, ilay = synth.ae_frame(pl2, g["prec"])
    p = _params_from_golden(api, g)
    other = enc.encode_host(iframe2, ilay, p)
    assert other != cs
    assert enc.encode_host(frame, lay, p, via_sink=True) == cs
    enc.encode_begin_host(frame, lay, p)
    assert enc.encode_end() == cs
    enc.encode_begin_borrowed(frame, lay, p)
    assert enc.encode_end() == cs
    d, d2 = enc.upload(frame), enc.upload(frame2)
    try:
        assert enc.encode_device(d, lay, p)[2] == cs
        assert [r[2] for r in enc.encode_sequence_device([d, d2], lay, p)] == [cs, other]
        parts = [enc.encode_tiles_device(d, lay, p, a, b) for (a, b) in [(0, 1), (1, 3), (4, 2)]]
        assert api.main_header(p) + b"".join(parts) + b"\xff\xd9" == cs
    finally:
        enc.free(d)
        enc.free(d2)
    # host tiles
    nc = p.channels
    planes = api.planes_from_layout(frame.ctypes.data, lay, nc)
    out, n = np.empty(1 << 20, np.uint8), C.c_size_t()
    enc._check(L.j2k_hip_encode_tiles(enc.h, C.byref(p), planes, 0, 6, out.ctypes.data, out.nbytes, C.byref(n)))
    assert api.main_header(p) + out[:n.value].tobytes() + b"\xff\xd9" == cs
    # the batch: two frames on two handles of one device
    planes2 = api.planes_from_layout(frame2.ctypes.data, lay, nc)
    both = (api.Plane * (2 * nc))(*(list(planes) + list(planes2)))
    chunks = [[], []]
    ids = (C.c_void_p * 2)(1, 2)

    @api.WRITE_FN
    def write(user, buf, nbytes):
        chunks[user - 1].append(C.string_at(buf, nbytes))
        return nbytes
    devs = (C.c_int * 2)(0, 0)
    assert L.j2k_hip_encode_batch(devs, 2, 1, C.byref(p), both, 2, write, ids) == 0, L.j2k_hip_multi_last_error()
    assert [b"".join(c) for c in chunks] == [cs, other]
    # layer_rates: the allocation sees the same coefficients, so the same file as from the 16-bit frame
    iframe, _ = synth.ae_frame(pl, g["prec"])
    pr = _params_from_golden(api, g, rates=[40.0, 10.0])
    assert enc.encode_host(frame, lay, pr) == enc.encode_host(iframe, ilay, pr)
    # rgb_to_sycc at 4:2:0 from the float world: the file of the 16-bit world
    ps = api.make_params(g["width"], g["height"], 3, g["prec"], num_resolutions=4, sub=[(1, 1), (2, 2), (2, 2)], rgb_to_sycc=True)
    assert enc.encode_host(frame, lay, ps) == enc.encode_host(iframe, ilay, ps)


@pytest.mark.parametrize("rev", [True, False], ids=["53", "97"])
def test_off_grid_floats_encode_as_the_model_s_16_bit_frame(api, enc, rev):
    w, h = 150, 70
    x = _floats(np.random.default_rng(9), (4, h, w))
    buf, lay = _argb128(list(x), row_pad=16)
    ibuf, ilay = _argb64([fm.quantise(c, 16) for c in x])
    for nc, prec in ((4, 16), (3, 12)):
        p = api.make_params(w, h, nc, prec, reversible=rev, ycc=True, num_resolutions=4)
        assert enc.encode_host(buf, lay, p) == enc.encode_host(ibuf, ilay, p)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing(api, enc):
    w, h = 16, 8
    frame, lay = synth.ae_frame_float(synth.planes(w, h, 3, 16, 1), 16)
    out = np.full(1 << 16, 0x5a, np.uint8)

    def refused(p, planes):
        n = C.c_size_t(12345)
        rc = enc.L.j2k_hip_encode_to_buffer(enc.h, C.byref(p), planes, out.ctypes.data, out.nbytes, C.byref(n))
        assert rc == J2K_HIP_ERR_PARAM, rc
        text = enc.L.j2k_hip_last_error(enc.h)
        assert np.all(out == 0x5a)
        d = enc.upload(frame)
        try:
            dptr, dn = C.c_void_p(), C.c_size_t()
            dplanes = api.planes_from_layout(d, lay, 3)
            for c in range(3):
                dplanes[c].depth, dplanes[c].rowbytes = planes[c].depth, planes[c].rowbytes
            assert enc.L.j2k_hip_encode_device(enc.h, C.byref(p), dplanes, C.byref(dptr), C.byref(dn), None, 0) == J2K_HIP_ERR_PARAM
        finally:
            enc.free(d)
        return text

    p = api.make_params(w, h, 3, 16, num_resolutions=2)
    for depth in (17, 0):
        refused(p, api.planes_from_layout(frame.ctypes.data, lay, 3, depth_bits=depth))
    bad = api.planes_from_layout(frame.ctypes.data, lay, 3)
    for c in range(3):
        bad[c].rowbytes = lay["rowbytes"] + 2
    assert b"multiples of 4" in refused(p, bad)
    refused(api.make_params(w, h, 3, 16, num_resolutions=2, promote=True), api.planes_from_layout(frame.ctypes.data, lay, 3, depth_bits=12))
    # and the handle is as usable as before
    assert len(enc.encode_host(frame, lay, p)) > 0


def test_forced_bands_do_not_take_a_float_frame(api, enc, golden):
    g, pl, _, cs = golden_case(golden, "g4_300x200_rgb16_53_rct_tile128")
    frame, lay = _float_frame_of_golden(g, pl, row_pad=0)
    p = _params_from_golden(api, g)
    api.tune("bands", 3)
    try:
        assert enc.encode_host(frame, lay, p) == cs
        assert enc.stats()["bands"] == 0
        assert enc.encode_host(frame, lay, p, via_sink=True) == cs
        assert enc.stats()["bands"] == 0
    finally:
        api.tune("bands", 0)
