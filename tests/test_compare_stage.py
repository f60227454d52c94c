"""GPU: the compare's reduction kernel alone (j2k_hip_stage_compare, j2k_amd/csrc/compare.hip): source planes against decoded
planes that the test makes up.  Every expectation is the numpy model of the definition (compare_model.py); every integer
field is compared exactly, mse and psnr to the last bit of the header's double formulas."""
import math

import numpy as np
import pytest

import compare_model as cm

pytestmark = pytest.mark.gpu

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


def _interleaved(chans, dtype, row_pad=0):
    """[R, G, B, A] planes -> (buffer, layout) of an A,R,G,B interleaved frame of `dtype` samples (ARGB32 / ARGB64 / ARGB128)."""
    sb = np.dtype(dtype).itemsize
    h, w = chans[0].shape
    rowbytes = 4 * sb * w + row_pad
    buf = np.full(h * rowbytes, 0xff, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(buf.view(dtype), shape=(h, w, 4), strides=(rowbytes, 4 * sb, sb), writeable=True)
    for slot, c in zip((1, 2, 3, 0), chans):
        view[:, :, slot] = np.asarray(c).astype(dtype)
    return buf, dict(sample_bytes=sb, colbytes=4 * sb, rowbytes=rowbytes, channel_offsets=(0, sb, 2 * sb, 3 * sb))


def _noisy(rng, s, depth, density=0.3):
    """Decoded planes: the source with errors of every size on some of its samples, clipped to the depth."""
    top = (1 << depth) - 1
    e = rng.integers(-top, top + 1, size=s.shape) * (rng.random(s.shape) < density)
    small = rng.integers(-2, 3, size=s.shape) * (rng.random(s.shape) < density)
    return np.clip(np.asarray(s).astype(np.int64) + e + small, 0, top)


def _same(got, want):
    assert len(got) == len(want)
    for c, (g, w) in enumerate(zip(got, want)):
        assert g == w, (c, g, w)  # (dict equality: the integers exactly, the doubles bit for bit -- inf == inf, no NaN occurs)


# (260: rows that four-sample loads read whole; 1030: past one workgroup's 1024 samples of a row)
SHAPES = [(1, 1), (7, 1), (1, 63), (65, 3), (130, 5), (257, 9), (260, 3), (1030, 2)]


@pytest.mark.parametrize("size", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_across_lane_wave_and_workgroup_edges(api, enc, size):
    w, h = size
    rng = np.random.default_rng(w * 1000 + h)
    # dense 8-bit planes (four samples per load where a row allows), three components
    src = rng.integers(0, 256, size=(3, h, w))
    dec = [_noisy(rng, src[c], 8) for c in range(3)]
    p = api.make_params(w, h, 3, 8)
    _same(enc.stage_compare(dec, p, planar=src), cm.diffs(list(src), dec, 8))
    # an ARGB64 frame with padded rows (a pixel per load), four components of 16 bits
    src = rng.integers(0, 65536, size=(4, h, w))
    dec = [_noisy(rng, src[c], 16) for c in range(4)]
    buf, lay = _interleaved(list(src), np.uint16, row_pad=8)
    p = api.make_params(w, h, 4, 16)
    _same(enc.stage_compare(dec, p, frame=buf, layout=lay), cm.diffs(list(src), dec, 16))
    # dense 16-bit planes of one component
    p = api.make_params(w, h, 1, 16)
    _same(enc.stage_compare(dec[:1], p, planar=src[:1]), cm.diffs([src[0]], dec[:1], 16))
    # dense planes whose rows are padded to a multiple of four samples: four samples per load, the row's ragged end one by one
    for dtype, d in ((np.uint8, 8), (np.uint16, 16)):
        store = rng.integers(0, 1 << d, size=(2, h, (w + 3) // 4 * 4 + 4)).astype(dtype)
        views = [store[c, :, :w] for c in range(2)]
        s = [v.astype(np.int64) for v in views]
        dec2 = [_noisy(rng, c, d) for c in s]
        make = lambda dev: api.planes_from_arrays(views, d, base_of=lambda c: dev + (views[c].ctypes.data - store.ctypes.data))
        _same(enc.stage_compare(dec2, api.make_params(w, h, 2, d), views=(store.reshape(-1).view(np.uint8), make)), cm.diffs(s, dec2, d))


def test_sums_beyond_32_bits(api, enc):
    """Source 0, decoded 65535 everywhere: sum_sq = 90000 * 65535^2 does not fit 32 bits, nor does sum_abs."""
    src = np.zeros((1, 300, 300), np.int64)
    dec = [np.full((300, 300), 65535)]
    got = enc.stage_compare(dec, api.make_params(300, 300, 1, 16), planar=src)
    assert got[0]["sum_sq"] == 90000 * 65535 ** 2 and got[0]["sum_abs"] == 90000 * 65535 and got[0]["differing"] == 90000
    assert got[0]["max_abs"] == 65535 and (got[0]["first_x"], got[0]["first_y"]) == (0, 0) and got[0]["psnr"] == 0.0
    _same(got, cm.diffs(list(src), dec, 16))


@pytest.mark.parametrize("size", [(257, 9), (1030, 5)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_and_two_differing_samples(api, enc, size):
    w, h = size
    rng = np.random.default_rng(5)
    src = rng.integers(0, 4096, size=(1, h, w))
    p = api.make_params(w, h, 1, 12)
    for x, y in ((0, 0), (w - 1, h - 1), (w // 2, h - 1), (0, h - 1), (w - 1, 0)):
        dec = src[0].copy()
        dec[y, x] ^= 0x155
        got = enc.stage_compare([dec], p, planar=src)
        assert (got[0]["differing"], got[0]["first_x"], got[0]["first_y"]) == (1, x, y)
        assert got[0]["max_abs"] == abs(int(dec[y, x]) - int(src[0, y, x])) == got[0]["sum_abs"]
        _same(got, cm.diffs(list(src), [dec], 12))
    # two: the first in raster order is reported, whichever lane, wave or workgroup meets it
    for a, b in (((w - 1, 2), (0, 3)), ((5, 4), (w - 2, 4)), ((w // 2, 0), (w // 2 - 1, h - 1)), ((3, 1), (2, 1))):
        dec = src[0].copy()
        dec[a[1], a[0]] ^= 1
        dec[b[1], b[0]] ^= 0x800
        got = enc.stage_compare([dec], p, planar=src)
        first = min(a, b, key=lambda q: (q[1], q[0]))
        assert (got[0]["differing"], got[0]["first_x"], got[0]["first_y"], got[0]["max_abs"]) == (2, first[0], first[1], 0x800)
        _same(got, cm.diffs(list(src), [dec], 12))


def test_identical_planes(api, enc):
    rng = np.random.default_rng(6)
    src = rng.integers(0, 1024, size=(3, 9, 130))
    got = enc.stage_compare(list(src), api.make_params(130, 9, 3, 10), planar=src)
    for c in range(3):
        assert got[c] == dict(samples=130 * 9, differing=0, sum_abs=0, sum_sq=0, max_abs=0, first_x=0, first_y=0, mse=0.0, psnr=math.inf)


W, H = 17, 9


def _float_world(rng, d):
    x = rng.uniform(-0.05, 1.05, size=(4, H, W)).astype(F32)
    x[0, 0, :6] = np.array([np.nan, np.inf, -np.inf, -0.0, 1.0, 0.5], F32)
    grid = rng.integers(0, 1 << d, size=(H, W))
    x[3] = (grid.astype(F32) / F32((1 << d) - 1)).astype(F32)
    return x


@pytest.mark.parametrize("promote", [False, True], ids=["plain", "promote"])
def test_interleaved_source_forms(api, enc, promote):
    """ARGB32, ARGB64 and ARGB128 pixels, three and four components, with promote_ae16 off and on (it acts on 16-bit samples
    and on floats of depth 16 only)."""
    rng = np.random.default_rng(7 + promote)
    for dtype, d, prec in ((np.uint8, 8, 8), (np.uint16, 16, 16), (np.uint16, 16, 12), (np.float32, 16, 16), (np.float32, 16, 10)) + \
                          (() if promote else ((np.float32, 8, 8), (np.float32, 10, 12))):
        if dtype == np.float32:
            chans = list(_float_world(rng, d))
        else:
            chans = list(rng.integers(0, (32769 if promote and d == 16 else 1 << d), size=(4, H, W)))
        buf, lay = _interleaved(chans, dtype, row_pad=(16 if dtype == np.float32 else 8))
        lay["depth"] = d
        stored = [np.asarray(c).astype(dtype) for c in chans]
        for nc in (3, 4):
            s = cm.source_components(stored[:nc], [d] * nc, prec, promote)
            dec = [_noisy(rng, c, prec) for c in s]
            p = api.make_params(W, H, nc, prec, promote=promote)
            _same(enc.stage_compare(dec, p, frame=buf, layout=lay), cm.diffs(s, dec, prec))


def _strided_views(api, arrays, depths):
    """Channel views over 2-D arrays that are slices of bigger stores (colbytes > sample size, padded rows)."""
    def planes(store, views):
        def make(dev):
            arr = api.planes_from_arrays(views, 0, base_of=lambda c: dev + (views[c].ctypes.data - store.ctypes.data))
            for c, d in enumerate(depths):
                arr[c].depth = d
            return arr
        return make
    return planes


def test_strided_channels_and_depth_conversions(api, enc):
    rng = np.random.default_rng(8)
    # 8- and 16-bit channels, every third / second sample of a row (colbytes > sample size), depth conversions 8 -> 12, 16 -> 10, 5 -> 16
    for dtype, step, d, prec in ((np.uint8, 3, 8, 12), (np.uint16, 2, 16, 10), (np.uint8, 2, 5, 16), (np.uint16, 3, 12, 12)):
        store = rng.integers(0, 1 << d, size=(3, H, W * step + 1)).astype(dtype)
        views = [store[c, :, 1::step][:, :W] for c in range(3)]
        assert views[0].strides[1] == step * store.itemsize
        s = cm.source_components(views, [d] * 3, prec)
        dec = [_noisy(rng, c, prec) for c in s]
        p = api.make_params(W, H, 3, prec)
        make = _strided_views(api, views, [d] * 3)(store, views)
        _same(enc.stage_compare(dec, p, views=(store.reshape(-1).view(np.uint8), make)), cm.diffs(s, dec, prec))


def test_mixed_float_and_integer_channels(api, enc):
    """A float channel of depth 10, a 16-bit integer channel, an 8-bit one and a float of depth 16 in one call (one buffer)."""
    rng = np.random.default_rng(9)
    prec = 12
    f10, f16 = _float_world(rng, 10)[0], _float_world(rng, 16)[3]
    u16, u8 = rng.integers(0, 65536, size=(H, W)).astype(np.uint16), rng.integers(0, 256, size=(H, W)).astype(np.uint8)
    parts = [f10, u16, u8, f16]
    depths = [10, 16, 8, 16]
    offs, pos = [], 0
    for a in parts:
        offs.append(pos)
        pos += -(-a.nbytes // 16) * 16
    buf = np.zeros(pos, np.uint8)
    for a, o in zip(parts, offs):
        buf[o:o + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)

    def make(dev):
        arr = api.planes_from_arrays(parts, 0, base_of=lambda c: dev + offs[c])
        for c, d in enumerate(depths):
            arr[c].depth = d
        return arr
    s = cm.source_components(parts, depths, prec)
    dec = [_noisy(rng, c, prec) for c in s]
    _same(enc.stage_compare(dec, api.make_params(W, H, 4, prec), views=(buf, make)), cm.diffs(s, dec, prec))


def test_four_components_with_only_the_alpha_differing(api, enc):
    rng = np.random.default_rng(10)
    src = rng.integers(0, 256, size=(4, H, W))
    dec = [src[c].copy() for c in range(4)]
    dec[3] = _noisy(rng, src[3], 8)
    buf, lay = _interleaved(list(src), np.uint8)
    got = enc.stage_compare(dec, api.make_params(W, H, 4, 8), frame=buf, layout=lay)
    assert [g["differing"] for g in got[:3]] == [0, 0, 0] and got[3]["differing"] > 0
    _same(got, cm.diffs(list(src), dec, 8))


@pytest.mark.parametrize("sub", [(2, 1), (2, 2)], ids=["422", "420"])
def test_rgb_to_sycc(api, enc, sub):
    """R, G, B[, A] of the full image; Y, Cb, Cr[, A] are compared, the chroma on its decimated grid."""
    rng = np.random.default_rng(11)
    for dtype, d, prec, nc in ((np.uint8, 8, 8, 3), (np.uint16, 16, 12, 4), (np.uint8, 8, 8, 4)):
        src = rng.integers(0, 1 << d, size=(4, H, W))
        src[:3, :2, :] = (1 << d) - 1  # (saturated rows: the chroma clamp)
        buf, lay = _interleaved(list(src), dtype, row_pad=8)
        stored = [src[c].astype(dtype) for c in range(nc)]
        s = cm.source_components(stored, [d] * nc, prec, rgb_to_sycc=sub)
        assert s[1].shape == (-(-H // sub[1]), -(-W // sub[0])) and s[0].shape == (H, W)
        dec = [_noisy(rng, c, prec) for c in s]
        p = api.make_params(W, H, nc, prec, sub=[(1, 1), sub, sub] + [(1, 1)] * (nc - 3), rgb_to_sycc=True)
        _same(enc.stage_compare(dec, p, frame=buf, layout=lay), cm.diffs(s, dec, prec))
        same = enc.stage_compare(s, p, frame=buf, layout=lay)
        assert [g["differing"] for g in same] == [0] * nc


@pytest.mark.parametrize("sub", [(2, 2), (4, 1)], ids=["2x2", "4x1"])
def test_comp_sub_planes(api, enc, sub):
    """Components given as planes of their own sizes: 33 x 17, components 1 and 2 sub-sampled."""
    w, h = 33, 17
    rng = np.random.default_rng(12)
    subs = [(1, 1), sub, sub]
    for prec in (8, 12):
        comps = [rng.integers(0, 1 << prec, size=(-(-h // sy), -(-w // sx))) for sx, sy in subs]
        dec = [_noisy(rng, c, prec) for c in comps]
        p = api.make_params(w, h, 3, prec, sub=subs)
        _same(enc.stage_compare(dec, p, comps=comps), cm.diffs(comps, dec, prec))
