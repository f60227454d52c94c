"""GPU: writing sub-sampled components (4:2:2, 4:2:0 and other factors of 1, 2, 4) -- from component planes given at their
own sizes, byte for byte what libopenjp2 writes (tests/golden/subsample/), and from R, G, B[, A] through the Y Cb Cr front-end
kernel, sample for sample what the numpy model (sycc_model.py) says.  Every comparison is exact."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import cblk_style_cases as style_cases
import rgba_model
import subsample_cases as cases
import sycc_model
from conftest import golden_case
from j2k_amd import synth

pytestmark = pytest.mark.gpu

J2K_HIP_ERR_PARAM = 1
SUBS = {"444": (1, 1), "422": (2, 1), "420": (2, 2)}


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
def encoded(api, enc):
    """name -> the host encode (j2k_hip_encode_to_buffer) of the fixture's components, made once; without the COM segment that
    the cases with a byte budget carry (the fixtures are stored without theirs)."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = cases.strip_com(enc.encode_components_host(cases.components(name), cases.params(api, name)))
        return cache[name]
    return get


# ------------------------------------------------------------------------------------------------ whole codestreams
@pytest.mark.parametrize("name", cases.NAMES)
def test_encode_is_byte_identical_to_libopenjp2(encoded, name):
    ours, want = encoded(name), cases.golden_bytes(name)
    assert len(ours) == len(want) == cases.entry(name)["length"]
    assert ours == want


@pytest.mark.parametrize("name", cases.NAMES)
def test_own_decoder_reads_what_libopenjp2_reads(enc, encoded, name):
    g = cases.entry(name)
    w, h = g["width"], g["height"]
    dt = np.uint8 if g["prec"] <= 8 else np.uint16
    chans = [np.zeros((h, w), dtype=dt) for _ in g["sub"]]
    enc.decode_channels(encoded(name), chans, depth=g["prec"])
    # (the decoder replicates a sub-sampled component onto the channel's grid: its own samples are every dx-th, dy-th)
    got = [hashlib.sha256(np.ascontiguousarray(chans[c][::dy, ::dx], dtype=np.int32).tobytes()).hexdigest() for c, (dx, dy) in enumerate(cases.subs(name))]
    assert got == cases.decoded_hashes(name)


def _host_planes(api, comps, p):
    dt = np.uint16 if p.depth > 8 else np.uint8
    bufs = [np.ascontiguousarray(c.astype(dt)) for c in comps]
    return bufs, api.planes_from_arrays(bufs, p.depth)


def _device_planes(api, enc, comps, p):
    """One device buffer with the components back to back (16-byte aligned) -> (device pointer, Plane array)."""
    dt = np.uint16 if p.depth > 8 else np.uint8
    bufs = [np.ascontiguousarray(c.astype(dt)) for c in comps]
    offs, pos = [], 0
    for b in bufs:
        offs.append(pos)
        pos += -(-b.nbytes // 16) * 16
    flat = np.zeros(pos, np.uint8)
    for b, o in zip(bufs, offs):
        flat[o:o + b.nbytes] = b.reshape(-1).view(np.uint8)
    d = enc.upload(flat)
    return d, api.planes_from_arrays(bufs, p.depth, base_of=lambda c: d + offs[c])


@pytest.mark.parametrize("name", cases.ENTRY_POINT_NAMES)
def test_every_entry_point_writes_these_bytes_or_refuses(api, enc, name):
    L = enc.L
    want = cases.golden_bytes(name)
    p = cases.params(api, name)
    nc = p.channels
    comps, comps2 = cases.components(name), cases.components(name, seed_offset=1000)
    sc = cases.strip_com
    assert sc(enc.encode_components_host(comps, p)) == want
    assert sc(enc.encode_components_host(comps, p, via_sink=True)) == want
    keep, planes = _host_planes(api, comps, p)
    enc._check(L.j2k_hip_encode_begin(enc.h, C.byref(p), planes))
    assert sc(enc.encode_end()) == want
    enc._check(L.j2k_hip_encode_begin_borrowed(enc.h, C.byref(p), planes))
    assert sc(enc.encode_end()) == want
    # the tile-sharded entry points refuse, naming the fields, and leave the handle usable
    out, n = np.empty(1 << 20, np.uint8), C.c_size_t()
    assert L.j2k_hip_encode_tiles(enc.h, C.byref(p), planes, 0, 1, out.ctypes.data, out.nbytes, C.byref(n)) == J2K_HIP_ERR_PARAM
    assert b"comp_sub" in L.j2k_hip_last_error(enc.h)
    d, dplanes = _device_planes(api, enc, comps, p)
    d2, dplanes2 = _device_planes(api, enc, comps2, p)
    try:
        dptr, dn = C.c_void_p(), C.c_size_t()
        assert L.j2k_hip_encode_tiles_device(enc.h, C.byref(p), dplanes, 0, 1, C.byref(dptr), C.byref(dn), None, 0) == J2K_HIP_ERR_PARAM
        assert b"comp_sub" in L.j2k_hip_last_error(enc.h)

        def device(pl):
            enc._check(L.j2k_hip_encode_device(enc.h, C.byref(p), pl, C.byref(dptr), C.byref(dn), None, 0))
            return sc(enc.d2h(dptr.value, dn.value).tobytes())
        assert device(dplanes) == want
        other = device(dplanes2)
        assert other != want
        seq = (api.Plane * (2 * nc))(*(list(dplanes) + list(dplanes2)))
        ptrs, lens = (C.c_void_p * 2)(), (C.c_size_t * 2)()
        enc._check(L.j2k_hip_encode_sequence_device(enc.h, C.byref(p), seq, 2, ptrs, lens))
        assert [sc(enc.d2h(ptrs[f], lens[f]).tobytes()) for f in range(2)] == [want, other]
    finally:
        enc.free(d)
        enc.free(d2)
    # one process, several handles: the batch writes the same files; the distributed tiles refuse
    keep2, planes2 = _host_planes(api, comps2, p)
    both = (api.Plane * (2 * nc))(*(list(planes) + list(planes2)))
    chunks = [[], []]
    ids = (C.c_void_p * 2)(1, 2)

    @api.WRITE_FN
    def write(user, buf, nbytes):
        chunks[user - 1].append(C.string_at(buf, nbytes))
        return nbytes
    devs = (C.c_int * 2)(0, 0)
    assert L.j2k_hip_encode_batch(devs, 2, 1, C.byref(p), both, 2, write, ids) == 0, L.j2k_hip_multi_last_error()
    assert [sc(b"".join(c)) for c in chunks] == [want, other]
    assert L.j2k_hip_encode_tiles_distributed(devs, 2, C.byref(p), planes, write, 1) == J2K_HIP_ERR_PARAM
    assert b"comp_sub" in L.j2k_hip_multi_last_error()
    del keep, keep2


# ------------------------------------------------------------------------------------------------ the Y Cb Cr front end
def _world(w, h, bits, kind, seed, promote, row_pad=0):
    """An After Effects A,R,G,B world of 8- or 16-bit samples -> (buffer, layout, [R, G, B, A] stored samples as int64).
    kind: "zero", "top" or "edge" = seeded noise whose last column and last row are unlike their neighbours."""
    sb = bits // 8
    top = 32768 if (promote and bits == 16) else (1 << bits) - 1  # (a 15+1-bit world ends at 32768; Promote touches 16-bit samples only)
    rng = np.random.default_rng(seed)
    if kind == "zero":
        px = np.zeros((h, w, 4), np.int64)
    elif kind == "top":
        px = np.full((h, w, 4), top, np.int64)
    else:
        px = rng.integers(0, top + 1, size=(h, w, 4), dtype=np.int64)
        px[:, -1, :] = top - px[:, max(w - 2, 0), :] if w > 1 else px[:, -1, :]
        px[-1, :, :] = (px[max(h - 2, 0), :, :] + top // 2 + 1) % (top + 1) if h > 1 else px[-1, :, :]
    rowbytes = 4 * sb * w + row_pad
    buf = np.zeros(h * rowbytes, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf.view(np.uint16) if sb == 2 else buf, shape=(h, w, 4), strides=(rowbytes, 4 * sb, sb), writeable=True)
    view[...] = px.astype(view.dtype)
    lay = dict(sample_bytes=sb, colbytes=4 * sb, rowbytes=rowbytes, channel_offsets=(0, sb, 2 * sb, 3 * sb))
    return buf, lay, [px[:, :, 1], px[:, :, 2], px[:, :, 3], px[:, :, 0]]


def _to_depth(stored, bits, src_depth, depth, promote):
    out = []
    for s in stored:
        v = sycc_model.promote(s) if (promote and bits == 16) else s
        out.append(rgba_model.depth_convert(v, src_depth, depth, 32))
    return out


def _same(got, want, rev):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return False
    return np.array_equal(got, want) if rev else np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32))


#            bits depth nc  rev    promote row_pad
AE_CONFIGS = [(8, 8, 3, True, False, 0), (8, 8, 4, False, False, 4), (16, 16, 4, True, False, 0), (16, 16, 3, False, True, 8),
              (16, 12, 3, True, False, 0), (16, 12, 4, False, True, 0), (16, 16, 4, True, True, 0), (8, 8, 4, True, True, 0)]
SIZES = [(1, 1), (2, 1), (1, 2), (3, 3), (17, 9), (97, 61), (130, 65)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("chroma", ["444", "422", "420"])
def test_frontend_equals_the_model_interleaved_worlds(api, enc, chroma, size):
    w, h = size
    sub = SUBS[chroma]
    for k, (bits, depth, nc, rev, promote, pad) in enumerate(AE_CONFIGS):
        for kind in ("edge", "zero", "top"):
            buf, lay, stored = _world(w, h, bits, kind, 1000 * k + w + 7 * h, promote, pad)
            p = api.make_params(w, h, nc, depth, reversible=rev, promote=promote, num_resolutions=1,
                                sub=[(1, 1), sub, sub] + [(1, 1)] * (nc - 3), rgb_to_sycc=True)
            got = enc.stage_frontend(buf, lay, p)
            want = sycc_model.frontend_planes(_to_depth(stored[:nc], bits, bits, depth, promote), depth, sub)
            assert len(got) == nc
            for c in range(nc):
                assert _same(got[c], want[c], rev), (bits, depth, nc, rev, promote, kind, c)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("chroma", ["444", "422", "420"])
def test_frontend_equals_the_model_planar_strided_views(api, enc, chroma, size):
    """Planar channels with padded rows, each in a buffer region of its own; samples that hold `depth` bits and samples that
    are converted (10 in 16 -> 12; 8 -> 8)."""
    w, h = size
    sub = SUBS[chroma]
    for k, (dt, src_depth, depth, nc, rev) in enumerate([(np.uint16, 10, 10, 3, True), (np.uint8, 8, 8, 4, False), (np.uint16, 10, 12, 4, True),
                                                         (np.uint16, 16, 12, 3, False)]):
        rng = np.random.default_rng(77 * k + w + 3 * h)
        top = (1 << src_depth) - 1
        rowlen = w + 3 + k  # samples per padded row
        store = rng.integers(0, top + 1, size=(nc, h, rowlen)).astype(dt)
        store[:, :, w - 1] = top - store[:, :, max(w - 2, 0)]
        store[:, h - 1, :] = (store[:, max(h - 2, 0), :].astype(np.int64) + top // 2 + 1) % (top + 1)
        views = [store[c, :, :w] for c in range(nc)]
        p = api.make_params(w, h, nc, depth, reversible=rev, num_resolutions=1, sub=[(1, 1), sub, sub] + [(1, 1)] * (nc - 3), rgb_to_sycc=True)
        planes = lambda d: api.planes_from_arrays(views, src_depth, base_of=lambda c: d + (views[c].ctypes.data - store.ctypes.data))
        got = enc.stage_frontend_planes(store, planes, p)
        want = sycc_model.frontend_planes(_to_depth([v.astype(np.int64) for v in views], 8 * store.itemsize, src_depth, depth, False), depth, sub)
        for c in range(nc):
            assert _same(got[c], want[c], rev), (k, c)


# ------------------------------------------------------------------------------------------------ the transform
def _mallat(oracle, plane, rev, levels, tiles, sub):
    """Every tile-component's Mallat layout in place: the tile on the component's grid is ceil(tile / sub)."""
    dx, dy = sub
    src = np.ascontiguousarray(plane, dtype=np.int32 if rev else np.float32)
    out = np.empty_like(src)
    f = oracle.dwt53 if rev else oracle.dwt97
    for (x0, y0, x1, y1) in tiles:
        cx0, cy0, cx1, cy1 = -(-x0 // dx), -(-y0 // dy), -(-x1 // dx), -(-y1 // dy)
        if cx1 > cx0 and cy1 > cy0:
            out[cy0:cy1, cx0:cx1] = f(src[cy0:cy1, cx0:cx1], levels, cx0, cy0)
    return out


@pytest.mark.parametrize("name", cases.TRANSFORM_NAMES)
def test_transform_of_component_planes_equals_the_oracle(api, enc, oracle, name):
    g = cases.entry(name)
    w, h, prec = g["width"], g["height"], g["prec"]
    p = cases.params(api, name)
    rev, levels = bool(p.reversible), p.num_resolutions - 1
    ts = p.tile_size or max(w, h)
    tiles = [(x, y, min(x + ts, w), min(y + ts, h)) for y in range(0, h, ts) for x in range(0, w, ts)]
    comps = cases.components(name)
    dt = np.uint16 if prec > 8 else np.uint8
    bufs = [np.ascontiguousarray(c.astype(dt)) for c in comps]
    offs = np.cumsum([0] + [-(-b.nbytes // 16) * 16 for b in bufs])
    flat = np.zeros(int(offs[-1]), np.uint8)
    for b, o in zip(bufs, offs):
        flat[o:o + b.nbytes] = b.reshape(-1).view(np.uint8)
    got = enc.stage_transform(flat, lambda d: api.planes_from_arrays(bufs, prec, base_of=lambda c: d + int(offs[c])), p)
    assert len(got) == len(comps)
    for c, sub in enumerate(cases.subs(name)):
        want = _mallat(oracle, comps[c].astype(np.int64) - (1 << (prec - 1)), rev, levels, tiles, sub)
        assert got[c].shape == want.shape
        assert np.array_equal(got[c].view(np.int32), want.view(np.int32)), (name, c)


@pytest.mark.parametrize("name", cases.TRANSFORM_NAMES[:2])
def test_transform_behind_the_ycc_front_end_equals_the_oracle(api, enc, oracle, name):
    """The q2 / q3 geometries (4:2:0, 9/7 with 4 resolutions; 4:2:0 with alpha, 5/3) from an RGB[A] world."""
    g = cases.entry(name)
    w, h, prec, nc = g["width"], g["height"], g["prec"], len(g["sub"])
    bits = 8 if prec <= 8 else 16
    p = cases.params(api, name, rgb_to_sycc=True)
    rev, levels = bool(p.reversible), p.num_resolutions - 1
    buf, lay, stored = _world(w, h, bits, "edge", 4242, False, 8)
    model = sycc_model.frontend_planes(_to_depth(stored[:nc], bits, bits, prec, False), prec, cases.subs(name)[1])
    got = enc.stage_transform(buf, lambda d: api.planes_from_layout(d, lay, nc), p)
    for c, sub in enumerate(cases.subs(name)):
        want = _mallat(oracle, model[c], rev, levels, [(0, 0, w, h)], sub)
        assert np.array_equal(np.asarray(got[c]).view(np.int32), want.view(np.int32)), (name, c)


@pytest.mark.parametrize("chroma, tile, prog, rev", [("420", 33, 2, True), ("422", 50, 4, False), ("420", 64, 3, True)])
def test_tiled_encode_behind_the_ycc_front_end(api, enc, oracle, chroma, tile, prog, rev):
    """rgb_to_sycc with tiles (what HipCodec reaches with settings.tileSize): odd tile sizes that are no multiple of the
    factors, the position-driven progressions.  The transform equals the oracle's DWT of the model's planes per tile-component,
    and the whole file decodes to the model's planes (5/3) with the tile grid and the factors in its header."""
    w, h, nc, prec = 97, 61, 4, 8
    sub = SUBS[chroma]
    subs = [(1, 1), sub, sub, (1, 1)]
    p = api.make_params(w, h, nc, prec, reversible=rev, tile_size=tile, num_resolutions=3, progression=prog, sub=subs, rgb_to_sycc=True)
    buf, lay, stored = _world(w, h, 8, "edge", 31 + tile, False, 4)
    tiles = [(x, y, min(x + tile, w), min(y + tile, h)) for y in range(0, h, tile) for x in range(0, w, tile)]
    assert len(tiles) > 1
    model = sycc_model.frontend_planes(stored, prec, sub)
    got = enc.stage_transform(buf, lambda d: api.planes_from_layout(d, lay, nc), p)
    for c in range(nc):
        want = _mallat(oracle, model[c], rev, 2, tiles, subs[c])
        assert np.array_equal(np.asarray(got[c]).view(np.int32), want.view(np.int32)), c
    data = enc.encode_host(buf, lay, p)
    d = enc.upload(buf)
    try:
        assert enc.encode_device(d, lay, p)[2] == data
    finally:
        enc.free(d)
    info = api.read_info(data)
    assert (info["tile_width"], info["tile_height"], info["progression"]) == (min(tile, w), min(tile, h), prog)  # (the reader reports a tile cut to the image)
    assert (info["sub_x"][:4], info["sub_y"][:4]) == ([s[0] for s in subs], [s[1] for s in subs])
    if rev:
        chans = [np.zeros((h, w), np.uint8) for _ in range(nc)]
        enc.decode_channels(data, chans, depth=prec)
        ycc = sycc_model.sycc_planes(stored, prec, sub)
        for c in range(nc):
            assert np.array_equal(chans[c][::subs[c][1], ::subs[c][0]], ycc[c]), c


# ------------------------------------------------------------------------------------------------ host planes of their own
def _apart(arrays):
    """Copies of the arrays that are allocations of their own, megabytes of other allocations between them.  The allocator puts
    a copy where it finds room, and holes that earlier tests' arrays left in the heap may take the small copies side by side
    while the spacers go elsewhere: such an attempt is kept alive (it fills the holes) and the copies are made again."""
    kept = []
    for _ in range(32):
        out, spacers = [], []
        for a in arrays:
            spacers.append(np.full(3 << 20, 7, np.uint8))
            out.append(np.array(a, copy=True, order="C"))
        lo = min(a.ctypes.data for a in out)
        hi = max(a.ctypes.data + a.nbytes for a in out)
        if hi - lo > sum(a.nbytes for a in out) + (1 << 20):
            return out, spacers + kept
        kept += out + spacers
    raise AssertionError("the planes were not allocated apart")


def test_separately_allocated_component_planes(api, enc):
    """512 x 512 at 4:2:0: a 256 KiB luma plane and two 64 KiB chroma planes, each an allocation of its own (one beyond the
    allocator's mmap threshold, two below it): every plane goes up by itself, whatever lies between them."""
    w = h = 512
    pl = synth.planes(w, h, 3, 8, 901, "B")
    comps = [pl[0].astype(np.uint8), pl[1][:256, :256].astype(np.uint8), pl[2][:256, :256].astype(np.uint8)]
    p = api.make_params(w, h, 3, 8, num_resolutions=4, sub=[(1, 1), (2, 2), (2, 2)])
    d, dplanes = _device_planes(api, enc, comps, p)
    try:
        dptr, dn = C.c_void_p(), C.c_size_t()
        enc._check(enc.L.j2k_hip_encode_device(enc.h, C.byref(p), dplanes, C.byref(dptr), C.byref(dn), None, 0))
        want = enc.d2h(dptr.value, dn.value).tobytes()
    finally:
        enc.free(d)
    bufs, spacers = _apart(comps)
    planes = api.planes_from_arrays(bufs, 8)
    assert enc._encode_planes_host(planes, sum(b.nbytes for b in bufs), p, False) == want
    assert enc._encode_planes_host(planes, sum(b.nbytes for b in bufs), p, True) == want
    assert enc.encode_components_host(comps, p) == want
    chans = [np.zeros((h, w), np.uint8) for _ in range(3)]
    enc.decode_channels(want, chans, depth=8)
    assert np.array_equal(chans[0], comps[0]) and np.array_equal(chans[1][::2, ::2], comps[1]) and np.array_equal(chans[2][::2, ::2], comps[2])
    del spacers


def test_separately_allocated_full_size_planes(api, enc):
    """The same for components of one size (no sub-sampling, RCT): three 256 KiB planes apart write what one buffer writes."""
    w = h = 512
    pl = synth.planes(w, h, 3, 8, 902, "B")
    p = api.make_params(w, h, 3, 8, ycc=True, num_resolutions=4)
    want = enc.encode_planar_host(pl, p)
    bufs, spacers = _apart([pl[c].astype(np.uint8) for c in range(3)])
    assert enc._encode_planes_host(api.planes_from_arrays(bufs, 8), 3 * w * h, p, False) == want
    del spacers


# ------------------------------------------------------------------------------------------------ round trips
@pytest.mark.parametrize("size", [(97, 61), (130, 65)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("chroma", ["422", "420"])
def test_round_trip_through_the_rgba_reader(api, enc, chroma, size):
    w, h = size
    sub = SUBS[chroma]
    buf, lay, stored = _world(w, h, 16, "edge", 99 + w, False, 0)
    ycc = sycc_model.sycc_planes(stored[:3], 16, sub)
    p = api.make_params(w, h, 3, 16, jp2=True, color_space=3, sub=[(1, 1), sub, sub], rgb_to_sycc=True)
    data = enc.encode_host(buf, lay, p)
    assert api.rgba_mode(data) == api.RGBA_SYCC
    info = api.read_info(data)
    assert (info["sub_x"][:3], info["sub_y"][:3]) == ([1, sub[0], sub[0]], [1, sub[1], sub[1]])
    blank = np.full(buf.size, 0x5a, np.uint8)
    got = enc.decode_rgba(data, blank.copy(), lay, w, h, depth=16)
    want = rgba_model.rgba(rgba_model.SYCC, ycc, [16] * 3, [(1, 1), sub, sub], w, h, 16, 16)
    assert np.all(want[3] == 65535)  # no alpha in the file: the destination gets the fill value
    assert np.array_equal(got, rgba_model.into_ae_frame(blank, lay, want))
    # alpha kept as a fourth, full-size component: it comes back unchanged, beside Y
    p4 = api.make_params(w, h, 4, 16, jp2=True, color_space=3, alpha_channel=3, sub=[(1, 1), sub, sub, (1, 1)], rgb_to_sycc=True)
    data4 = enc.encode_host(buf, lay, p4)
    chans = [np.zeros((h, w), np.uint16) for _ in range(4)]
    enc.decode_channels(data4, chans, depth=16)
    assert np.array_equal(chans[3], stored[3])
    assert np.array_equal(chans[0], ycc[0])
    assert np.array_equal(chans[1][::sub[1], ::sub[0]], ycc[1]) and np.array_equal(chans[2][::sub[1], ::sub[0]], ycc[2])


@pytest.fixture(scope="module")
def host(api):
    from j2k_amd import build
    path = os.path.join(os.path.dirname(api.LIBPATH), "libj2k_host.so")
    if not os.path.exists(path):
        build.build_host()
    api.load_library()
    H = C.CDLL(path)
    H.j2k_host_test_write_ex.restype = C.c_long
    H.j2k_host_test_write_ex.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_long] + [C.c_int] * 8 + [C.c_long, C.c_int, C.c_int,
                                         C.c_char_p, C.c_ulong, C.c_int, C.c_void_p, C.c_ulong, C.c_char_p, C.c_ulong]
    H.j2k_host_test_read_rgba.restype = C.c_long
    H.j2k_host_test_read_rgba.argtypes = [C.c_void_p, C.c_ulong, C.c_uint, C.c_void_p, C.c_uint, C.c_uint, C.c_long, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.c_char_p, C.c_ulong]
    return H


def _env(**kw):
    class Env:
        def __enter__(self):
            self.old = {k: os.environ.get(k) for k in kw}
            for k, v in kw.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v

        def __exit__(self, *a):
            for k, v in self.old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    return Env()


@pytest.mark.parametrize("promote", [False, True])
@pytest.mark.parametrize("chroma", ["422", "420"])
def test_hip_codec_writes_and_reads_sub_sampled_chroma(api, enc, host, chroma, promote):
    w, h = 97, 61
    sub = SUBS[chroma]
    buf, lay, stored = _world(w, h, 16, "edge", 555, promote, 0)
    JP2_FMT, SRGB = 2, 1

    def write(honour, chroma_env):
        out, err = np.empty(buf.nbytes + (1 << 16), np.uint8), C.create_string_buffer(512)
        with _env(J2K_HOST_TEST_CHROMA=chroma_env, J2K_HOST_TEST_PROMOTE="1" if promote else None):
            n = host.j2k_host_test_write_ex(buf.ctypes.data, w, h, lay["rowbytes"], 2, 4, 16, 1, 1, 1, 0, int(honour), -1, JP2_FMT, SRGB, None, 0, -1,
                                            out.ctypes.data, out.nbytes, err, 512)
        assert n >= 0, err.value
        return out[:n].tobytes()
    data = write(True, chroma)
    p = api.make_params(w, h, 4, 16, reversible=True, ycc=False, comment=None, jp2=True, color_space=3, alpha_channel=3, promote=promote,
                        sub=[(1, 1), sub, sub, (1, 1)], rgb_to_sycc=True)
    assert data == enc.encode_host(buf, lay, p)
    # ReadRGBA takes the file (sYCC) and returns the model's R, G, B; A is filled
    frame = np.full(buf.size, 0x5a, np.uint8)
    err = C.create_string_buffer(512)
    arr = np.frombuffer(data, np.uint8)
    assert host.j2k_host_test_read_rgba(arr.ctypes.data, len(data), 1, frame.ctypes.data, w, h, lay["rowbytes"], 2, 16, 0, 1, err, 512) == 1, err.value
    ycc = sycc_model.sycc_planes(_to_depth(stored[:3], 16, 16, 16, promote), 16, sub)
    want = rgba_model.rgba(rgba_model.SYCC, ycc, [16] * 3, [(1, 1), sub, sub], w, h, 16, 16)
    assert np.array_equal(frame, rgba_model.into_ae_frame(np.full(buf.size, 0x5a, np.uint8), lay, want))
    # ReferenceLiteral ignores the option bits: the raw codestream it has always written for this world -- 5/3, no colour
    # transform, four full-size components, the library's own COM -- pinned by the plain C-ABI encode it maps to
    literal = enc.encode_host(buf, lay, api.make_params(w, h, 4, 16, reversible=True, ycc=False, comment=None, promote=promote))
    assert write(False, chroma) == literal
    assert write(False, None) == literal
    assert api.read_info(literal)["sub_x"][:4] == [1, 1, 1, 1] and literal[:2] == b"\xff\x4f"


# ------------------------------------------------------------------------------------------------ what stays as it was
def test_sub_sampled_host_call_is_not_band_pipelined(api, enc):
    """2048 x 1024 ARGB64 is 16 MiB, the band threshold: without sub-sampling the synchronous call goes up in bands (today's
    behaviour, observed here and not changed), with it the frame goes up in one piece."""
    w, h = 2048, 1024
    pl = synth.planes(w, h, 4, 16, 31, "B")  # (four channels: the bytes the call uploads begin at the first A sample)
    frame, lay = synth.ae_frame(pl, 16)
    assert frame.nbytes == 16 << 20
    plain = api.make_params(w, h, 4, 16, reversible=False, ycc=True)
    p422 = api.make_params(w, h, 4, 16, reversible=False, sub=[(1, 1), (2, 1), (2, 1), (1, 1)], rgb_to_sycc=True)
    enc.encode_host(frame, lay, plain, via_sink=True)
    assert enc.stats()["bands"] > 0
    ours = enc.encode_host(frame, lay, p422, via_sink=True)
    assert enc.stats()["bands"] == 0
    d = enc.upload(frame)
    try:
        assert enc.encode_device(d, lay, p422)[2] == ours
    finally:
        enc.free(d)


def test_all_ones_factors_move_nothing(api, enc, golden):
    for name in ("g3_300x200_rgb8_53_rct", "g9_150x130_rgb8_97_tile64"):
        g, pl, _, cs = golden_case(golden, name)
        kw = g["params"]
        p = api.make_params(g["width"], g["height"], g["ncomp"], g["prec"], reversible=kw.get("reversible", True), ycc=kw.get("mct", False),
                            tile_size=kw.get("tile", 0), num_resolutions=kw.get("numres", 6), comment="", sub=[(1, 1)] * g["ncomp"], rgb_to_sycc=False)
        assert enc.encode_planar_host(pl, p) == cs, name
        frame, lay = synth.ae_frame(pl, g["prec"])
        assert enc.encode_host(frame, lay, p) == cs, name
    name = "y9_150x130_rgb10_53_bypass_reset_segsym_tile64_rpcl"
    p = style_cases.params(api, name, sub=[(1, 1)] * 3)
    assert enc.encode_planar_host(style_cases.planes(name), p) == style_cases.golden_bytes(name)
