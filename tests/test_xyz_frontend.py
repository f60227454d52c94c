"""GPU: frontend_xyz_kernel through j2k_hip_stage_frontend against the numpy model (xyz_model.py) fed with the library's own
tables (api.xyz_tables): exact equality.  Shapes are the smallest at which the indexing can go wrong -- padded rows, one lane
past a workgroup's 256 columns, every sample type, with and without alpha, the LDS search (depth 8, 12) and the global-memory
search (depth 16), both wavelets, the RCT behind the codes."""
import numpy as np
import pytest

import xyz_model
from j2k_amd import api, synth

pytestmark = pytest.mark.gpu


def P(*a, **kw):
    """make_params without a wavelet's limit on the frame size: the stage ends before the DWT."""
    kw.setdefault("num_resolutions", 1)
    return api.make_params(*a, **kw)


@pytest.fixture(scope="module")
def enc():
    e = api.Encoder()
    yield e
    e.close()


_tables = {}


def tables(source, src_depth, dst_depth):
    key = (source, src_depth, dst_depth)
    if key not in _tables:
        _tables[key] = api.xyz_tables(source, src_depth, dst_depth)
    return _tables[key]


def model(rgb, source, src_depth, dst_depth):
    """X'Y'Z' codes minus the DC shift, (3, h, w) int64, from integer samples of src_depth bits."""
    return xyz_model.codes(rgb, source, src_depth, dst_depth, tables=tables(source, src_depth, dst_depth)) - (1 << (dst_depth - 1))


def planar_views(arrays, depth_bits):
    """2-D arrays -> (one buffer with every plane at a multiple of 16 bytes, device address -> Plane array)."""
    offs, pos = [], 0
    for a in arrays:
        offs.append(pos)
        pos += -(-a.nbytes // 16) * 16
    buf = np.zeros(pos, np.uint8)
    for a, o in zip(arrays, offs):
        buf[o:o + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    dense = [np.ascontiguousarray(a) for a in arrays]
    return buf, lambda addr: api.planes_from_arrays(dense, depth_bits, base_of=lambda c: addr + offs[c])


def rand16(shape, seed, top=65535):
    return np.random.default_rng(seed).integers(0, top + 1, size=shape, dtype=np.int64)


@pytest.mark.parametrize("promote", [False, True], ids=["plain", "promote"])
def test_argb64_with_padded_rows(enc, promote):
    w, h = 67, 5
    pl = rand16((3, h, w), 11, 32768 if promote else 65535)
    pl[:, 0, :4] = [[0, 1, 16384, 16385]] * 3
    pl[:, 1, :2] = [[32768, 32767]] * 3
    frame, lay = synth.ae_frame(pl.astype(np.int32), 16, row_pad_bytes=8)
    for source in (1, 2, 3):
        got = enc.stage_frontend(frame, lay, P(w, h, 3, 12, promote=promote, rgb_to_xyz=source))
        v = xyz_model.promote16(pl) if promote else pl
        assert np.array_equal(got, model(v, source, 16, 12)), source


def test_planar_8_bit_one_lane_past_a_workgroup(enc):
    w, h = 257, 3
    pl = rand16((3, h, w), 12, 255)
    pl[:, :, 256] = [[0, 255, 128]] * 3
    buf, planes = planar_views([p.astype(np.uint8) for p in pl], 8)
    for source in (1, 2, 3):
        got = enc.stage_frontend_planes(buf, planes, P(w, h, 3, 12, rgb_to_xyz=source))
        assert np.array_equal(got, model(pl, source, 8, 12)), source


def test_planar_planes_of_unlike_depths(enc):
    """R of 8 bits, G of 12 bits in 16-bit samples, B of 16 bits: a linear-light table per channel."""
    w, h = 33, 4
    r, g, b = rand16((h, w), 1, 255), rand16((h, w), 2, 4095), rand16((h, w), 3)
    arrays = [r.astype(np.uint8), g.astype(np.uint16), b.astype(np.uint16)]
    offs = [0, 256, 512 + 2 * w * h]
    buf = np.zeros(offs[2] + 2 * w * h + 16, np.uint8)
    for a, o in zip(arrays, offs):
        buf[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)

    def planes(addr):
        arr = api.planes_from_arrays(arrays, 8, base_of=lambda c: addr + offs[c])
        arr[1].depth, arr[2].depth = 12, 16
        return arr
    got = enc.stage_frontend_planes(buf, planes, P(w, h, 3, 12, rgb_to_xyz=1))
    lins = [tables(1, d, 12)[0] for d in (8, 12, 16)]
    want = xyz_model.codes([r, g, b], 1, (8, 12, 16), 12, tables=(lins,) + tuple(tables(1, 8, 12)[1:])) - 2048
    assert np.array_equal(got, want)


@pytest.mark.parametrize("promote", [False, True], ids=["plain", "promote"])
def test_argb128_floats_with_specials(enc, promote):
    w, h = 64, 4
    pl = rand16((3, h, w), 13)
    frame, lay = synth.ae_frame_float(pl.astype(np.int32), 16, promote=promote)
    f = np.lib.stride_tricks.as_strided(frame.view(np.float32), shape=(h, w, 4), strides=(lay["rowbytes"], 16, 4), writeable=True)
    rng = np.random.default_rng(5)
    f[1, :, 1:] = rng.random((w, 3), dtype=np.float32) * np.float32(1.25) - np.float32(0.125)  # off the grid, below 0, above 1
    f[0, :8, 1] = [np.nan, -1.0, 1.5, -0.0, 0.0, np.inf, -np.inf, 1.0]
    f[0, :8, 2] = [0.5, np.nan, 2.0 ** -20, 1.0 - 2.0 ** -24, 1.0 + 2.0 ** -23, 0.25, 1e-30, -1e-30]
    f[0, :8, 3] = [1.0, 0.0, np.nan, np.inf, -0.0, 0.999, 0.001, 3.0]
    v = np.stack([xyz_model.quantise_float(f[:, :, 1 + c], 16, promote) for c in range(3)])
    for source in (1, 2, 3):
        got = enc.stage_frontend(frame, lay, P(w, h, 3, 12, promote=promote, rgb_to_xyz=source))
        assert np.array_equal(got, model(v, source, 16, 12)), source


@pytest.mark.parametrize("bits", [8, 16])
def test_alpha_passes_through_as_without_the_field(enc, bits):
    w, h = 70, 6
    pl = rand16((4, h, w), 14, (1 << bits) - 1)
    frame, lay = synth.ae_frame(pl.astype(np.int32), bits, row_pad_bytes=16)
    for rev in (True, False):
        plain = enc.stage_frontend(frame, lay, P(w, h, 4, 12, reversible=rev))
        got = enc.stage_frontend(frame, lay, P(w, h, 4, 12, reversible=rev, rgb_to_xyz=1))
        assert got.dtype == plain.dtype and np.array_equal(got[3], plain[3])
        assert np.array_equal(got[:3].astype(np.int64), model(pl[:3], 1, bits, 12))
        assert not np.array_equal(got[:3], plain[:3])


@pytest.mark.parametrize("depth", [1, 2, 8, 10, 12, 13, 16])
def test_destination_depths(enc, depth):
    """Up to 12 bits the thresholds are searched in LDS, above in global memory; 1 and 2: the smallest tables."""
    w, h = 300, 7
    pl = rand16((3, h, w), 20 + depth)
    pl[:, 0, :3] = [[0, 65535, 1]] * 3
    frame, lay = synth.ae_frame(pl.astype(np.int32), 16)
    for source in (1, 3):
        got = enc.stage_frontend(frame, lay, P(w, h, 3, depth, rgb_to_xyz=source))
        want = model(pl, source, 16, depth)
        assert np.array_equal(got, want), source
        assert want.min() == -(1 << (depth - 1)) and want.max() <= (1 << (depth - 1)) - 1


@pytest.mark.parametrize("depth", [12, 16])
def test_irreversible_planes_hold_the_same_integers_and_the_rct_follows(enc, depth):
    w, h = 131, 9
    pl = rand16((3, h, w), 15)
    frame, lay = synth.ae_frame(pl.astype(np.int32), 16, row_pad_bytes=8)
    want = model(pl, 2, 16, depth)
    irr = enc.stage_frontend(frame, lay, P(w, h, 3, depth, reversible=False, rgb_to_xyz=2))
    assert irr.dtype == np.float32 and np.array_equal(irr, want.astype(np.float32))
    got = enc.stage_frontend(frame, lay, P(w, h, 3, depth, reversible=True, ycc=True, rgb_to_xyz=2))
    assert np.array_equal(got, xyz_model.rct(want))
    # the ICT of the same integers, product by product as the plain front end forms it
    ict = enc.stage_frontend(frame, lay, P(w, h, 3, depth, reversible=False, ycc=True, rgb_to_xyz=2))
    r, g, b = (want[i].astype(np.float32) for i in range(3))
    f = np.float32
    y = (f(0.299) * r + f(0.587) * g) + f(0.114) * b
    cb = (f(-0.16875) * r + f(-0.331260) * g) + f(0.5) * b
    cr = (f(0.5) * r + f(-0.41869) * g) + f(-0.08131) * b
    assert np.array_equal(ict, np.stack([y, cb, cr]).astype(np.float32))


@pytest.mark.parametrize("source", [1, 2, 3])
def test_every_code_value_on_the_grey_axis(enc, source):
    v = np.arange(65536, dtype=np.int64).reshape(256, 256)
    pl = np.stack([v, v, v])
    frame, lay = synth.ae_frame(pl.astype(np.int32), 16)
    got = enc.stage_frontend(frame, lay, P(256, 256, 3, 12, rgb_to_xyz=source))
    want = model(pl, source, 16, 12)
    assert np.array_equal(got, want)
    assert np.all(np.diff(got.reshape(3, -1), axis=1) >= 0)


@pytest.mark.parametrize("source", [1, 2, 3])
def test_a_lattice_of_colours_and_a_random_frame(enc, source):
    k = np.round(np.linspace(0, 65535, 17)).astype(np.int64)
    r, g, b = np.meshgrid(k, k, k, indexing="ij")
    pl = np.stack([r.reshape(17, 289), g.reshape(17, 289), b.reshape(17, 289)])
    frame, lay = synth.ae_frame(pl.astype(np.int32), 16)
    got = enc.stage_frontend(frame, lay, P(289, 17, 3, 12, rgb_to_xyz=source))
    assert np.array_equal(got, model(pl, source, 16, 12))
    pl = rand16((3, 37, 523), 100 + source)
    frame, lay = synth.ae_frame(pl.astype(np.int32), 16, row_pad_bytes=24)
    got = enc.stage_frontend(frame, lay, P(523, 37, 3, 12, rgb_to_xyz=source))
    assert np.array_equal(got, model(pl, source, 16, 12))


def test_stored_samples_above_their_depth_count_as_the_top(enc):
    """A 16-bit plane that says depth 12 but holds larger values: the table has 4096 entries and nothing beyond is read."""
    w, h = 40, 2
    pl = rand16((3, h, w), 16)
    arrays = [p.astype(np.uint16) for p in pl]
    buf, planes = planar_views(arrays, 12)
    got = enc.stage_frontend_planes(buf, planes, P(w, h, 3, 12, rgb_to_xyz=1))
    assert np.array_equal(got, model(np.minimum(pl, 4095), 1, 12, 12))
