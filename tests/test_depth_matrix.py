"""GPU: every encode-side copy of the depth conversion, through the stage hooks, over every (sample type, channel depth, file
depth) of depth_cases.PAIRS -- 384 triples -- and every legal stored value of each.  Every comparison is word for word (the
int32 view of the hook's output); there is no tolerance in this file.

Each test function is parametrised by the file depth prec = 1..16 (16 ids) and walks the 24 (sample_bits, d) of that depth
inside: 8-bit samples of depth 1..8 on 17 x 512 frames, 16-bit samples of depth 1..16 on 129 x 512 frames (depth_cases.channel:
the exhaustive ramp, rotated per channel, and a row of full-range corners).  8 + 16 channel depths x 16 file depths = 384.
512 columns, because a narrower frame has no FAST strip in the fused kernel (depth_cases.shape).

  a  test_strided_front_end       frontend_kernel, fe_load's strided branch: four channels of unequal depth per launch, no MCT
  b  test_interleaved_front_end   frontend_kernel, fe_unpack32 / fe_unpack64: four channels, RCT and ICT
  c  test_fused_level_1           dwt_fused_kernel's sample(): GEN (d < prec), `smp >> rs` (d > prec), SPEC (d == prec) and the
                                  generic kernel at d == prec under fused_generic
  d  test_ycc_front_end           frontend_sycc_kernel's fe_sample, 4:2:0
  e  test_compare_kernel          compare.hip's fe_sample: dense aligned planes (four samples per load) and strided views
  f  test_float_channels          fe_quantise_float + depth_convert over depth_cases.FLOAT_PAIRS (256): strided and ARGB128
  g  test_promote                 promote_ae16 over every 16-bit stored value, through a, b, c and f

The model: depth_cases.convert (held to the oracle's CopyChannel by test_depth_model.py), Promote in numpy where asked, then
the oracle's DC shift and RCT / ICT (j2ko_dc_mct) and, for c, one level of its dwt53 / dwt97.

Not reached, on purpose: depth_convert's "two fills" branch (src_depth >= 8 and shift > src_depth) needs a destination deeper
than twice the source, that is more than 16 bits; no file depth the ABI accepts takes it."""
import functools

import numpy as np
import pytest

import compare_model as cm
import depth_cases as dc
import sycc_model

pytestmark = pytest.mark.gpu

PREC = pytest.mark.parametrize("prec", dc.PRECS, ids=lambda p: f"prec{p}")


@pytest.fixture(scope="module")
def api():
    from j2k_amd import api
    return api


@pytest.fixture(scope="module")
def enc(api):
    e = api.Encoder(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=32)
def _frame(sample_bits, d):
    """(channels (4, H, W), frame bytes, layout) of the After Effects frame whose four channels have depth d."""
    ch = dc.channels(sample_bits, [d] * 4)
    buf, lay = dc.interleaved(list(ch), sample_bits)
    ch.setflags(write=False)
    buf.setflags(write=False)
    return ch, buf, lay


def _depths(api, arrays, base_of, ds):
    """Address of the buffer -> the Plane array of `arrays` with channel c at depth ds[c]."""
    def make(dev):
        arr = api.planes_from_arrays(arrays, 0, base_of=lambda c: dev + base_of(c))
        for c, d in enumerate(ds):
            arr[c].depth = d
        return arr
    return make


def _strided_views(api, chans, dt, ds):
    store, views = dc.strided(chans, dt)
    return store, _depths(api, views, lambda c: views[c].ctypes.data - store.ctypes.data, ds)


def _check(got, want, what):
    g = np.ascontiguousarray(got).view(np.int32)
    assert g.shape == want.shape, (what, g.shape, want.shape)
    if not np.array_equal(g, want):
        bad = np.argwhere(g != want)
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} words differ, first at {i}: got 0x{int(g[i]) & 0xffffffff:08x}, "
                             f"model 0x{int(want[i]) & 0xffffffff:08x}")


def _as_float_words(ints):
    return np.ascontiguousarray(np.asarray(ints).astype(np.float32)).view(np.int32)


# ------------------------------------------------------------------------------------------------ a
def _strided_front_end(api, enc, oracle, chans, sample_bits, ds, prec, promoted=False):
    smp = dc.samples(chans, ds, prec, promoted)
    _, h, w = smp.shape
    store, make = _strided_views(api, chans, dc.dtype_of(sample_bits), ds)
    words = dc.frontend_words(oracle, smp, prec, True, False)
    assert np.array_equal(words, smp - (1 << (prec - 1)))
    for rev in (True, False):
        p = api.make_params(w, h, len(ds), prec, reversible=rev, ycc=False, promote=promoted, num_resolutions=1)
        want = dc.frontend_words(oracle, smp, prec, rev, False)
        if not rev:
            assert np.array_equal(want, _as_float_words(words))  # float32 of the same integers
        _check(enc.stage_frontend_planes(store, make, p), want, f"strided {sample_bits}-bit depths {ds} -> {prec} {'53' if rev else '97'}")


@PREC
def test_strided_front_end(api, enc, oracle, prec):
    """a: planar views (every second sample of a padded row), four channels of unequal depth in one launch -- the arrangement
    that keeps an encode off the fused path (encoder.cpp: fuse_frontend).  No MCT; 5/3 and 9/7."""
    for sample_bits, groups in dc.GROUPS.items():
        for ds in groups:
            _strided_front_end(api, enc, oracle, dc.channels(sample_bits, ds), sample_bits, ds, prec)


# ------------------------------------------------------------------------------------------------ b
@PREC
def test_interleaved_front_end(api, enc, oracle, prec):
    """b: ARGB32 / ARGB64 frames whose samples have depth d; four channels with the RCT (5/3) and the ICT (9/7), the frame's
    last row holding every full-range corner of R, G, B."""
    for sample_bits, d in dc.pairs_of(prec):
        ch, buf, lay = _frame(sample_bits, d)
        smp = dc.samples(ch, [d] * 4, prec)
        _, h, w = ch.shape
        for rev in (True, False):
            p = api.make_params(w, h, 4, prec, reversible=rev, ycc=True, num_resolutions=1)
            _check(enc.stage_frontend(buf, lay, p, depth_bits=d), dc.frontend_words(oracle, smp, prec, rev, True),
                   f"interleaved {sample_bits}-bit depth {d} -> {prec} {'53' if rev else '97'}")


# ------------------------------------------------------------------------------------------------ c
def _fused_level_1(api, enc, oracle, ch, buf, lay, d, prec, promoted=False, what=""):
    _, h, w = ch.shape
    for rev, nc in ((True, 3), (False, 4)):
        smp = dc.samples(ch[:nc], [d] * nc, prec, promoted)
        p = api.make_params(w, h, nc, prec, reversible=rev, ycc=True, promote=promoted, num_resolutions=2)
        got = enc.stage_transform(buf, lambda dev: api.planes_from_layout(dev, lay, nc, depth_bits=d), p)
        _check(got, dc.level1_words(oracle, smp, prec, rev, True), f"fused{what} depth {d} -> {prec} {'53' if rev else '97'} c{nc}")


@PREC
def test_fused_level_1(api, enc, oracle, prec):
    """c: the same frames through stage_transform with one DWT level: 5/3 on three channels with the RCT, 9/7 on four with the
    ICT (alpha takes no part in it).  d < prec runs GEN, d > prec the right shift, d == prec SPEC -- and, a second time under
    fused_generic, the generic kernel with a shift of 0.
    Strips: every frame is 512 columns wide and at least 17 rows high, so each launch has three strips, the second of them
    (columns 244..499) a FAST one -- 16-byte loads of ARGB64 and of ARGB32 pixels, paired stores -- and the first and third
    edge strips: both instantiations of dwt_wave run on every pair.
    What this test cannot see: that stage_transform took the fused kernel at all.  fuse_frontend decides that silently
    (interleaved layout, equal depths, 1, 3 or 4 channels, at least one level -- all true here); a fallback to frontend_kernel
    plus the plain level kernel would give the same words.  test_depth_model.py::test_frames_reach_fast_and_edge_strips holds
    the launch model of dwt_variant_cases, not the library, to both claims."""
    for sample_bits, d in dc.pairs_of(prec):
        ch, buf, lay = _frame(sample_bits, d)
        _fused_level_1(api, enc, oracle, ch, buf, lay, d, prec)
    assert api.get_tune("fused_generic") == 0
    api.tune("fused_generic", 1)
    try:
        for sample_bits, d in dc.pairs_of(prec):
            if d == prec:
                ch, buf, lay = _frame(sample_bits, d)
                _fused_level_1(api, enc, oracle, ch, buf, lay, d, prec, what=" generic")
    finally:
        api.tune("fused_generic", 0)


# ------------------------------------------------------------------------------------------------ d
@PREC
def test_ycc_front_end(api, enc, prec):
    """d: rgb_to_sycc at 4:2:0 against sycc_model.frontend_planes of the converted samples: three channels under 5/3, four (the
    alpha beside Y) under 9/7."""
    sub = (2, 2)
    for sample_bits, d in dc.pairs_of(prec):
        ch, buf, lay = _frame(sample_bits, d)
        _, h, w = ch.shape
        for rev, nc in ((True, 3), (False, 4)):
            smp = dc.samples(ch[:nc], [d] * nc, prec)
            p = api.make_params(w, h, nc, prec, reversible=rev, num_resolutions=1, sub=[(1, 1), sub, sub] + [(1, 1)] * (nc - 3), rgb_to_sycc=True)
            got = enc.stage_frontend(buf, lay, p, depth_bits=d)
            want = sycc_model.frontend_planes(list(smp), prec, sub)
            assert len(got) == nc
            for c in range(nc):
                w32 = np.ascontiguousarray(want[c].astype(np.int32)) if rev else _as_float_words(want[c])
                _check(got[c], w32, f"ycc {sample_bits}-bit depth {d} -> {prec} {'53' if rev else '97'} component {c}")


# ------------------------------------------------------------------------------------------------ e
def _perturbed(smp, prec):
    """Decoded planes: the model's samples with a few off by one and by the whole range 2^prec - 1, in every component."""
    top = (1 << prec) - 1
    dec = smp.copy()
    nc, h, w = dec.shape
    for c in range(nc):
        flat, src = dec[c].reshape(-1), smp[c].reshape(-1)
        zero, full = np.flatnonzero(src == 0), np.flatnonzero(src == top)
        flat[zero[len(zero) // 2]] = top
        flat[full[-1]] = 0
        for k in (3 + c, w + 1, flat.size - 2 - c):  # off by one, towards the inside of the range
            if flat[k] == src[k]:
                flat[k] += 1 if src[k] < top else -1
    assert dec.min() >= 0 and dec.max() <= top
    return dec


def _same(got, want, what):
    assert len(got) == len(want)
    for c, (g, w) in enumerate(zip(got, want)):
        assert g == w, (what, c, g, w)


@PREC
def test_compare_kernel(api, enc, prec):
    """e: stage_compare of four channels of unequal depth against the model's samples -- no sample differs -- and against
    samples a few of which are off by one and by 2^prec - 1: every field as compare_model.diffs has it.  Once over dense
    aligned planes (the `wide` path, four samples per load), once over strided views (one sample per load)."""
    for sample_bits, groups in dc.GROUPS.items():
        dt = dc.dtype_of(sample_bits)
        for ds in groups:
            chans = dc.channels(sample_bits, ds)
            smp = dc.samples(chans, ds, prec)
            _, h, w = smp.shape
            dec = _perturbed(smp, prec)
            p = api.make_params(w, h, 4, prec)
            buf, offs, arrs = dc.dense(list(chans), dt)
            assert all(o % 16 == 0 for o in offs) and all(a.strides == (w * a.itemsize, a.itemsize) for a in arrs) and w % 4 == 0
            store, make = _strided_views(api, chans, dt, ds)
            for name, views in (("dense", (buf, _depths(api, arrs, lambda c: offs[c], ds))), ("strided", (store.reshape(-1).view(np.uint8), make))):
                what = f"compare {name} {sample_bits}-bit depths {ds} -> {prec}"
                got = enc.stage_compare(list(smp), p, views=views)
                assert [g["differing"] for g in got] == [0] * 4, (what, got)
                _same(got, cm.diffs(list(smp), list(smp), prec), what)
                got = enc.stage_compare(list(dec), p, views=views)
                want = cm.diffs(list(smp), list(dec), prec)
                assert all(x["max_abs"] == (1 << prec) - 1 and x["differing"] >= 2 for x in want)
                _same(got, want, what + " perturbed")


# ------------------------------------------------------------------------------------------------ f
def _float_front_end(api, enc, oracle, x, d, prec, promoted=False):
    """x: (4, H, W) float32 channels standing for depth d: strided views (4-byte loads) and an ARGB128 frame (fe_unpack128)."""
    smp = dc.float_samples(x, d, prec, promoted)
    _, h, w = x.shape
    store, views = dc.strided(list(x), np.float32)
    make = _depths(api, views, lambda c: views[c].ctypes.data - store.ctypes.data, [d] * 4)
    buf, lay = dc.interleaved(list(x), 32)
    lay["depth"] = d
    for rev in (True, False):
        p = api.make_params(w, h, 4, prec, reversible=rev, ycc=True, promote=promoted, num_resolutions=1)
        want = dc.frontend_words(oracle, smp, prec, rev, True)
        what = f"float depth {d} -> {prec} {'53' if rev else '97'}{' promote' if promoted else ''}"
        _check(enc.stage_frontend_planes(store, make, p), want, what + " strided")
        _check(enc.stage_frontend(buf, lay, p), want, what + " ARGB128")


@PREC
def test_float_channels(api, enc, oracle, prec):
    """f: float channels standing for depth d = 1..16, every grid point p / (2^d - 1): four channels with the RCT and the ICT."""
    for d, pr in dc.FLOAT_PAIRS:
        if pr == prec:
            _float_front_end(api, enc, oracle, dc.float_channels(d, 4), d, prec)


# ------------------------------------------------------------------------------------------------ g
@PREC
def test_promote(api, enc, oracle, prec):
    """g: promote_ae16 on 16-bit samples of depth 16, every stored value 0..65535 (and on floats of depth 16 holding
    Demote(v) / 32768), through a, b, c and f: Promote, then the conversion 16 -> prec."""
    ch, buf, lay = _frame(16, 16)
    assert np.array_equal(np.sort(ch[0, :-1].reshape(-1)), np.arange(65536))
    _, h, w = ch.shape
    _strided_front_end(api, enc, oracle, ch, 16, (16,) * 4, prec, promoted=True)
    smp = dc.samples(ch, [16] * 4, prec, True)
    for rev in (True, False):
        p = api.make_params(w, h, 4, prec, reversible=rev, ycc=True, promote=True, num_resolutions=1)
        _check(enc.stage_frontend(buf, lay, p, depth_bits=16), dc.frontend_words(oracle, smp, prec, rev, True),
               f"interleaved promote -> {prec} {'53' if rev else '97'}")
    _fused_level_1(api, enc, oracle, ch, buf, lay, 16, prec, promoted=True, what=" promote")
    _float_front_end(api, enc, oracle, dc.float_channels(16, 4, True), 16, prec, promoted=True)
