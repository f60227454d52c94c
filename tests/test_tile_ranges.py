"""GPU: the tile-range entry points (j2k_hip_encode_tiles_device, j2k_hip_encode_tiles and, over the latter,
j2k_hip_encode_tiles_distributed) against the CPU oracle's tile-parts.

The cases are those of tests/tile_range_cases.py; tests/test_tile_range_refs.py shows on the CPU that their references hold.  A
range (first, count) must return exactly the oracle's parts[first:first + count]: every contiguous range of the grids of at most
12 tiles, and of the 20-tile grids every single tile, the whole grid and every range of 2, ntx and ntx + 1 tiles -- single
interior tiles (both box origins non-zero), runs inside a row, runs across a row end (a full-width box that holds tiles nobody
asked for) and whole rows.  All ranges of one (configuration, view, entry point) go through ONE handle in a seeded shuffled order
(the geometry cache is keyed on the range); the same handle then encodes the whole frame from host memory, and three of the
ranges are repeated on a fresh handle.  The host entry point gets a frame whose bytes outside the rows of the range's box are
flipped: nothing but those rows may be read.  Every partition of the grid over 1 .. ntiles + 1 ranks reassembles to the whole
file, and so does the distributed call over 2, 3 and 7 handles; the single-tile ranges of A and F run again under the
launch-shape knobs; refused ranges leave the handle exact."""
import ctypes as C

import pytest

import tile_range_cases as tc

pytestmark = pytest.mark.gpu

J2K_HIP_ERR_PARAM = 1


@pytest.fixture(scope="module")
def api():
    from j2k_amd import api
    return api


@pytest.fixture
def enc(api):
    """A handle of the test's own: what one handle has seen is part of what is tested."""
    e = api.Encoder(0)
    yield e
    e.close()


class Frame:
    """One source on one handle: the device copy for the device entry point, poisoned host copies for the host one."""

    def __init__(self, api, e, c, view):
        self.api, self.e, self.c, self.g = api, e, c, c.geo
        self.src = tc.source(c.geo, view)
        self.views = tc.plane_views(api, self.src)
        self.p = tc.api_params(api, c, promote=self.src.promote)
        self.d = e.upload(self.src.buf)
        self._host = {}

    def close(self):
        self.e.free(self.d)

    def device(self, first, count, e=None):
        return tc.tiles_device(self.api, e or self.e, self.views(self.d), self.p, first, count)

    def host(self, first, count, e=None):
        _, y0, _, y1 = tc.box(self.g, first, count)
        if (y0, y1) not in self._host:
            self._host[(y0, y1)] = tc.poisoned(self.g, self.src, y0, y1)
        buf = self._host[(y0, y1)]
        return (e or self.e).encode_tiles_host(self.views(buf.ctypes.data), self.p, first, count)

    def whole(self):
        """The whole frame from (unpoisoned) host memory through j2k_hip_encode_to_buffer."""
        return self.e._encode_planes_host(self.views(self.src.buf.ctypes.data), self.src.buf.nbytes, self.p, False)


def _mismatches(g, parts, got):
    """[(first, count, box kind, box, first differing tile-part)] of the ranges whose bytes are not the oracle's."""
    bad = []
    for (first, count), data in got:
        want = b"".join(parts[first:first + count])
        if data != want:
            pos, where = 0, None
            for t in range(first, first + count):
                if data[pos:pos + len(parts[t])] != parts[t]:
                    where = t
                    break
                pos += len(parts[t])
            bad.append((first, count, tc.box_kind(g, first, count), tc.box(g, first, count), where, len(data), len(want)))
    return bad


# -- every range, every view, both entry points ----------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", tc.ENTRIES)
@pytest.mark.parametrize("cv", tc.PAIRS, ids=tc.pair_id)
def test_ranges_equal_the_oracles_tile_parts(api, enc, oracle, cv, entry):
    c, view = cv
    g = c.geo
    cs, hdr, parts = tc.reference(oracle, c, tc.KIND[view])
    fr = Frame(api, enc, c, view)
    try:
        assert api.main_header(fr.p) == hdr
        order = tc.shuffled_ranges(g, 1000 + len(c.name) + tc.VIEWS.index(view))
        with tc.dv.knobs(fr.src.knobs):
            got = [(r, getattr(fr, entry)(*r)) for r in order]
            bad = _mismatches(g, parts, got)
            assert not bad, f"{len(bad)} of {len(got)} ranges differ (first, count, kind, box, first wrong tile, bytes, expected): {bad[:6]}"
            # the handle that has seen every box encodes the whole frame
            assert fr.whole() == cs
            # ... and a handle that has seen nothing writes the same for three of the ranges
            fresh = api.Encoder(0)
            try:
                again = [(r, getattr(fr, entry)(*r, e=fresh)) for r in (order[0], order[len(order) // 2], order[-1])]
            finally:
                fresh.close()
            assert not _mismatches(g, parts, again)
            assert dict(again) == {r: data for r, data in got if r in dict(again)}
    finally:
        fr.close()


# -- partitions over 1 .. ntiles + 1 ranks ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", tc.ENTRIES)
@pytest.mark.parametrize("c", tc.CONFIGS, ids=lambda c: c.name)
def test_every_partition_reassembles_to_the_whole_file(api, enc, oracle, c, entry):
    from j2k_amd import sharding
    cs, _, parts = tc.reference(oracle, c)
    fr = Frame(api, enc, c, "ae")
    done = {}
    try:
        for world, shares in tc.partitions(c.geo):
            for r in shares:
                if r not in done:
                    done[r] = getattr(fr, entry)(*r)
            assert sharding.assemble(fr.p, [done[r] for r in shares]) == cs, (world, _mismatches(c.geo, parts, [(r, done[r]) for r in shares]))
    finally:
        fr.close()
    assert len(done) >= tc.ntiles(c.geo)


DISTRIBUTED = [(c, v) for c, v in tc.PAIRS if c in tc.BASE and v in ("ae", "ae_bottomup", "planar10_bottomup")]


@pytest.mark.parametrize("ndev", [2, 3, 7])
@pytest.mark.parametrize("cv", DISTRIBUTED, ids=tc.pair_id)
def test_tiles_distributed_writes_the_oracles_file(api, oracle, cv, ndev):
    """j2k_hip_encode_tiles_distributed: one handle and one thread per share, the shares of sharding.partition_tiles, from host
    memory (the box has one device: the list names it ndev times).  7 shares: runs that cross a row end on the 20-tile grids,
    shares of 2 and 1 tiles on B, more devices than tiles on D and E."""
    c, view = cv
    cs, _, _ = tc.reference(oracle, c, tc.KIND[view])
    src = tc.source(c.geo, view)
    p = tc.api_params(api, c, promote=src.promote)
    chunks = []

    @api.WRITE_FN
    def write(user, buf, n):
        chunks.append(C.string_at(buf, n))
        return n
    L = api.load_library()
    devs = (C.c_int * ndev)(*([0] * ndev))
    rc = L.j2k_hip_encode_tiles_distributed(devs, ndev, C.byref(p), tc.plane_views(api, src)(src.buf.ctypes.data), write, None)
    assert rc == 0, L.j2k_hip_multi_last_error()
    assert b"".join(chunks) == cs


# -- launch shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kn", tc.LAUNCH_KNOBS, ids=tc.dv.kid)
@pytest.mark.parametrize("name", tc.LAUNCH_CONFIGS)
def test_single_tiles_under_the_launch_shape_knobs(api, enc, oracle, name, kn):
    """The knobs change how strips and chunks map onto px0 / py0 of a job; no output byte may change."""
    c = tc.BY_NAME[name]
    _, _, parts = tc.reference(oracle, c)
    fr = Frame(api, enc, c, "ae")
    try:
        with tc.dv.knobs(kn):
            got = [(r, fr.device(*r)) for r in tc.single_tiles(c.geo)]
    finally:
        fr.close()
    for k in kn:
        assert api.get_tune(k) == tc.dv.DEFAULTS[k]
    bad = _mismatches(c.geo, parts, got)
    assert not bad, f"{tc.dv.kid(kn)}: {len(bad)} of {len(got)} tiles differ: {bad[:6]}"


# -- bottom-up sources, whole frame ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv", [cv for cv in tc.PAIRS if cv[1].endswith("bottomup")], ids=tc.pair_id)
def test_whole_frame_from_a_bottom_up_source(api, enc, oracle, cv):
    """base = the last row of the buffer, rowbytes negative: through encode_host's entry point and through the device one."""
    c, view = cv
    cs, _, _ = tc.reference(oracle, c, tc.KIND[view])
    fr = Frame(api, enc, c, view)
    try:
        assert all(ch.rowbytes < 0 for ch in fr.src.chans)
        assert fr.whole() == cs
        assert enc._encode_planes_host(fr.views(fr.src.buf.ctypes.data), fr.src.buf.nbytes, fr.p, True) == cs  # (via the sink)
        dptr, n = C.c_void_p(), C.c_size_t()
        enc._check(enc.L.j2k_hip_encode_device(enc.h, C.byref(fr.p), fr.views(fr.d), C.byref(dptr), C.byref(n), None, 0))
        assert enc.d2h(dptr.value, n.value).tobytes() == cs
    finally:
        fr.close()


# -- refusals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", tc.ENTRIES)
@pytest.mark.parametrize("what", tc.BAD_RANGES)
def test_bad_ranges_are_refused_and_leave_the_handle_exact(api, enc, oracle, what, entry):
    c = tc.BY_NAME["B_53_rct"]
    g = c.geo
    _, _, parts = tc.reference(oracle, c)
    first, count = tc.bad_range(g, what)
    fr = Frame(api, enc, c, "ae")
    try:
        assert fr.device(5, 2) == b"".join(parts[5:7])  # (a geometry is cached when the refusal comes)
        with pytest.raises(api.J2kHipError, match="tile range out of bounds") as ei:
            _unboxed(fr, entry, first, count)
        assert ei.value.code == J2K_HIP_ERR_PARAM
        for r in ((5, 2), (6, 1), (3, 6)):
            assert getattr(fr, entry)(*r) == b"".join(parts[r[0]:r[0] + r[1]]), (what, r)
    finally:
        fr.close()


def _unboxed(fr, entry, first, count):
    """A range that has no box: the host frame goes in as it is."""
    if entry == "device":
        return fr.device(first, count)
    return fr.e.encode_tiles_host(fr.views(fr.src.buf.ctypes.data), fr.p, first, count)


def test_poison_outside_the_box_would_change_the_file(api, enc, oracle):
    """The host sweep's guard bites: the same poisoned frame, asked for a tile whose rows ARE flipped, gives other bytes."""
    c = tc.BY_NAME["B_53_rct"]
    _, _, parts = tc.reference(oracle, c)
    fr = Frame(api, enc, c, "ae")
    try:
        buf = tc.poisoned(c.geo, fr.src, 40, 80)  # rows of tile row 1 kept
        assert enc.encode_tiles_host(fr.views(buf.ctypes.data), fr.p, 5, 1) == parts[5]
        assert enc.encode_tiles_host(fr.views(buf.ctypes.data), fr.p, 1, 1) != parts[1]
    finally:
        fr.close()
