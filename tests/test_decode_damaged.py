"""GPU: whole files whose code-block bytes are damaged (tests/golden/damaged, written by tests/golden/make_damaged_golden.py):
six small files of libopenjp2 with SOP and EPH markers, their packet bodies patched by the committed lists of damaged.json
-- single bit flips, 0xFF + a marker byte, 0xFF 0xFF 0xFF, every byte random.  Packet headers and lengths are the clean
file's, so the decoder does the clean file's work on other bytes.  libopenjp2 decodes such files without complaint; the
decode here must deliver its samples: every comparison is exact, against the committed per-component hashes of libopenjp2's
decode (test_t1_dec_damaged_refs.py holds the oracle and the live library to the same hashes) or against oracle.decode."""
import hashlib

import numpy as np
import pytest

import damaged_cases as dm
import layers_cases as lc
from j2k_amd import api

pytestmark = pytest.mark.gpu

CASES = [(n, m) for n in dm.FILE_NAMES for m in dm.FILE_MODES]
IDS = [f"{n[:2]}-{m}" for n, m in CASES]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def enc():
    e = api.Encoder(0)
    yield e
    e.close()


class Knobs:
    """Sets tuning knobs and puts back what they were."""

    def __init__(self, **kw):
        self.kw, self.before = kw, {}

    def __enter__(self):
        for k, v in self.kw.items():
            self.before[k] = api.get_tune(k)
            api.tune(k, v)

    def __exit__(self, *exc):
        for k, v in self.before.items():
            api.tune(k, v)


def check(dec, want, what):
    assert dec.shape[0] == len(want), what
    assert [sha(dec[c].astype(np.int32)) for c in range(dec.shape[0])] == want, what


@pytest.mark.parametrize("name,mode", CASES, ids=IDS)
def test_planar_decode_of_a_damaged_file(enc, name, mode):
    """Either Tier-1 kernel (a styled file takes the lanes whatever the knob says: decoded once), the heaviest blocks moved
    to the wave kernel, and half the size."""
    bad, want = dm.patched(name, mode), dm.hashes(name, mode)
    check(enc.decode_planar(bad), want[0], (name, mode, "default"))
    lanes_seen = []
    for lanes in ([2] if dm.styled(name) else [0, 2]):
        with Knobs(t1dec_lanes=lanes):
            check(enc.decode_planar(bad), want[0], (name, mode, "lanes", lanes))
            lanes_seen.append(enc.decode_kernels())
    (lane_blocks, wave_blocks) = lanes_seen[-1]
    assert lane_blocks > 0
    if not dm.styled(name):
        assert lanes_seen[0][0] == 0 and lanes_seen[0][1] == lane_blocks + wave_blocks
    with Knobs(t1dec_lanes=2, t1dec_tail=2):
        check(enc.decode_planar(bad), want[0], (name, mode, "tail"))
    check(enc.decode_planar(bad, subsample=2), want[1], (name, mode, "subsample 2"))
    check(enc.decode_planar(dm.load(name)), dm.hashes(name)[0], (name, "clean, after the damaged ones"))


@pytest.mark.parametrize("mode", dm.FILE_MODES)
def test_region_across_the_tile_edge_of_a_damaged_file(enc, mode):
    bad = dm.patched(dm.TILED, mode)
    whole = enc.decode_planar(bad)
    check(whole, dm.hashes(dm.TILED, mode)[0], mode)
    x, y, w, h = 41, 9, 50, 37  # columns 41 .. 90: both tiles (the edge is at 64)
    win = enc.decode_region_planar(bad, (x, y, w, h))
    assert np.array_equal(win, whole[:, y:y + h, x:x + w]), mode
    assert not np.array_equal(win, enc.decode_planar(dm.load(dm.TILED))[:, y:y + h, x:x + w]), "the damage does not show in the window"


@pytest.mark.parametrize("mode", dm.FILE_MODES)
def test_layer_limit_on_the_damaged_layered_file(enc, oracle, mode):
    bad = dm.patched(dm.LAYERED, mode)
    try:
        for L in (1, 2):
            enc.set_max_layers(L)
            got = enc.decode_planar(bad)
            assert np.array_equal(got.astype(np.int32), oracle.decode(lc.strip(bad, L))), (mode, L)
    finally:
        enc.set_max_layers(0)
    check(enc.decode_planar(bad), dm.hashes(dm.LAYERED, mode)[0], mode)


@pytest.mark.parametrize("name,mode", CASES, ids=IDS)
def test_damage_does_not_leak_across_the_frames_of_a_sequence(enc, name, mode):
    """[clean, damaged, clean] in one call: the frames share the Tier-1 launches (and a wave of the lane kernel)."""
    clean, bad = dm.load(name), dm.patched(name, mode)
    got = enc.decode_sequence_planar([clean, bad, clean])
    check(got[0], dm.hashes(name)[0], (name, mode, "frame 0"))
    check(got[1], dm.hashes(name, mode)[0], (name, mode, "frame 1"))
    check(got[2], dm.hashes(name)[0], (name, mode, "frame 2"))
