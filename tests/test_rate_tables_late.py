"""GPU: tiled frames through the device side of the rate control (rate.hip), with the allocation's host threads.

With the per-block work on the device, encode_begin sends the Tier-1 pass tables to the host on a side stream and the
allocation asks for them (RateDevice::need_tables) before its first look.  A frame of several small tiles and 2048 blocks or
more has its tiles dealt whole to the allocation's threads; the allocation then does not use the device, and it still has to
ask for the tables, because it reads them at once.  No other test takes that path: the tiled rate-control golden has too few
blocks for more than one thread, and the big rate-controlled frames are single tiles.

What this file is and is not.  The deterministic detector of a read before need_tables() is the host program
tests/native/host_sanitize.cpp (tests/test_host_sanitize.py), which hands the allocation decoy tables until it asks.  On a
GPU the copy is lost or won by microseconds, so these tests need not fail when the call is missing; encoding a decoy frame
of the same geometry first only makes a lost race visible, since the handle's pinned buffer then holds another frame's rows.
They are here so that tiled rate control has actually run through the device path with threads, under every setting of the
knobs that choose the path, and written the oracle's bytes.  One pass over the settings is the test: nothing is repeated."""
import itertools

import pytest

from j2k_amd import api, synth
from oracle.oracle import make_params

pytestmark = pytest.mark.gpu

W = H = 256
KNOBS = ("rate_dev", "overlap", "alloc_threads", "rate_dev_scan")
# name: reversible, rates, tile
FRAMES = {
    "97_ict_two_layers": (False, [40.0, 10.0], 128),
    "53_rct_three_layers": (True, [40.0, 10.0, 0.0], 128),
    "97_ict_two_layers_untiled": (False, [40.0, 10.0], 0),
}
TILED = [n for n in FRAMES if FRAMES[n][2]]

_WANT = {}


def _planes(seed):
    return synth.planes(W, H, 3, 8, seed, "A")


def _want(oracle, name):
    """The CPU oracle's file of the target frame: made once, shared."""
    if name not in _WANT:
        rev, rates, tile = FRAMES[name]
        p = make_params(W, H, 3, 8, reversible=rev, mct=True, numres=4, cblk=(8, 8), layers=len(rates), tile=tile)
        _WANT[name] = oracle.encode_rates(_planes(501), p, rates, comment="x")
    return _WANT[name]


def _params(name):
    rev, rates, tile = FRAMES[name]
    return api.make_params(W, H, 3, 8, reversible=rev, ycc=True, num_resolutions=4, tile_size=tile, cblk=(8, 8), comment="x", rates=rates)


class _Knobs:
    """The knobs' values as found, put back on the way out."""

    def __enter__(self):
        self.before = {k: api.get_tune(k) for k in KNOBS}
        return self

    def __exit__(self, *exc):
        for k, v in self.before.items():
            api.tune(k, v)


@pytest.mark.parametrize("name", TILED)
def test_tiled_rate_control_under_every_allocation_setting_equals_the_oracle(oracle, name):
    """3072 blocks of 8 x 8 in four tiles.  rate_dev 1 puts the per-block work on the device (-1: all on the host), overlap 1
    sends the tables down on the side stream, alloc_threads 8 deals the tiles to threads (1: one thread, which keeps the
    device), rate_dev_scan 1 scans every round on the device (0: rounds of 512 open blocks and more)."""
    want = _want(oracle, name)
    p = _params(name)
    target, lay = synth.ae_frame(_planes(501), 8)
    decoy, _ = synth.ae_frame(_planes(502), 8)
    enc = api.Encoder(0)
    try:
        with _Knobs():
            api.tune("rate_dev", 1)
            api.tune("overlap", 1)
            api.tune("alloc_threads", 8)
            api.tune("rate_dev_scan", 0)
            assert enc.encode_host(decoy, lay, p) != want  # (the pinned table buffer now holds the decoy's rows)
            for rate_dev, overlap, threads, scan in itertools.product((1, -1), (1, 0), (8, 1), (0, 1)):
                api.tune("rate_dev", rate_dev)
                api.tune("overlap", overlap)
                api.tune("alloc_threads", threads)
                api.tune("rate_dev_scan", scan)
                got = enc.encode_host(target, lay, p)
                assert enc.stats()["num_codeblocks"] >= 2048
                assert got == want, (rate_dev, overlap, threads, scan)
    finally:
        enc.close()


@pytest.mark.parametrize("name", list(FRAMES))
def test_rate_control_on_the_device_through_the_other_entry_points_equals_the_oracle(oracle, name):
    """rate_dev 1, overlap 1, alloc_threads 8: begin / end, and a frame that is on the device already -- each after a decoy
    frame through the same entry point.  The untiled frame keeps the device with several layers on a small frame."""
    want = _want(oracle, name)
    p = _params(name)
    target, lay = synth.ae_frame(_planes(501), 8)
    decoy, _ = synth.ae_frame(_planes(502), 8)
    enc = api.Encoder(0)
    try:
        with _Knobs():
            api.tune("rate_dev", 1)
            api.tune("overlap", 1)
            api.tune("alloc_threads", 8)
            api.tune("rate_dev_scan", 0)
            assert enc.encode_host(decoy, lay, p) != want
            assert enc.encode_host(target, lay, p) == want
            assert enc.stats()["num_codeblocks"] >= 2048
            enc.encode_begin_host(decoy, lay, p)
            assert enc.encode_end() != want
            enc.encode_begin_host(target, lay, p)
            assert enc.encode_end() == want
            d, d2 = enc.upload(target), enc.upload(decoy)
            try:
                assert enc.encode_device(d2, lay, p)[2] != want
                assert enc.encode_device(d, lay, p)[2] == want
            finally:
                enc.free(d)
                enc.free(d2)
    finally:
        enc.close()
