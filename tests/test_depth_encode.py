"""Whole encode, decode and compare calls at every file depth 1..16: what lies behind the front end -- the quantiser's exponents
and numbps, Mb, the DC shift at prec = 1, the rate weights, the SIZ / QCD bytes, the decode of such files.

  16 depths x {5/3, 9/7} x {1 channel, 3 with MCT, 4 with MCT} = 96 ids per test function, on 70 x 45 with 3 resolutions
  (depth_cases.planes: a 0 and a 2^prec - 1 in every component), then one tiled geometry and two quality layers by rate at
  a few depths.

Encode: byte for byte against Oracle.encode, from an After Effects frame (samples left-justified in the container as
synth.ae_frame stores them: the fused level-1 kernel's right shift), from planar views of depth == prec in the smallest
container (the stand-alone front end) and from the uploaded frame (encode_device).  These images are narrower than 500
columns, so the fused kernel serves them with edge strips only; its FAST strips at these depths are test_depth_matrix.py's.
Decode: decode_planar of the oracle's stream equals Oracle.decode exactly at the file's depth, at depth 8 and at depth 16
(Oracle.copy_channel_out); a 5/3 file returns the source.
Compare: Encoder.compare of the file against its source frame: a lossless file differs nowhere and has an infinite PSNR, any
other gives the figures of compare_model.diffs on the oracle's decoded planes."""
import functools
import math

import numpy as np
import pytest

import compare_model as cm
import depth_cases as dc
from j2k_amd import synth
from oracle.oracle import make_params

gpu = pytest.mark.gpu

W, H, NUMRES = 70, 45, 3
CHANNELS = [(1, False), (3, True), (4, True)]  # (channels, mct)
WHOLE = [(prec, rev, nc) for prec in dc.PRECS for rev in (True, False) for nc, _ in CHANNELS]
TILED = [(prec, rev) for prec in (1, 5, 9, 13, 15) for rev in (True, False)]  # 97 x 61, tiles of 64, 4 resolutions, RGB with MCT
# Two quality layers by compression ratio, RGB with MCT on 70 x 45: (prec, reversible) -> the two ratios.  Chosen on the CPU
# so that both layers of the oracle's stream carry bytes (test_rate_table_gives_both_layers_bytes holds the table to that):
# the raw image is 70 * 45 * 3 * prec / 8 bytes, a layer's budget is that over its ratio.
RATES = {
#                                                               bytes behind SOD: first layer alone / both layers
    (3, True): [6.0, 3.0],      # 506 / 1099
    (3, False): [8.0, 4.0],     # 352 / 563 (the whole 9/7 file at 3 bits has 546: a smaller ratio leaves the second layer empty)
    (7, True): [6.0, 3.0],      # 1289 / 2641
    (7, False): [6.0, 3.0],     # 1281 / 2607
    (11, True): [4.0, 2.0],     # 3155 / 6343
    (11, False): [4.0, 2.0],    # 3134 / 6408
    (14, True): [3.0, 1.5],     # 5423 / 10846
    (14, False): [3.0, 1.5],    # 5425 / 10857
}


def _id(case):
    return f"prec{case[0]}-{'53' if case[1] else '97'}" + (f"-c{case[2]}" if len(case) > 2 else "")


@pytest.fixture(scope="module")
def api():
    from j2k_amd import api
    return api


@pytest.fixture(scope="module")
def enc(api):
    e = api.Encoder(0)
    yield e
    e.close()


_shared = []


@pytest.fixture(scope="module", autouse=True)
def _session_oracle(oracle):
    """The session's one Oracle (conftest.py), where the cached _file() -- which can take no fixture -- finds it."""
    _shared.append(oracle)
    yield
    _shared.clear()


def _oracle():
    return _shared[0]


@functools.lru_cache(maxsize=None)
def _file(w, h, nc, prec, rev, numres, tile=0, rates=None):
    """(source planes, the oracle's codestream, the oracle's decode of it): computed once, shared, never written to."""
    pl = dc.planes(w, h, nc, prec, 900 + 16 * nc + prec)
    op = make_params(w, h, nc, prec, reversible=rev, mct=nc >= 3, numres=numres, tile=tile, layers=len(rates) if rates else 1)
    cs = _oracle().encode_rates(pl, op, list(rates)) if rates else _oracle().encode(pl, op)
    dec = _oracle().decode(cs)
    pl.setflags(write=False)
    dec.setflags(write=False)
    return pl, cs, dec


def _params(api, w, h, nc, prec, rev, numres, tile=0, rates=None):
    return api.make_params(w, h, nc, prec, reversible=rev, ycc=nc >= 3, num_resolutions=numres, tile_size=tile,
                           rates=list(rates) if rates else None)


def _encodes(api, enc, geo):
    pl, cs, _ = _file(*geo)
    w, h, nc, prec = geo[:4]
    p = _params(api, *geo)
    frame, lay = synth.ae_frame(pl, prec)
    assert lay["sample_bytes"] == (1 if prec <= 8 else 2)
    assert enc.encode_host(frame, lay, p) == cs, "from the After Effects frame"
    assert enc.encode_planar_host(pl, p) == cs, "from planar views of depth == prec"
    d = enc.upload(frame)
    try:
        assert enc.encode_device(d, lay, p)[2] == cs, "from the uploaded frame"
    finally:
        enc.free(d)


def _decodes(enc, geo, lossless):
    pl, cs, dec = _file(*geo)
    w, h, nc, prec = geo[:4]
    assert np.array_equal(enc.decode_planar(cs).astype(np.int32), dec)
    if lossless:
        assert np.array_equal(dec, pl)
    for bits in (8, 16):
        got = enc.decode_planar(cs, sample_bits=bits, depth=bits)
        sb = bits // 8
        for c in range(nc):
            exp = _oracle().copy_channel_out(dec[c], prec, sb, bits, sb, w * sb, w, h).view(np.uint16 if sb == 2 else np.uint8).reshape(h, w)
            assert np.array_equal(got[c], exp), (bits, c)


def _compares(api, enc, geo, lossless):
    pl, cs, dec = _file(*geo)
    w, h, nc, prec = geo[:4]
    frame, lay = synth.ae_frame(pl, prec)
    got = enc.compare(cs, _params(api, *geo), frame=frame, layout=lay)
    want = cm.diffs(list(pl), list(dec), prec)
    assert len(got) == nc
    for c in range(nc):
        assert got[c] == want[c], (c, got[c], want[c])
        if lossless:
            assert got[c]["differing"] == 0 and got[c]["psnr"] == math.inf


@gpu
@pytest.mark.parametrize("case", WHOLE, ids=_id)
def test_encode_equals_the_oracle(api, enc, case):
    prec, rev, nc = case
    _encodes(api, enc, (W, H, nc, prec, rev, NUMRES))


@gpu
@pytest.mark.parametrize("case", WHOLE, ids=_id)
def test_decode_equals_the_oracle(enc, case):
    prec, rev, nc = case
    _decodes(enc, (W, H, nc, prec, rev, NUMRES), lossless=rev)


@gpu
@pytest.mark.parametrize("case", WHOLE, ids=_id)
def test_compare_with_the_source(api, enc, case):
    prec, rev, nc = case
    _compares(api, enc, (W, H, nc, prec, rev, NUMRES), lossless=rev)


@gpu
@pytest.mark.parametrize("case", TILED, ids=_id)
def test_tiled_geometry(api, enc, case):
    """97 x 61 in tiles of 64 (four tiles, three of them cut by the image's edge), 4 resolutions, RGB with MCT."""
    prec, rev = case
    geo = (97, 61, 3, prec, rev, 4, 64)
    _encodes(api, enc, geo)
    _decodes(enc, geo, lossless=rev)
    _compares(api, enc, geo, lossless=rev)


def _body_bytes(cs: bytes) -> int:
    """Bytes behind the SOD marker of the one tile-part of an untiled codestream."""
    sot = cs.index(b"\xff\x90\x00\x0a")
    psot = int.from_bytes(cs[sot + 6:sot + 10], "big")
    assert cs[sot + 12:sot + 14] == b"\xff\x93" and sot + psot + 2 == len(cs)
    return psot - 14


@pytest.mark.parametrize("case", sorted(RATES), ids=_id)
def test_rate_table_gives_both_layers_bytes(case):
    """No GPU: the oracle's two-layer stream against its one-layer stream at the first ratio alone.  A packet without a
    code-block contribution is one byte, and a layer has 3 resolutions x 3 components = 9 packets: the first layer holds well
    over 9 bytes, and the second adds well over 9 more."""
    prec, rev = case
    rates = RATES[case]
    assert rates[0] > rates[1] > 1.0
    pl, two, _ = _file(W, H, 3, prec, rev, NUMRES, 0, tuple(rates))
    one = _oracle().encode_rates(pl, make_params(W, H, 3, prec, reversible=rev, mct=True, numres=NUMRES, layers=1), rates[:1])
    first, both = _body_bytes(one), _body_bytes(two)
    assert first >= 9 + 64, (case, first)
    assert both - first >= 9 + 64, (case, first, both)


@gpu
@pytest.mark.parametrize("case", sorted(RATES), ids=_id)
def test_two_quality_layers_by_rate(api, enc, case):
    prec, rev = case
    geo = (W, H, 3, prec, rev, NUMRES, 0, tuple(RATES[case]))
    _encodes(api, enc, geo)
    _decodes(enc, geo, lossless=False)
    _compares(api, enc, geo, lossless=False)
