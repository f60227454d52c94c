"""Two-wave MQ coder: the instantiation without per-pass byte counts.

A plain frame reads no per-pass byte counts, so its coder is t1_mq2_kernel<false>: the consumer wave keeps none (no pass-end
tests, one copy of its decision loop, no loads of the modeller's per-pass decision counts, no stores of rates).  Rate control
and the stage hook with want_passes take t1_mq2_kernel<true>, the kernel as it was.  Both must write the same codewords.

One launch of 130 blocks -- three coder workgroups, the last with two live lanes -- mixes all-zero blocks (no pass), blocks of
one bit-plane (one pass), 64 x 64 noise blocks of nine planes and a 1 x 1 block; it goes through stage_t1 plain and with
want_passes, against the CPU oracle.  One frame of 512 x 512 RGB16 9/7 is encoded plain and under rate control (ratio 20) on
one handle in either order -- a handle switches between the two instantiations -- against the oracle's codestreams.
"""
import numpy as np
import pytest

from j2k_amd import api, synth
from oracle.oracle import make_params
from t1_families import layout as _layout

pytestmark = pytest.mark.gpu

NBLOCKS = 130
PLANES = 9  # the most the dense families of test_t1_decision_tables.py use


def _blocks():
    rng = np.random.default_rng(130)
    cases = []
    for i in range(NBLOCKS):
        kind = i % 4
        if i == NBLOCKS - 2:
            kind = 2  # the last workgroup's two live lanes: a noise block and the 1 x 1 block
        if i == NBLOCKS - 1:
            b = np.array([[-(1 << (PLANES - 1)) - 5]], dtype=np.int64)
        elif kind == 0:
            b = np.zeros((64, 64), dtype=np.int64)  # no bit-plane, no pass
        elif kind == 1:
            w, h = ((64, 64), (17, 33), (64, 5))[(i // 4) % 3]
            b = (rng.random((h, w)) < 0.3).astype(np.int64) * np.where(rng.random((h, w)) < 0.5, -1, 1)  # one plane: one cleanup pass
        elif kind == 2:
            b = rng.integers(0, 1 << PLANES, size=(64, 64)) * np.where(rng.random((64, 64)) < 0.5, -1, 1)
            b[0, 0] = 1 << (PLANES - 1)
        else:
            w, h = ((63, 64), (64, 30), (33, 47))[(i // 4) % 3]
            b = np.rint(rng.laplace(0, 20, size=(h, w))).astype(np.int64)
        cases.append((b, i % 4))
    return cases


_REF = {}


def _reference(oracle, rev):
    if rev not in _REF:
        coef, rects, orients = _layout(_blocks())
        step = 1.0 if rev else 0.37
        plane = coef.astype(np.int32) if rev else (coef * 0.61).astype(np.float32)
        refs = []
        for (x, y, w, h), o in zip(rects, orients):
            blk = plane[y:y + h, x:x + w]
            if rev:
                data = (blk.astype(np.int64) << 6).astype(np.int32)
            else:
                data = np.array([[oracle.L.j2ko_quant97(float(v), step) for v in row] for row in blk], dtype=np.int32)
            refs.append(oracle.t1_block(data, o))
        _REF[rev] = (plane, rects, orients, step, refs)
    return _REF[rev]


@pytest.fixture(scope="module")
def enc():
    e = api.Encoder(0)
    yield e
    e.close()


@pytest.mark.parametrize("rev", [True, False], ids=["rev", "irr"])
def test_both_instantiations_write_the_oracles_codewords(enc, oracle, rev):
    plane, rects, orients, step, refs = _reference(oracle, rev)
    assert len(rects) == NBLOCKS
    assert any(r["npasses"] == 0 for r in refs) and any(r["npasses"] == 1 for r in refs)
    assert max(r["numbps"] for r in refs) >= PLANES  # (9/7: the scaling by 0.61 / 0.37 adds one)
    assert rects[-1][2:] == (1, 1) and refs[-1]["npasses"] > 0
    plain = enc.stage_t1(plane.copy(), rects, orients, [step] * NBLOCKS, rev)
    rated = enc.stage_t1(plane.copy(), rects, orients, [step] * NBLOCKS, rev, want_passes=True)
    again = enc.stage_t1(plane.copy(), rects, orients, [step] * NBLOCKS, rev)  # (and back: the handle switches both ways)
    for r, o, p, q, a, ref in zip(rects, orients, plain, rated, again, refs):
        for g in (p, q, a):
            assert g["numbps"] == ref["numbps"], (r, o)
            assert g["npasses"] == ref["npasses"], (r, o)
            assert g["length"] == len(ref["data"]), (r, o)
            assert g["data"] == ref["data"], (r, o)
        assert q["rates"] == ref["rates"], (r, o)
        assert q["nmsedec"] == ref["nmsedec"], (r, o)


W = H = 512
_FRAME = {}


def _frame(oracle):
    if not _FRAME:
        pl = synth.planes(W, H, 3, 16, 512, "A")
        _FRAME["plain"] = oracle.encode(pl, make_params(W, H, 3, 16, reversible=False, mct=True, numres=6), comment="x")
        _FRAME["rate"] = oracle.encode_rates(pl, make_params(W, H, 3, 16, reversible=False, mct=True, numres=6, layers=1), [20.0], comment="x")
        _FRAME["frame"], _FRAME["lay"] = synth.ae_frame(pl, 16)
    return _FRAME


@pytest.mark.parametrize("order", [("plain", "rate", "plain"), ("rate", "plain", "rate")], ids=["plain_first", "rate_first"])
def test_a_handle_switches_between_plain_and_rate_controlled_frames(oracle, order):
    f = _frame(oracle)
    assert f["plain"] != f["rate"] and len(f["rate"]) < len(f["plain"])
    e = api.Encoder(0)
    try:
        for what in order:
            p = api.make_params(W, H, 3, 16, reversible=False, ycc=True, num_resolutions=6, comment="x",
                                **({"rates": [20.0]} if what == "rate" else {}))
            assert e.encode_host(f["frame"], f["lay"], p) == f[what], what
    finally:
        e.close()
