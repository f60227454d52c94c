"""Two-wave MQ coder, plain instantiation: the consumer's wide code register on the GPU.

t1_mq2_kernel<false> carries (C, CT, B) as one number from group to group of four decisions (j2k_amd/csrc/t1_mq_window.h),
peels finished bytes after the group, and codes a group again per decision when a lane reports that the wide form is not
exact for it.  t1_mq2_kernel<true> -- rate control, the stage hook with want_passes -- keeps the per-decision consumer and is
the independent implementation on the device; the CPU oracle's block coder is the reference.  What the header's host test
(test_t1_mq_window_host.py) cannot see is here: 64 lanes of unequal length voting on one path, the zero-filled tail past a
lane's end going through accumulate and peel, the LDS stage and its flush, a workgroup with a single live lane.

Both instantiations, byte for byte against each other and the oracle, under the knob mq_window = 0 (as shipped), -1 (every
group per decision) and 2 (every group accumulated, sent back and coded per decision: both state conversions at every group):

  noise   65 blocks of 64 x 64, 16-bit noise -- two workgroups, the second with one live lane -- one of them all zero (no
          pass).  About 3.7 M decisions: by the rates of the host test, thousands of groups in which some lane reports.
  shapes  4 x 4 and 32 x 32 blocks; 64 x 64 of one large magnitude (long runs of more probable symbols: small Qe, large
          shifts); odd sizes; and 64 x 64 noise of 22 bit-planes, about the longest codeword the oracle's block buffer (16 KiB) takes:
          some 12 KiB, the stage's 64-byte flush runs two hundred times.  (A codeword beyond 64 KiB does not exist: a
          code-block has at most 4096 samples.)
"""
import numpy as np
import pytest

from j2k_amd import api
from t1_families import layout as _layout

pytestmark = pytest.mark.gpu


def _signs(rng, shape):
    return np.where(rng.random(shape) < 0.5, -1, 1)


def _noise():
    rng = np.random.default_rng(65)
    cases = []
    for i in range(65):
        if i == 37:
            b = np.zeros((64, 64), dtype=np.int64)  # no bit-plane, no pass: a lane without a decision among full ones
        else:
            b = rng.integers(0, 1 << 16, size=(64, 64)) * _signs(rng, (64, 64))
            b[0, 0] = 1 << 15
        cases.append((b, i % 4))
    return cases


def _shapes():
    rng = np.random.default_rng(4432)
    cases = []
    for w, h in ((4, 4), (32, 32), (4, 4), (33, 47), (1, 1), (64, 5)):
        cases.append(rng.integers(0, 1 << 12, size=(h, w)) * _signs(rng, (h, w)))
    cases.append(np.full((64, 64), (1 << 15) + (1 << 14)) * _signs(rng, (64, 64)))
    cases.append(np.full((64, 64), (1 << 13) - 1, dtype=np.int64))
    cases.append(np.full((32, 32), 1 << 10, dtype=np.int64))
    big = rng.integers(0, 1 << 22, size=(64, 64)) * _signs(rng, (64, 64))
    big[0, 0] = 1 << 21
    cases.append(big)
    return [(np.asarray(b, dtype=np.int64), i % 4) for i, b in enumerate(cases)]


_FAMILIES = {"noise": _noise, "shapes": _shapes}
_REF = {}


def _reference(oracle, family):
    if family not in _REF:
        coef, rects, orients = _layout(_FAMILIES[family]())
        plane = coef.astype(np.int32)
        refs = []
        for (x, y, w, h), o in zip(rects, orients):
            refs.append(oracle.t1_block((plane[y:y + h, x:x + w].astype(np.int64) << 6).astype(np.int32), o))
        rated = None
        _REF[family] = [plane, rects, orients, refs, rated]
    return _REF[family]


@pytest.fixture(scope="module")
def enc():
    e = api.Encoder(0)
    before = api.get_tune("mq_window")
    yield e
    api.tune("mq_window", before)
    e.close()


@pytest.mark.parametrize("window", [0, -1, 2], ids=["wide", "per_decision", "sent_back"])
@pytest.mark.parametrize("family", ["noise", "shapes"])
def test_plain_coder_writes_the_oracles_codewords(enc, oracle, family, window):
    ref = _reference(oracle, family)
    plane, rects, orients, refs = ref[:4]
    nb = len(rects)
    if family == "noise":
        assert nb == 65 and sum(r["npasses"] == 0 for r in refs) == 1
        assert len({len(r["data"]) for r in refs}) > 16  # lanes of unequal length
    else:
        assert max(len(r["data"]) for r in refs) > 11_000  # the 24-plane block
        assert min(len(r["data"]) for r in refs if r["npasses"]) < 64  # ... beside blocks that never fill a flush unit
    before = api.get_tune("mq_window")
    api.tune("mq_window", window)
    try:
        assert api.get_tune("mq_window") == window
        plain = enc.stage_t1(plane.copy(), rects, orients, [1.0] * nb, True)
        if ref[4] is None:  # the <true> kernel does not read the knob: once per family
            ref[4] = enc.stage_t1(plane.copy(), rects, orients, [1.0] * nb, True, want_passes=True)
        rated = ref[4]
    finally:
        api.tune("mq_window", before)
    for r, o, p, q, want in zip(rects, orients, plain, rated, refs):
        for g in (p, q):
            assert g["numbps"] == want["numbps"], (r, o)
            assert g["npasses"] == want["npasses"], (r, o)
            assert g["length"] == len(want["data"]), (r, o)
            assert g["data"] == want["data"], (r, o)
        assert p["length"] == q["length"] and p["data"] == q["data"], (r, o)
        assert q["rates"] == want["rates"], (r, o)
