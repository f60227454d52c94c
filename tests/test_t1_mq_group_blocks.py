"""Two-wave MQ coder, plain instantiation: groups summed by the producer wave, on the GPU.

In t1_mq2_kernel<false> the producer wave sums each group of four decisions into {G, N} and queues it beside the four addends
and shifts (j2k_amd/csrc/t1_mq_window.h); the consumer takes the group in one step, peels, and has the wave code the group
again per decision -- from the addends and shifts, unpacked only then -- if a lane's shifts sum to more than 15 (long), a carry
stands above a 0xFF, or a byte reads 0x00 and a carry crossed its top boundary.  The header's host test
(test_t1_mq_group_host.py) holds that text to Figure C.3; here are the 64 lanes, the LDS queue in its two halves, lanes that end
inside a group and a chunk, and the knob mq_window = 3, under which every lane reports every group long, so that the long
protocol -- G ignored, the group unpacked and coded per decision -- runs at every group.  (test_t1_mq_window_blocks.py runs the
knobs 0, -1 and 2 over the first two families.)

Under the knobs 0 (as shipped) and 3, byte for byte against the CPU oracle's block coder and against t1_mq2_kernel<true> (the
per-decision consumer on the old queue words, which does not read the knob):

  noise   65 blocks of 64 x 64, 16-bit noise: two workgroups, the second with one live lane; one block all zero
  shapes  4 x 4 to 64 x 64, odd sizes, 1 x 1, flat magnitudes, the 22-plane block            (both families as in
          test_t1_mq_window_blocks.py, and their reference shared with it)
  sparse  64 blocks of 64 x 64, zero but for a few isolated large samples: long runs of one context drive it to the small Qe
          of Table C.2, whose less probable symbol shifts by 10 to 15 -- such shifts meet in one group, and N passes 15
  small   64 blocks of every size from 1 x 1 to 8 x 8: lanes end at every position inside a group and a chunk
"""
import numpy as np
import pytest

from j2k_amd import api
from test_t1_mq_window_blocks import _FAMILIES, _reference, _signs

pytestmark = pytest.mark.gpu


def _sparse():
    rng = np.random.default_rng(1564)
    cases = []
    for i in range(64):
        b = np.zeros((64, 64), dtype=np.int64)
        for _ in range(1 + i % 12):
            y, x = (int(v) for v in rng.integers(0, 64, size=2))
            b[y, x] = int(rng.integers(1 << 13, 1 << 15)) * (1 if rng.random() < 0.5 else -1)
        b[int(rng.integers(0, 64)), int(rng.integers(0, 64))] = 1 << 14  # (every block has its top plane)
        cases.append((b, i % 4))
    return cases


def _small():
    rng = np.random.default_rng(88)
    cases = []
    for h in range(1, 9):
        for w in range(1, 9):
            b = rng.integers(0, 1 << 12, size=(h, w)) * _signs(rng, (h, w))
            cases.append((np.asarray(b, dtype=np.int64), (w + h) % 4))
    return cases


# (the two new families join the other file's table, so that one reference per family serves both files)
_FAMILIES.setdefault("sparse", _sparse)
_FAMILIES.setdefault("small", _small)


@pytest.fixture(scope="module")
def enc():
    e = api.Encoder(0)
    before = api.get_tune("mq_window")
    yield e
    api.tune("mq_window", before)
    e.close()


@pytest.mark.parametrize("window", [0, 3], ids=["grouped", "every_group_long"])
@pytest.mark.parametrize("family", ["noise", "shapes", "sparse", "small"])
def test_grouped_coder_writes_the_oracles_codewords(enc, oracle, family, window):
    ref = _reference(oracle, family)
    plane, rects, orients, refs = ref[:4]
    nb = len(rects)
    if family == "noise":
        assert nb == 65 and sum(r["npasses"] == 0 for r in refs) == 1
    elif family == "sparse":
        assert nb == 64 and all(r["npasses"] > 30 for r in refs)
        assert all(len(r["data"]) < 400 for r in refs)  # thousands of decisions in a few hundred bytes: small Qe, large shifts
    elif family == "small":
        assert nb == 64 and sorted((w, h) for _, _, w, h in rects) == [(w, h) for w in range(1, 9) for h in range(1, 9)]
        assert len({len(r["data"]) for r in refs}) > 16
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
