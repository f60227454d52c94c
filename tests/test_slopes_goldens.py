"""GPU: the libopenjp2 pin of layers at given slopes (j2k_hip_params.layer_slopes).

A file written with layer_slopes set to the thresholds a layer_rates / layer_psnr encode reports
(j2k_hip_encode_get_layer_slopes) is that encode's file, byte for byte -- and that file is libopenjp2's, committed under
tests/golden/.  For every single-tile rate and quality golden: encode under its rates / targets (the committed bytes), read the
thresholds back, encode the same frame under them through the planar host call, j2k_hip_encode_device, begin / end and a
two-frame j2k_hip_encode_sequence_device (the second frame from another seed: each frame must be its own single-frame slopes
file), with the cut on the device (the default) and on the host (rate_dev = -1).

So that nothing passes vacuously, per golden: at least one threshold is positive, and the oracle's reader
(file_blocks(layers=True): the pieces every block has per layer) finds at least one code-block that a layer with a positive
threshold leaves short of the passes it coded -- fewer passes in the layers up to that one than its bit-planes hold
(3 numbps - 2): the threshold really cut something.  Read per layer because four of the goldens (r4, r6, r8, q3) end in a
layer that takes everything left: over the whole file none of their blocks is short, the cuts are in the layers before.
No golden of the list fails the condition; none was dropped.
"""
import hashlib
import os

import pytest

from conftest import GOLDEN_DIR
from j2k_amd import api, synth

pytestmark = pytest.mark.gpu

NAMES = ["r1_128_grey8_53_r20", "r2_128_grey8_97_r20", "r3_300x200_rgb8_97_ict_r40_20_10", "r4_300x200_rgb8_53_rct_r30_10_0",
         "r6_64_grey8_53_r5_2_1", "r7_97x61_grey12_97_r12_6_3", "r8_300x200_rgba8_53_rct_7layers", "r9_200x150_rgb10_97_cblk32_r25_8",
         "q1_128_grey8_53_q35", "q2_300x200_rgb8_97_ict_q30_38_45", "q3_300x200_rgb8_53_rct_q32_40_0", "q5_239x97_rgba16_97_q43_47"]


def params(g, **how):
    kw = g["params"]
    return api.make_params(g["width"], g["height"], g["ncomp"], g["prec"], reversible=kw.get("reversible", True), ycc=kw.get("mct", False),
                           tile_size=kw.get("tile", 0), num_resolutions=kw.get("numres", 6), cblk=tuple(kw.get("cblk", (64, 64))),
                           comment=g["comment"], **how)


@pytest.fixture(scope="module")
def enc():
    e = api.Encoder(0)
    yield e
    api.tune("rate_dev", 0)
    e.close()


@pytest.mark.parametrize("name", NAMES)
def test_slopes_read_back_write_the_committed_file(enc, oracle, golden, name):
    g = golden[name]
    with open(os.path.join(GOLDEN_DIR, name + ".j2k"), "rb") as fh:
        f = fh.read()
    assert hashlib.sha256(f).hexdigest() == g["sha256"]
    pl = synth.planes(g["width"], g["height"], g["ncomp"], g["prec"], g["seed"], g["dist"])
    pl2 = synth.planes(g["width"], g["height"], g["ncomp"], g["prec"], g["seed"] + 1000, g["dist"])
    frame, lay = synth.ae_frame(pl, g["prec"])
    frame2, _ = synth.ae_frame(pl2, g["prec"])
    searched = params(g, rates=g["rates"]) if "rates" in g else params(g, psnr=g["psnr_targets"])
    assert enc.encode_planar_host(pl, searched) == f
    slopes = enc.layer_slopes(0)
    assert len(slopes) == searched.layers and all(s == s and abs(s) != float("inf") for s in slopes)
    with pytest.raises(api.J2kHipError):
        enc.layer_slopes(1)  # a tile the file does not have
    # the condition: a positive threshold, and a block cut short
    assert any(s > 0 for s in slopes), slopes
    blocks = oracle.file_blocks(f, layers=True)["blocks"]
    assert any(sum(n for lay, _, n in b["pieces"] if lay <= l) < 3 * b["numbps"] - 2 for l, s in enumerate(slopes) if s > 0 for b in blocks), name
    p = params(g, slopes=slopes)
    d1, d2 = enc.upload(frame), enc.upload(frame2)
    try:
        second = None
        for rate_dev in (0, -1):
            api.tune("rate_dev", rate_dev)
            assert enc.encode_planar_host(pl, p) == f, (name, rate_dev, "planar host")
            assert enc.layer_slopes(0) == slopes  # the thresholds it was given
            assert enc.encode_device(d1, lay, p)[2] == f, (name, rate_dev, "device")
            enc.encode_begin_host(frame, lay, p)
            assert enc.encode_end() == f, (name, rate_dev, "begin / end")
            one = enc.encode_device(d2, lay, p)[2]
            assert one != f and (second is None or one == second), (name, rate_dev)  # (both paths write the same second frame)
            second = one
            seq = enc.encode_sequence_device([d1, d2], lay, p)
            assert seq[0][2] == f and seq[1][2] == one, (name, rate_dev, "sequence")
            assert enc.layer_slopes(0) == slopes
    finally:
        api.tune("rate_dev", 0)
        enc.free(d1)
        enc.free(d2)
