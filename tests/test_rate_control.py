"""Rate control: compression ratios per quality layer with OpenJPEG's tcp_rates /
cp_disto_alloc semantics -- what the reference's CompressionSettings would select if WriteFile copied
them (src/common/j2k_openjpeg_codec.cpp:707).  Oracle and GPU path against codestreams written by
libopenjp2 itself (tests/golden/r*.j2k, made by tests/golden/make_golden.py)."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR
from j2k_amd import api, synth
from oracle.oracle import make_params

RATE = ["r1_128_grey8_53_r20", "r2_128_grey8_97_r20", "r3_300x200_rgb8_97_ict_r40_20_10", "r4_300x200_rgb8_53_rct_r30_10_0",
        "r5_300x200_rgb16_97_ict_tile128_r50_25", "r6_64_grey8_53_r5_2_1", "r7_97x61_grey12_97_r12_6_3",
        "r8_300x200_rgba8_53_rct_7layers", "r9_200x150_rgb10_97_cblk32_r25_8"]


def case(golden, name):
    g = golden[name]
    pl = synth.planes(g["width"], g["height"], g["ncomp"], g["prec"], g["seed"], g["dist"])
    f = open(os.path.join(GOLDEN_DIR, name + ".j2k"), "rb").read()
    assert hashlib.sha256(f).hexdigest() == g["sha256"]
    return g, pl, f


@pytest.mark.parametrize("name", RATE)
def test_oracle_rate_control_matches_golden(oracle, golden, name):
    g, pl, f = case(golden, name)
    p = make_params(g["width"], g["height"], g["ncomp"], g["prec"], layers=len(g["rates"]), **g["params"])
    assert oracle.encode_rates(pl, p, g["rates"], comment=g["comment"]) == f


def test_oracle_rate_control_live_library(oracle, opj):
    """A few more shapes against whichever libopenjp2 is installed."""
    rng = np.random.default_rng(5)
    for t in range(6):
        w, h = int(rng.integers(40, 200)), int(rng.integers(40, 160))
        nc, prec = int(rng.choice([1, 3])), int(rng.choice([8, 12, 16]))
        kw = dict(numres=int(rng.integers(1, 5)), reversible=bool(t & 1), mct=nc == 3, tile=int(rng.choice([0, 64])))
        rates = [30.0, 12.5, 4.0][:int(rng.integers(1, 4))]
        pl = synth.planes(w, h, nc, prec, 100 + t, "B")
        p = make_params(w, h, nc, prec, layers=len(rates), **kw)
        assert oracle.encode_rates(pl, p, rates, comment=opj.comment) == opj.encode_rates(pl, p, rates)


def test_rates_must_decrease():
    p = api.make_params(64, 64, 1, 8, num_resolutions=2, rates=[10.0, 20.0])
    with pytest.raises(api.J2kHipError, match="strictly lesser"):
        api.main_header(p)
    api.main_header(api.make_params(64, 64, 1, 8, num_resolutions=2, rates=[20.0, 10.0, 0.0]))
    api.main_header(api.make_params(64, 64, 1, 8, num_resolutions=2, rates=[0.0, 0.0]))  # both "no limit": accepted like OpenJPEG


def hip_params(g, **extra):
    kw = g["params"]
    return api.make_params(g["width"], g["height"], g["ncomp"], g["prec"], reversible=kw.get("reversible", True),
                           ycc=kw.get("mct", False), tile_size=kw.get("tile", 0), num_resolutions=kw.get("numres", 6),
                           cblk=tuple(kw.get("cblk", (64, 64))), comment=g["comment"], rates=g["rates"], **extra)


# ------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", RATE)
def test_gpu_rate_control_matches_golden(golden, name):
    g, pl, f = case(golden, name)
    enc = api.Encoder(0)
    p = hip_params(g)
    if g["ncomp"] in (3, 4):
        frame, lay = synth.ae_frame(pl, g["prec"])
        got = enc.encode_host(frame, lay, p)
        d = enc.upload(frame)
        _, _, dev = enc.encode_device(d, lay, p)
        assert dev == f
    else:
        got = enc.encode_planar_host(pl, p)
    enc.close()
    assert got == f


@pytest.mark.gpu
@pytest.mark.parametrize("scan", [1, 100])
@pytest.mark.parametrize("name", RATE)
def test_gpu_rate_control_with_the_per_block_work_on_the_device_matches_golden(golden, name, scan):
    """rate.hip: distortions, slope ranges, the bound walk and the scans of the rounds with at least `scan` open blocks run
    on the device right behind the coder (by default only for frames of 8192 blocks and more); libopenjp2's bytes."""
    g, pl, f = case(golden, name)
    enc = api.Encoder(0)
    p = hip_params(g)
    try:
        api.tune("rate_dev", 1)
        api.tune("rate_dev_scan", scan)
        if g["ncomp"] in (3, 4):
            frame, lay = synth.ae_frame(pl, g["prec"])
            got = enc.encode_host(frame, lay, p)
        else:
            got = enc.encode_planar_host(pl, p)
        assert got == f
    finally:
        api.tune("rate_dev", 0)
        api.tune("rate_dev_scan", 0)
        enc.close()


@pytest.mark.gpu
def test_gpu_rate_control_with_two_coder_groups_matches_libopenjp2(golden):
    """Rate control on a frame big enough for two coder groups, under five thread / device settings of the layer
    allocation: 4096^2 RGB16 9/7, ratio 20, against libopenjp2's file (hash)."""
    name = "rh1_4096_rgb16_97_r20"
    if name not in golden:
        pytest.skip("full-size golden not generated")
    g = golden[name]
    pl = synth.planes(g["width"], g["height"], g["ncomp"], g["prec"], g["seed"], g["dist"])
    frame, lay = synth.ae_frame(pl, g["prec"])
    del pl
    enc = api.Encoder(0)
    try:
        # the host allocation cuts its scans and packet walks across this many threads; 12288 blocks: the per-block work is on
        # the device by default (rate_dev -1: all of it on the host; rate_dev_scan 1: every scan on the device)
        for threads, rate_dev, scan in ((8, 0, 0), (1, 0, 0), (3, -1, 0), (8, 0, 1), (2, -1, 0)):
            api.tune("alloc_threads", threads)
            api.tune("rate_dev", rate_dev)
            api.tune("rate_dev_scan", scan)
            got = enc.encode_host(frame, lay, hip_params(g))
            st = enc.stats()
            assert st["num_codeblocks"] >= 8192
            assert len(got) == g["length"]
            assert hashlib.sha256(got).hexdigest() == g["sha256"], (threads, rate_dev, scan)
    finally:
        api.tune("alloc_threads", 8)
        api.tune("rate_dev", 0)
        api.tune("rate_dev_scan", 0)
        enc.close()


@pytest.mark.gpu
def test_gpu_rate_control_four_layers_on_the_device_equal_the_oracle(oracle):
    """A frame of 9228 blocks (the layer allocation's per-block work runs on the device by default) cut into four layers: the
    later layers start from the passes of the ones before (RateDevice::begin_layer), their candidates are priced on top of
    committed layers.  Bytes against the oracle (~10 s of CPU)."""
    w, h = 4096, 3072
    pl = synth.planes(w, h, 3, 16, 77, "A")
    rates = [100.0, 30.0, 10.0, 4.0]
    ref = oracle.encode_rates(pl, make_params(w, h, 3, 16, reversible=False, mct=True, numres=6, layers=len(rates)), rates, comment="x")
    frame, lay = synth.ae_frame(pl, 16)
    del pl
    enc = api.Encoder(0)
    try:
        got = enc.encode_host(frame, lay, api.make_params(w, h, 3, 16, reversible=False, ycc=True, num_resolutions=6, comment="x", rates=rates))
        assert enc.stats()["num_codeblocks"] >= 8192
        assert got == ref
    finally:
        enc.close()


@pytest.mark.gpu
def test_gpu_rate_control_tile_sharded_equals_whole(golden):
    from j2k_amd import sharding
    g, pl, f = case(golden, "r5_300x200_rgb16_97_ict_tile128_r50_25")
    frame, lay = synth.ae_frame(pl, g["prec"])
    enc = api.Encoder(0)
    d = enc.upload(frame)
    p = hip_params(g)
    parts = [enc.encode_tiles_device(d, lay, p, t, 1) for t in range(6)]
    enc.close()
    assert sharding.assemble(p, parts) == f


@pytest.mark.gpu
def test_gpu_rate_control_sizes_and_quality_are_monotone(opj):
    """Property at a size no fixture covers: tighter ratios give smaller streams and lower PSNR, every
    stream decodes, and the achieved size respects the budget of the last layer."""
    w, h = 1024, 768
    pl = synth.planes(w, h, 3, 8, 321, "B")
    frame, lay = synth.ae_frame(pl, 8)
    enc = api.Encoder(0)
    raw = w * h * 3
    sizes, psnrs = [], []
    for ratio in (8.0, 16.0, 40.0):
        p = api.make_params(w, h, 3, 8, reversible=False, ycc=True, rates=[ratio * 4, ratio * 2, ratio], comment="")
        cs = enc.encode_host(frame, lay, p)
        assert len(cs) <= raw / ratio + 16  # OpenJPEG leaves SOT, SOD and EOC (16 bytes) out of the budget
        dec = opj.decode(cs)
        mse = np.mean((dec.astype(np.float64) - pl) ** 2)
        sizes.append(len(cs)); psnrs.append(10 * np.log10(255 ** 2 / mse))
    enc.close()
    assert sizes[0] > sizes[1] > sizes[2] and psnrs[0] > psnrs[1] > psnrs[2]


def _jr_case(golden):
    name = "jr1_300x200_rgba8_jp2_srgb_alpha_r30_8"
    g = golden[name]
    pl = synth.planes(g["width"], g["height"], g["ncomp"], g["prec"], g["seed"], g["dist"])
    f = open(os.path.join(GOLDEN_DIR, name + ".jp2"), "rb").read()
    assert hashlib.sha256(f).hexdigest() == g["sha256"]
    return g, pl, f


def test_oracle_jp2_with_rate_control_matches_golden(oracle, golden):
    """The JP2 boxes in front of the codestream are charged to the byte budget (opj_stream_tell at the
    time OpenJPEG fixes the rates)."""
    g, pl, f = _jr_case(golden)
    p = make_params(g["width"], g["height"], g["ncomp"], g["prec"], layers=len(g["rates"]), **g["params"])
    k = f.index(b"jp2c") + 4
    cs = oracle.encode_rates(pl, p, g["rates"], comment=g["comment"], prefix_len=k)
    assert oracle.jp2_wrap(cs, p, g["color_space"], None, g["alpha_channel"]) == f


@pytest.mark.gpu
def test_gpu_jp2_with_rate_control_matches_golden(golden):
    g, pl, f = _jr_case(golden)
    frame, lay = synth.ae_frame(pl, g["prec"])
    enc = api.Encoder(0)
    got = enc.encode_host(frame, lay, hip_params(g, jp2=True, color_space=g["color_space"], alpha_channel=g["alpha_channel"]))
    enc.close()
    assert got == f


@pytest.mark.gpu
def test_hip_codec_file_size_target(opj, monkeypatch):
    """HipCodec::HonourSettings: settings.method == SIZE turns settings.fileSize (KiB) into layer ratios; the file
    written through the Codec interface meets the size, decodes, and equals the C ABI call with those ratios."""
    import ctypes as C
    api.load_library()
    H = C.CDLL(os.path.join(os.path.dirname(api.LIBPATH), "libj2k_host.so"))
    H.j2k_host_test_write.restype = C.c_long
    H.j2k_host_test_write.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_int, C.c_long, C.c_void_p, C.c_ulong, C.c_char_p, C.c_ulong]
    w, h, kb, layers = 640, 480, 40, 3
    pl = synth.planes(w, h, 3, 8, 99, "B")
    frame, lay = synth.ae_frame(pl, 8)
    out = np.empty(1 << 22, dtype=np.uint8)
    err = C.create_string_buffer(512)
    monkeypatch.setenv("J2K_HOST_TEST_FILESIZE_KB", str(kb))
    n = H.j2k_host_test_write(frame.ctypes.data, w, h, lay["rowbytes"], lay["sample_bytes"], 3, 8, 0, 1, layers, 0, 1, -1,
                              out.ctypes.data, out.nbytes, err, 512)
    assert n > 0, err.value
    got = out[:n].tobytes()
    assert kb * 1024 * 0.9 < len(got) <= kb * 1024 + 16
    assert opj.decode(got).shape == pl.shape
    ratio = w * h * 3 / (kb * 1024.0)
    enc = api.Encoder(0)
    p = api.make_params(w, h, 3, 8, reversible=False, ycc=True, comment=None, rates=[ratio * 4, ratio * 2, ratio])
    assert enc.encode_host(frame, lay, p) == got
    enc.close()


# ------------------------------------------------------------------------------------ fixed quality
QUALITY = ["q1_128_grey8_53_q35", "q2_300x200_rgb8_97_ict_q30_38_45", "q3_300x200_rgb8_53_rct_q32_40_0",
           "q4_300x200_rgb16_97_ict_tile128_q40_60", "q5_239x97_rgba16_97_q43_47"]


@pytest.mark.parametrize("name", QUALITY)
def test_oracle_fixed_quality_matches_golden(oracle, golden, name):
    """PSNR targets per layer (OpenJPEG cp_fixed_quality / tcp_distoratio)."""
    g, pl, f = case(golden, name)
    p = make_params(g["width"], g["height"], g["ncomp"], g["prec"], layers=len(g["psnr_targets"]), **g["params"])
    assert oracle.encode_psnr(pl, p, g["psnr_targets"], comment=g["comment"]) == f


def test_rates_and_psnr_exclude_each_other():
    p = api.make_params(64, 64, 1, 8, num_resolutions=2, rates=[10.0], psnr=[40.0])
    with pytest.raises(api.J2kHipError, match="exclude"):
        api.main_header(p)


@pytest.mark.gpu
@pytest.mark.parametrize("name", QUALITY)
def test_gpu_fixed_quality_matches_golden(golden, name):
    g, pl, f = case(golden, name)
    kw = g["params"]
    p = api.make_params(g["width"], g["height"], g["ncomp"], g["prec"], reversible=kw.get("reversible", True),
                        ycc=kw.get("mct", False), tile_size=kw.get("tile", 0), num_resolutions=kw.get("numres", 6),
                        comment=g["comment"], psnr=g["psnr_targets"])
    enc = api.Encoder(0)
    if g["ncomp"] in (3, 4):
        frame, lay = synth.ae_frame(pl, g["prec"])
        got = enc.encode_host(frame, lay, p)
    else:
        got = enc.encode_planar_host(pl, p)
    enc.close()
    assert got == f


@pytest.mark.gpu
def test_hip_codec_cinema_method_and_resolution_box(monkeypatch, oracle):
    """settings.method == CINEMA (src/aftereffects/j2k.cpp:817-830: fileSize = one frame's budget in KiB): the DCI coding
    style (9/7, one layer, CPRL, 32 x 32 blocks, 6 resolutions for 2K, precincts 128 / 256) cut to the budget -- equal to
    the same parameters through the C ABI; frames beyond 4096 x 2160 are lossless (:639-646).  With format JP2 and a pixel
    aspect the file carries a resolution box and still decodes to the same samples."""
    api.load_library()
    H = C.CDLL(os.path.join(os.path.dirname(api.LIBPATH), "libj2k_host.so"))
    H.j2k_host_test_write.restype = C.c_long
    H.j2k_host_test_write.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_int, C.c_long, C.c_void_p, C.c_ulong, C.c_char_p, C.c_ulong]
    H.j2k_host_test_write_ex.restype = C.c_long
    H.j2k_host_test_write_ex.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_long] + [C.c_int] * 8 + [C.c_long, C.c_int, C.c_int,
                                         C.c_char_p, C.c_ulong, C.c_int, C.c_void_p, C.c_ulong, C.c_char_p, C.c_ulong]
    w, h, kb = 1024, 540, 60
    pl = synth.planes(w, h, 3, 12, 99, "A")
    frame, lay = synth.ae_frame(pl, 12)
    out = np.empty(frame.nbytes, dtype=np.uint8)
    err = C.create_string_buffer(512)
    monkeypatch.setenv("J2K_HOST_TEST_FILESIZE_KB", str(kb))
    monkeypatch.setenv("J2K_HOST_TEST_CINEMA", "2")
    n = H.j2k_host_test_write(frame.ctypes.data, w, h, lay["rowbytes"], lay["sample_bytes"], 3, 12, 1, 0, 12, 0, 1, -1,
                              out.ctypes.data, out.nbytes, err, 512)
    assert n > 0, err.value
    got = out[:n].tobytes()
    assert kb * 1024 * 0.9 < len(got) <= kb * 1024 + 16
    cod = got.index(b"\xff\x52")
    assert got[cod + 5] == 4 and got[cod + 6:cod + 8] == b"\x00\x01"   # CPRL, one layer
    assert got[cod + 9] == 5 and got[cod + 10:cod + 12] == b"\x03\x03" and got[cod + 13] == 0  # 5 levels, 32 x 32 blocks, 9/7
    assert got[cod + 4] == 1 and got[cod + 14:cod + 20] == b"\x77\x88\x88\x88\x88\x88"        # DCI precincts: 128 x 128, then 256 x 256
    # three 12-bit channels inside the 2K container: the real profile -- Rsiz 3, a TLM segment, a tile-part per component
    assert got[6:8] == b"\x00\x03" and b"\xff\x55" in got[:200] and got.count(b"\xff\x90\x00\x0a\x00\x00") == 3
    enc = api.Encoder(0)
    p = api.make_params(w, h, 3, 12, num_resolutions=6, dci_profile=3, max_cs_size=kb * 1024, comment=None)
    assert enc.encode_host(frame, lay, p) == got
    # the 4K profile on the same frame: Rsiz 4, seven resolutions, the progression order change, six tile-parts
    monkeypatch.setenv("J2K_HOST_TEST_CINEMA", "4")
    n = H.j2k_host_test_write(frame.ctypes.data, w, h, lay["rowbytes"], lay["sample_bytes"], 3, 12, 1, 0, 12, 0, 1, -1,
                              out.ctypes.data, out.nbytes, err, 512)
    assert n > 0, err.value
    got4 = out[:n].tobytes()
    assert got4[6:8] == b"\x00\x04" and b"\xff\x5f" in got4[:220] and got4.count(b"\xff\x90\x00\x0a\x00\x00") == 6
    assert got4 == enc.encode_host(frame, lay, api.make_params(w, h, 3, 12, num_resolutions=7, dci_profile=4, max_cs_size=kb * 1024, comment=None))
    # 16-bit channels cannot carry the profile: the same coding style without the flag (Rsiz 0, one tile-part), cut to the budget
    pl16 = synth.planes(w, h, 3, 16, 98, "A")
    f16, l16 = synth.ae_frame(pl16, 16)
    monkeypatch.setenv("J2K_HOST_TEST_CINEMA", "2")
    n = H.j2k_host_test_write(f16.ctypes.data, w, h, l16["rowbytes"], l16["sample_bytes"], 3, 16, 1, 0, 12, 0, 1, -1,
                              out.ctypes.data, out.nbytes, err, 512)
    assert n > 0, err.value
    got16 = out[:n].tobytes()
    assert got16[6:8] == b"\x00\x00" and got16.count(b"\xff\x90\x00\x0a\x00\x00") == 1 and len(got16) <= kb * 1024 + 16
    ratio = w * h * 3 * 16 / 8.0 / (kb * 1024.0)
    p = api.make_params(w, h, 3, 16, reversible=False, ycc=False, num_resolutions=6, cblk=(32, 32), progression=4, rates=[ratio], comment=None,
                        precincts=[(256, 256)] * 5 + [(128, 128)])
    assert enc.encode_host(f16, l16, p) == got16
    # (CPRL over several precincts per resolution: beyond the plain-C restatement's decoder -- libopenjp2 itself is the checker)
    try:
        from oracle.oracle import OpjReplay
        ref = OpjReplay().decode_ex(got)[0]
    except OSError:
        ref = None
    if ref is not None:
        assert np.array_equal(enc.decode_planar(got).astype(np.int32), ref)
    # a frame beyond the DCI container: lossless, the method's budget is not applied
    w2, h2 = 4100, 64
    pl2 = synth.planes(w2, h2, 3, 8, 5, "B")
    f2, l2 = synth.ae_frame(pl2, 8)
    out2 = np.empty(f2.nbytes * 2, dtype=np.uint8)
    n = H.j2k_host_test_write(f2.ctypes.data, w2, h2, l2["rowbytes"], l2["sample_bytes"], 3, 8, 0, 0, 1, 0, 1, -1, out2.ctypes.data, out2.nbytes, err, 512)
    assert n > 0, err.value
    assert np.array_equal(enc.decode_planar(out2[:n].tobytes()), pl2)
    # JP2 with non-square pixels: resolution box present, samples unchanged
    monkeypatch.delenv("J2K_HOST_TEST_CINEMA")
    monkeypatch.delenv("J2K_HOST_TEST_FILESIZE_KB")
    monkeypatch.setenv("J2K_HOST_TEST_ASPECT", "10:11")
    out3 = np.empty(f2.nbytes * 2, dtype=np.uint8)
    n = H.j2k_host_test_write_ex(f2.ctypes.data, w2, h2, l2["rowbytes"], l2["sample_bytes"], 3, 8, 1, 1, 1, 0, 1, -1, 2, 1, None, 0, -1,
                                 out3.ctypes.data, out3.nbytes, err, 512)
    assert n > 0, err.value
    jp2 = out3[:n].tobytes()
    assert b"res " in jp2[:200] and b"resc" in jp2[:200]
    assert np.array_equal(enc.decode_planar(jp2), pl2)
    assert np.array_equal(oracle.decode(jp2), pl2)
    enc.close()


# ------------------------------------------------------------------------------------------------ digital cinema profiles (Rsiz 3 / 4)
DCI_CASES = [("d1_512x270_rgb12_cinema2k", 3, 0, 0), ("d2_1024x540_rgb12_cinema4k_poc", 4, 0, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,profile,max_cs,max_comp", DCI_CASES)
def test_cinema_profiles_equal_the_committed_libopenjp2_files(golden, name, profile, max_cs, max_comp):
    """dci_profile = 3 / 4 on small frames whose budgets do not bind: Rsiz, COD with the 128 / 256 precincts, no comment, TLM,
    the 4K progression order change, a tile-part per component -- the bytes of libopenjp2 2.4.0's own cinema files."""
    g = golden[name]
    want = open(os.path.join(GOLDEN_DIR, "ext", name + ".j2k"), "rb").read()
    pl = synth.planes(g["width"], g["height"], 3, 12, g["seed"], "B")
    frame, lay = synth.ae_frame(pl, 12)
    e = api.Encoder(0)
    try:
        p = api.make_params(g["width"], g["height"], 3, 12, num_resolutions=g["ext"]["numres"], dci_profile=profile, max_cs_size=max_cs, max_comp_size=max_comp,
                            comment="")  # (the committed files have their COM segment, with the library's version in it, taken out)
        got = e.encode_host(frame, lay, p)
        assert got[:200] == want[:200]
        assert got == want
        assert np.array_equal(e.decode_planar(got), e.decode_planar(want))
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,profile,numres,max_cs,max_comp", [(1024, 540, 3, 6, 90000, 0), (1024, 540, 3, 5, 120000, 30000), (2048, 858, 4, 7, 400000, 0),
                                                                (1998, 1080, 4, 7, 300000, 90000), (640, 360, 3, 6, 25000, 9000),
                                                                (4096, 2160, 4, 7, 0, 0), (2048, 1080, 3, 6, 0, 0)])  # (full containers, DCI's own limits)
def test_cinema_profiles_with_binding_budgets_equal_libopenjp2(opj, w, h, profile, numres, max_cs, max_comp):
    """The frame budget (max_cs_size) and the cap per component (max_comp_size) of the cinema profiles: the allocation
    libopenjp2 arrives at for the same limits (its tile-part overhead and main header come off the budget; a candidate
    layer is too large when its packets exceed the budget or one component's packets exceed the cap)."""
    if not opj.version.startswith("2.4"):
        pytest.skip("the cinema profiles are pinned to libopenjp2 2.4 (2.5 writes other limits and markers)")
    pl = synth.planes(w, h, 3, 12, 4000 + w, "A")
    want = opj.encode_ext([pl[0], pl[1], pl[2]], x1=w, y1=h, prec=12, reversible=False, mct=True, numres=numres, rsiz=profile, max_cs_size=max_cs,
                          max_comp_size=max_comp, threads=8)
    frame, lay = synth.ae_frame(pl, 12)
    e = api.Encoder(0)
    try:
        got = e.encode_host(frame, lay, api.make_params(w, h, 3, 12, num_resolutions=numres, dci_profile=profile, max_cs_size=max_cs, max_comp_size=max_comp,
                                                        comment=opj.comment))
        assert len(got) == len(want), (len(got), len(want))
        assert got == want
        assert len(got) <= (max_cs or 1302083) + 16  # (the first tile-part's SOT + SOD and the EOC are not in libopenjp2's accounting: it may overshoot by 16 bytes)
    finally:
        e.close()


@pytest.mark.gpu
def test_cinema_profile_through_the_other_entry_points():
    """The cinema profiles through the frame-sequence call (every frame its own TLM and tile-parts), inside a JP2 wrapper and
    through j2k_hip_encode_begin / _end; the tile-sharded entry points refuse them."""
    w, h = 640, 360
    frames = []
    for k in range(3):
        pl = synth.planes(w, h, 3, 12, 700 + k, "A")
        frames.append(synth.ae_frame(pl, 12))
    lay = frames[0][1]
    e = api.Encoder(0)
    try:
        p = api.make_params(w, h, 3, 12, num_resolutions=6, dci_profile=3, max_cs_size=40000, comment="")
        singles = [e.encode_host(f, lay, p) for f, _ in frames]
        ds = [e.upload(f) for f, _ in frames]
        seq = e.encode_sequence_device(ds, lay, p)
        assert [cs for _, _, cs in seq] == singles
        for d in ds:
            e.free(d)
        e.encode_begin_host(frames[1][0], lay, p)
        assert e.encode_end() == singles[1]
        pj = api.make_params(w, h, 3, 12, num_resolutions=6, dci_profile=3, max_cs_size=40000, comment="", jp2=True, color_space=1)  # J2K_HIP_CS_SRGB
        jp2 = e.encode_host(frames[0][0], lay, pj)
        # (the boxes in front of the codestream come off the budget like the main header does: not the raw file's bytes, the same profile)
        cs = jp2[jp2.index(b"jp2c") + 4:]
        assert jp2[4:8] == b"jP  " and cs[:2] == b"\xff\x4f" and cs[6:8] == b"\x00\x03" and cs.count(b"\xff\x90\x00\x0a\x00\x00") == 3 and cs.endswith(b"\xff\xd9")
        tlm = cs.index(b"\xff\x55")
        sot = cs.index(b"\xff\x90")
        for k in range(3):
            psot = int.from_bytes(cs[sot + 6:sot + 10], "big")
            assert int.from_bytes(cs[tlm + 7 + 5 * k:tlm + 11 + 5 * k], "big") == psot and cs[sot + 10] == k
            sot += psot
        a, b = e.decode_planar(jp2).astype(np.int64), e.decode_planar(singles[0]).astype(np.int64)
        assert a.shape == b.shape and np.abs(a - b).mean() < 2.0  # (a few blocks are cut one pass earlier: the same picture)
        d = e.upload(frames[0][0])
        with pytest.raises(api.J2kHipError, match="one tile"):
            e.encode_tiles_device(d, lay, p, 0, 1)
        e.free(d)
    finally:
        e.close()
