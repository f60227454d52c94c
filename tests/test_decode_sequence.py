"""GPU: the frames of an image sequence decoded in one call (include/j2k_hip.h: j2k_hip_decode_sequence*), their code-blocks
sharing the gather, Tier-1, inverse DWT and output launches.

References.  An uncut committed file is held to its committed libopenjp2 hash (golden.json: decoded_sha256,
decoded_reduced_sha256, decoded_comps; styles_dec.json).  Cut copies and frames encoded here are held to the CPU oracle's
decode (oracle.decode) where it reads the file; the oracle reads neither sub-sampled nor signed components nor image / tile
origin offsets, so the cut copies of those three ext/ files are held to the single-frame call on a fresh handle, which the
existing tests pin.  Every case holds at least one frame to a libopenjp2 hash or to the oracle.  Exact equality throughout."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import rgba_cases as rc
from conftest import GOLDEN_DIR
from j2k_amd import api, synth
from test_read_fallback import _with_coc

pytestmark = pytest.mark.gpu

GUARD = 0xA5
J2K_HIP_ERR_PARAM, J2K_HIP_ERR_UNSUPPORTED = 1, 6


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def load(rel):
    with open(os.path.join(GOLDEN_DIR, rel), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def enc():
    e = api.Encoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def styles_dec():
    with open(os.path.join(GOLDEN_DIR, "styles_dec", "styles_dec.json")) as f:
        return json.load(f)


@pytest.fixture
def knobs():
    """Sets tuning knobs for one test and puts back what they were."""
    before = {}

    def tune(key, value):
        before.setdefault(key, api.get_tune(key))
        api.tune(key, value)
    yield tune
    for k, v in before.items():
        api.tune(k, v)


def cut(data: bytes, frac: float) -> bytes:
    """The first `frac` of a codestream.  A cut that would fall into the first bytes of a tile-part (its SOT segment: a
    reader refuses a file that ends inside one, libopenjp2 included) is moved behind them."""
    at = int(len(data) * frac)
    pos = 2
    while int.from_bytes(data[pos:pos + 2], "big") != 0xFF90:  # the main header's segments
        pos += 2 + int.from_bytes(data[pos + 2:pos + 4], "big")
    while pos + 12 <= len(data) and data[pos:pos + 2] == b"\xff\x90":
        psot = int.from_bytes(data[pos + 6:pos + 10], "big") or len(data) - pos
        if pos <= at < pos + 32:
            at = pos + min(32, psot)
        pos += psot
    return data[:at]


def cut_jp2(data: bytes, frac: float) -> bytes:
    """A JP2 file whose codestream box is cut short: the box is made to reach the end of the file (LBox = 0)."""
    k = data.index(b"jp2c")
    out = bytearray(data[:k + 4 + int((len(data) - k - 4) * frac)])
    out[k - 4:k] = bytes(4)
    return bytes(out)


def single(data, subsample=1, region=None):
    """The single-frame call on a fresh handle."""
    e = api.Encoder(0)
    try:
        if region is not None:
            return e.decode_region_planar(data, region, subsample=subsample), e.stats()
        return e.decode_planar(data, subsample=subsample), e.stats()
    finally:
        e.close()


def params_of(g):
    kw = g["params"]
    return api.make_params(g["width"], g["height"], g["ncomp"], g["prec"], reversible=kw.get("reversible", True), ycc=kw.get("mct", False),
                           layers=kw.get("layers", 1), tile_size=kw.get("tile", 0), num_resolutions=kw.get("numres", 6),
                           cblk=tuple(kw.get("cblk", (64, 64))), comment="")  # (tests/test_gpu_parity.py: the goldens' own bytes)


def encoded_like(enc, g, planes):
    """A frame of golden g's geometry and coding parameters with other samples, encoded here."""
    frame, lay = synth.ae_frame(planes, g["prec"])
    return enc.encode_host(frame, lay, params_of(g))


_frames = {}


def frames_like(enc, golden, name, seeds):
    """[the golden file] + one frame encoded here per seed, with the golden's parameters (cached: encoded once)."""
    key = (name, tuple(seeds))
    if key not in _frames:
        g = golden[name]
        out = [load(name + ".j2k")]
        for s in seeds:
            out.append(encoded_like(enc, g, synth.planes(g["width"], g["height"], g["ncomp"], g["prec"], s, "AB"[s & 1])))
        _frames[key] = out
    return _frames[key]


_oracle_cache = {}


def oracle_ref(oracle, data, red=0):
    key = (hashlib.sha256(data).hexdigest(), red)
    if key not in _oracle_cache:
        _oracle_cache[key] = oracle.decode(data, red)
    return _oracle_cache[key]


def check_golden_hash(golden, name, dec, red=0):
    g = golden[name]
    want = g["decoded_sha256"] if red == 0 else g["decoded_reduced_sha256"][str(red)]
    assert sha(dec.astype(np.int32)) == want, (name, red)


def check_comp_hashes(comps, dec, info):
    """dec (channels, h, w) against the committed per-component hashes of libopenjp2's samples: a sub-sampled component is
    replicated onto the channel's grid and a signed one offset by 2^(depth-1) on the way out."""
    for c, exp in enumerate(comps[:dec.shape[0]]):
        dx, dy = exp.get("dx", 1), exp.get("dy", 1)
        own = dec[c][::dy, ::dx].astype(np.int32)
        if exp.get("sgnd"):
            own = own - (1 << (exp["prec"] - 1))
        assert list(own.shape) == exp["shape"] and sha(own) == exp["sha256"], c
        assert np.array_equal(dec[c], np.repeat(np.repeat(dec[c][::dy, ::dx], dy, axis=0), dx, axis=1)[:dec.shape[1], :dec.shape[2]])


# ------------------------------------------------------------------------------------------------ 1: several frames in one wave
@pytest.mark.parametrize("lanes,tail", [(0, 1), (2, 1), (2, 2)], ids=["waves", "lanes", "lanes-tail2"])
def test_several_frames_in_one_wave(enc, oracle, golden, knobs, lanes, tail):
    """About 13 blocks per frame: the blocks of all frames fit one wave of the lane kernel.  One frame holds no block at all
    (constant mid-grey: zero after the level shift), one is an all-zero image (its LL band alone holds something)."""
    name = "g9_97x61_grey12_97_4lvl"
    g = golden[name]
    key = (name, "flat")
    if key not in _frames:
        flat = [np.full((1, g["height"], g["width"]), v, dtype=np.int32) for v in (1 << (g["prec"] - 1), 0)]
        _frames[key] = frames_like(enc, golden, name, [31]) + [encoded_like(enc, g, p) for p in flat]
    files = _frames[key]
    knobs("t1dec_lanes", lanes)
    knobs("t1dec_tail", tail)
    got = enc.decode_sequence_planar(files)
    st = enc.stats()
    check_golden_hash(golden, name, got[0])
    for f in range(1, 4):
        assert np.array_equal(got[f].astype(np.int32), oracle_ref(oracle, files[f])), f
    assert (got[2] == 1 << (g["prec"] - 1)).all()
    blocks = [single(d)[1]["num_codeblocks"] for d in files]
    assert blocks[2] == 0 and 0 < sum(blocks) <= 64 and st["num_codeblocks"] == sum(blocks)
    assert st["codestream_bytes"] == sum(len(d) for d in files)
    red = enc.decode_sequence_planar(files, subsample=2)
    check_golden_hash(golden, name, red[0], 1)
    for f in range(1, 4):
        assert np.array_equal(red[f].astype(np.int32), oracle_ref(oracle, files[f], 1)), f


# ------------------------------------------------------------------------------------------------ 2: waves that straddle frames
@pytest.mark.parametrize("name,seeds", [("g3_300x200_rgb8_53_rct", [41]), ("g4_300x200_rgb16_53_rct_tile128", [42, 43])], ids=["g3x2", "g4x3"])
@pytest.mark.parametrize("lanes", [1, 2], ids=["default", "lanes"])
def test_waves_straddle_frames(enc, oracle, golden, knobs, name, seeds, lanes):
    files = frames_like(enc, golden, name, seeds)
    assert single(files[0])[1]["num_codeblocks"] > 64
    knobs("t1dec_lanes", lanes)
    got = enc.decode_sequence_planar(files)
    check_golden_hash(golden, name, got[0])
    for f in range(1, len(files)):
        assert np.array_equal(got[f].astype(np.int32), oracle_ref(oracle, files[f])), f
    assert not np.array_equal(got[0], got[1])
    back = enc.decode_sequence_planar(files[::-1])
    assert np.array_equal(back, got[::-1])
    dev = enc.decode_sequence_planar(files, device=True)
    assert np.array_equal(dev, got)


# ------------------------------------------------------------------------------------------------ 3: styles
STYLED = [("styles_dec", "z1_97x61_grey16_53_vcausal"), ("styles_dec", "z5_128_grey16_53_vcausal_bypass_3layers"),
          ("ext", "s2_300x200_rgb8_97_reset_vcausal_segsym"), ("ext", "u7_128_grey8_53_bypass_termall")]


@pytest.mark.parametrize("sub,name", STYLED, ids=[n for _, n in STYLED])
def test_styled_frames_whole_and_cut(enc, oracle, golden, styles_dec, sub, name):
    data = load(os.path.join(sub, name + ".j2k"))
    files = [data, cut(data, 0.7), cut(data, 0.35)]
    got = enc.decode_sequence_planar(files)
    comps = styles_dec[name]["decoded_comps"] if sub == "styles_dec" else golden[name]["decoded_comps"]["0"]
    check_comp_hashes(comps, got[0], api.read_info(data))
    for f in (1, 2):
        assert np.array_equal(got[f].astype(np.int32), oracle_ref(oracle, files[f])), f
    assert not np.array_equal(got[0], got[2])


# ------------------------------------------------------------------------------------------------ 4: ext/ features
EXT = [("u1_300x200_ycc420_8_53", False), ("u5_97x61_grey12_signed_53", False), ("u6_200x150_rgb8_53_offset", False),
       ("u3_300x200_rgb8_53_precincts_rpcl", True)]


@pytest.mark.parametrize("name,oracle_reads", EXT, ids=[n for n, _ in EXT])
@pytest.mark.parametrize("subsample", [1, 2])
def test_ext_features_whole_and_cut(enc, oracle, golden, name, oracle_reads, subsample):
    """4:2:0 components, a signed component, image and tile origin offsets, RPCL with precincts."""
    data = load(os.path.join("ext", name + ".j2k"))
    files = [data, cut(data, 0.7), cut(data, 0.35)]
    red = subsample.bit_length() - 1
    got = enc.decode_sequence_planar(files, subsample=subsample)
    check_comp_hashes(golden[name]["decoded_comps"][str(red)], got[0], api.read_info(data))
    for f in (1, 2):
        if oracle_reads:
            assert np.array_equal(got[f].astype(np.int32), oracle_ref(oracle, files[f], red)), f
        else:
            assert np.array_equal(got[f], single(files[f], subsample)[0]), f
    if subsample == 1:  # (the frames are told apart at full size: at half size a cut may have cost only the top resolution, which is not decoded)
        assert not np.array_equal(got[0], got[2])


# ------------------------------------------------------------------------------------------------ 5: region
@pytest.mark.parametrize("name,seeds", [("g3_300x200_rgb8_53_rct", [41]), ("g4_300x200_rgb16_53_rct_tile128", [42, 43])], ids=["g3x2", "g4x3"])
@pytest.mark.parametrize("subsample", [1, 2])
def test_region(enc, oracle, golden, name, seeds, subsample):
    files = frames_like(enc, golden, name, seeds)
    red = subsample.bit_length() - 1
    for x, y, w, h in ((120 >> red, 120 >> red, 20, 17), (77, 63, 1, 1)):  # across the tile edge at 128 (64 at half size); a single pixel
        got = enc.decode_sequence_planar(files, subsample=subsample, region=(x, y, w, h))
        st = enc.stats()
        blocks = 0
        for f, d in enumerate(files):
            assert np.array_equal(got[f].astype(np.int32), oracle_ref(oracle, d, red)[:, y:y + h, x:x + w]), (f, x, y)
            one, s1 = single(d, subsample, (x, y, w, h))
            assert np.array_equal(one, got[f])
            blocks += s1["num_codeblocks"]
        assert st["num_codeblocks"] == blocks
    check_golden_hash(golden, name, enc.decode_sequence_planar(files[:1], subsample=subsample,
                                                                 region=(0, 0, -(-golden[name]["width"] >> red), -(-golden[name]["height"] >> red)))[0], red)


# ------------------------------------------------------------------------------------------------ 6: RGBA
RGBA_FILES = ["j3", "j6", "j5", "pal"]  # RGB + A, grey + A, sYCC, the crafted palette


def rgba_frames(name):
    data = rc.load(name)
    return [data, cut_jp2(data, 0.7)]


def oracle_comps(oracle, data):
    i = api.read_info(data)
    dec = oracle_ref(oracle, data)
    return [dict(data=dec[c].astype(np.int64), prec=i["comp_depth"][c] or i["depth"], sgnd=0, dx=1, dy=1) for c in range(dec.shape[0])]


@pytest.fixture(scope="module")
def rgba_table():
    with open(os.path.join(GOLDEN_DIR, "rgba", "rgba.json")) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("name", RGBA_FILES)
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_rgba_into_argb64_frames_with_demote(enc, oracle, rgba_table, name, device):
    files = rgba_frames(name)
    case = rc._case(name, 16, demote=True)
    w, h = rc.image_size(case)
    blank, lay = rc.blank_frame(case)
    frames = np.stack([blank, blank])
    got = enc.decode_rgba_sequence(files, frames, lay, w, h, depth=16, demote=True, device=device)
    assert rc.sha(got[0]) == rgba_table[case["id"]]
    for f in (0, 1):
        assert np.array_equal(got[f], rc.expected_from_comps(case, oracle_comps(oracle, files[f]))), f
    assert not np.array_equal(got[0], got[1])


@pytest.mark.parametrize("name", RGBA_FILES)
def test_rgba_into_planar_channels_and_without_alpha(enc, oracle, rgba_table, name):
    files = rgba_frames(name)
    case = rc._case(name, 8)
    w, h = rc.image_size(case)
    lay = rc.blank_frame(case)[1]
    want = [rc.expected_from_comps(case, oracle_comps(oracle, d)) for d in files]  # A,R,G,B frames of 8-bit samples
    assert rc.sha(want[0]) == rgba_table[case["id"]]
    for alpha in (True, False):
        buf = np.full((2, 4, h + 2, w + 5), GUARD, dtype=np.uint8)  # both frames' channels in one buffer, guards around each
        chans = [[buf[f, 0, 1:h + 1, 2:w + 2], buf[f, 1, h:0:-1, 2:w + 2], buf[f, 2, 1:h + 1, 2:w + 2], buf[f, 3, 1:h + 1, 2:w + 2] if alpha else None]
                 for f in (0, 1)]
        enc.decode_rgba_sequence_channels(files, chans, depth=8)
        for f in (0, 1):
            px = np.lib.stride_tricks.as_strided(want[f], shape=(h, w, 4), strides=(lay["rowbytes"], 4, 1))  # A,R,G,B per pixel
            assert np.array_equal(chans[f][0], px[:, :, 1]) and np.array_equal(chans[f][1], px[:, :, 2]) and np.array_equal(chans[f][2], px[:, :, 3])
            if alpha:
                assert np.array_equal(chans[f][3], px[:, :, 0])
        inner = np.zeros(buf.shape, dtype=bool)
        inner[:, :4 if alpha else 3, 1:h + 1, 2:w + 2] = True
        assert (buf[~inner] == GUARD).all()


# ------------------------------------------------------------------------------------------------ 7: destination layouts
def test_destination_layouts(enc, oracle, golden):
    name = "g3_300x200_rgb8_53_rct"
    files = frames_like(enc, golden, name, [41])
    w, h = golden[name]["width"], golden[name]["height"]
    ref = [oracle_ref(oracle, d) for d in files]
    # all frames into slices of one buffer, larger than the frames: guards to the right of and below every channel
    for device in (False, True):
        out = np.full((2, 3, h + 3, w + 7), GUARD, dtype=np.uint8)
        enc.decode_sequence_planar(files, out=out, device=device)
        check_golden_hash(golden, name, out[0, :, :h, :w])
        for f in (0, 1):
            assert np.array_equal(out[f, :, :h, :w].astype(np.int32), ref[f])
        assert (out[:, :, h:, :] == GUARD).all() and (out[:, :, :, w:] == GUARD).all()
    # row padding, bottom-up rows, 16-bit channels at depth 8
    pad = np.full((2, 3, h, w + 9), GUARD, dtype=np.uint16)
    chans = [[pad[f, 0, :, :w], pad[f, 1, ::-1, :w], pad[f, 2, :, 4:w + 4]] for f in (0, 1)]
    enc.decode_sequence_channels(files, chans, depth=8)
    for f in (0, 1):
        assert np.array_equal(pad[f, 0, :, :w], ref[f][0]) and np.array_equal(pad[f, 1, ::-1, :w], ref[f][1]) and np.array_equal(pad[f, 2, :, 4:w + 4], ref[f][2])
    assert (pad[:, :2, :, w:] == GUARD).all() and (pad[:, 2, :, :4] == GUARD).all() and (pad[:, 2, :, w + 4:] == GUARD).all()
    # After Effects frames (A,R,G,B interleaved, row padding): R, G, B decoded, the A samples and the padding keep their bytes
    pl = synth.planes(w, h, 3, 8, golden[name]["seed"], golden[name]["dist"])
    blank, lay = synth.ae_frame(pl, 8, row_pad_bytes=12)
    frames = np.full((2,) + blank.shape, GUARD, dtype=blank.dtype)
    rb = lay["rowbytes"]
    order = [lay["channel_offsets"][k] for k in (1, 2, 3)]
    chans = [[np.ndarray((h, w), np.uint8, frames[f], order[c], (rb, lay["colbytes"])) for c in range(3)] for f in (0, 1)]
    enc.decode_sequence_channels(files, chans)
    for f in (0, 1):
        px = np.lib.stride_tricks.as_strided(frames[f], shape=(h, w, 4), strides=(rb, 4, 1))
        for c in range(3):
            assert np.array_equal(px[:, :, order[c]].astype(np.int32), ref[f][c])
        assert (px[:, :, lay["channel_offsets"][0]] == GUARD).all()
        assert (np.lib.stride_tricks.as_strided(frames[f][4 * w:], shape=(h, 12), strides=(rb, 1)) == GUARD).all()


# ------------------------------------------------------------------------------------------------ 8: groups
def first_sot(data: bytes) -> int:
    pos = 2
    while int.from_bytes(data[pos:pos + 2], "big") != 0xFF90:
        pos += 2 + int.from_bytes(data[pos + 2:pos + 4], "big")
    return pos


def test_groups(enc, oracle, golden, knobs):
    name = "g9_150x130_rgb8_97_tile64"
    files = frames_like(enc, golden, name, [51, 52, 53, 54])
    outs = []
    for cap in (1, 2, 0):
        knobs("decseq_group", cap)
        outs.append(enc.decode_sequence_planar(files))
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    check_golden_hash(golden, name, outs[0][0])
    for f in range(1, 5):
        assert np.array_equal(outs[0][f].astype(np.int32), oracle_ref(oracle, files[f])), f
    # frame 4 malformed in its packets' tile-part (the first SOT names a tile the image does not have), its main header intact
    bad = bytearray(files[4])
    k = first_sot(files[4])
    bad[k + 4:k + 6] = (999).to_bytes(2, "big")
    bad = bytes(bad)
    assert api.read_info(bad)["width"] == golden[name]["width"]
    api.sequence_check(files[:4] + [bad])
    with pytest.raises(api.J2kHipError) as e1:
        single(bad)
    knobs("decseq_group", 2)
    out = np.full_like(outs[0], GUARD)
    with pytest.raises(api.J2kHipError) as ei:
        enc.decode_sequence_planar(files[:4] + [bad], out=out)
    assert ei.value.code == e1.value.code == J2K_HIP_ERR_PARAM and "frame 4: " in str(ei.value)
    assert np.array_equal(out[:4], outs[0][:4]) and (out[4] == GUARD).all()
    assert np.array_equal(enc.decode_sequence_planar(files), outs[0])  # the handle is intact


# ------------------------------------------------------------------------------------------------ 9: handle reuse
def test_handle_reuse(oracle, golden):
    e = api.Encoder(0)
    try:
        a = frames_like(e, golden, "g4_300x200_rgb16_53_rct_tile128", [42, 43])
        b = frames_like(e, golden, "g9_97x61_grey12_97_4lvl", [31])
        ref_a = [oracle_ref(oracle, d) for d in a]
        first = e.decode_sequence_planar(a)
        for f in range(3):
            assert np.array_equal(first[f].astype(np.int32), ref_a[f])
        check_golden_hash(golden, "g4_300x200_rgb16_53_rct_tile128", first[0])
        one = e.decode_sequence_planar(a[1:2])
        assert np.array_equal(one[0].astype(np.int32), ref_a[1])
        two = e.decode_sequence_planar(b)
        check_golden_hash(golden, "g9_97x61_grey12_97_4lvl", two[0])
        assert np.array_equal(two[1].astype(np.int32), oracle_ref(oracle, b[1]))
        check_golden_hash(golden, "g3_300x200_rgb8_53_rct", e.decode_planar(load("g3_300x200_rgb8_53_rct.j2k")))
        g = golden["g3_300x200_rgb8_53_rct"]
        frame, lay = synth.ae_frame(synth.planes(g["width"], g["height"], g["ncomp"], g["prec"], g["seed"], g["dist"]), g["prec"])
        assert e.encode_host(frame, lay, params_of(g)) == load("g3_300x200_rgb8_53_rct.j2k")
        assert np.array_equal(e.decode_sequence_planar(a), first)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 10: refusals
def test_refusals_leave_the_destinations_untouched(enc, golden):
    g3, g4 = load("g3_300x200_rgb8_53_rct.j2k"), load("g4_300x200_rgb16_53_rct_tile128.j2k")
    before = enc.decode_sequence_planar([g3, g3])

    def refused(code, frame, files, **kw):
        out = np.full((len(files), 3) + kw.pop("shape", (200, 300)), GUARD, dtype=np.uint8)
        with pytest.raises(api.J2kHipError) as ei:
            enc.decode_sequence_planar(files, out=out, sample_bits=8, depth=8, **kw)
        assert ei.value.code == code and str(ei.value).split(": ", 1)[1].startswith(f"frame {frame}: "), str(ei.value)
        assert (out == GUARD).all()

    refused(J2K_HIP_ERR_PARAM, 1, [g3, g4])                                    # another geometry
    refused(J2K_HIP_ERR_PARAM, 2, [g3, g3, g3[:60]])                            # a main header cut short
    refused(J2K_HIP_ERR_UNSUPPORTED, 1, [g3, _with_coc(g3, (1,), -1), g3])      # a frame for the fallback reader
    refused(J2K_HIP_ERR_PARAM, 0, [g3, g3], region=(290, 0, 20, 20), shape=(20, 20))  # a region that leaves the image
    refused(J2K_HIP_ERR_PARAM, 0, [g3, g3], region=(0, 0, 0, 4), shape=(4, 4))
    refused(J2K_HIP_ERR_PARAM, 0, [g3, g3], subsample=1 << 9)                   # more resolutions dropped than the file has
    # a bad destination: a NULL channel in frame 1, a depth that does not fit in frame 1, channels of unlike depth between frames
    out = np.full((2, 3, 200, 300), GUARD, dtype=np.uint8)
    fa, _keep = api._seq_files([g3, g3])
    for breakage in ("base", "depth", "unlike"):
        arr = (api.OutPlane * 6)()
        for k in range(6):
            api._set_outplane(arr[k], out.ctypes.data + k * 200 * 300, 1, 300, 8, 8, 300, 200)
        if breakage == "base":
            arr[4].base = None
        elif breakage == "depth":
            arr[5].depth = 9
        else:
            arr[3].depth = 7
        assert enc.L.j2k_hip_decode_sequence(enc.h, fa, 2, 1, None, arr, 3) == J2K_HIP_ERR_PARAM
        assert enc.L.j2k_hip_last_error(enc.h).decode().startswith("frame 1: ") and (out == GUARD).all()
    assert enc.L.j2k_hip_decode_sequence(enc.h, fa, 0, 1, None, arr, 3) == J2K_HIP_ERR_PARAM
    assert enc.L.j2k_hip_last_error(enc.h).decode().startswith("frame 0: ")
    # RGBA: a file the fused path does not take (CMYK), frames of unlike colour space
    case = rc._case("j1", 8)
    blank, lay = rc.blank_frame(rc._case("j7", 8))
    frames = np.stack([blank, blank])
    with pytest.raises(api.J2kHipError) as ei:
        enc.decode_rgba_sequence([rc.load("j7"), rc.load("j7")], frames, lay, 40, 30, depth=8)
    assert ei.value.code == J2K_HIP_ERR_UNSUPPORTED and "frame 0: " in str(ei.value) and (frames == rc.FILL).all()
    blank, lay = rc.blank_frame(case)
    frames = np.stack([blank, blank])
    with pytest.raises(api.J2kHipError) as ei:
        enc.decode_rgba_sequence([rc.load("j1"), rc.load("j5")], frames, lay, 64, 48, depth=8)  # sRGB beside sYCC (and 5/3 beside 9/7)
    assert ei.value.code == J2K_HIP_ERR_PARAM and "frame 1: " in str(ei.value) and (frames == rc.FILL).all()
    assert np.array_equal(enc.decode_sequence_planar([g3, g3]), before)


# ------------------------------------------------------------------------------------------------ 11: HipCodec::ReadFiles
def test_hip_codec_read_files(oracle):
    from test_read_fallback import _host, _read
    H = _host()
    H.j2k_host_test_read_files.restype = C.c_long
    H.j2k_host_test_read_files.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_ulong), C.c_uint, C.c_uint, C.c_void_p, C.c_uint, C.c_uint, C.c_int,
                                           C.c_char_p, C.c_ulong]
    g3 = load("g3_300x200_rgb8_53_rct.j2k")
    w, h, nc = 300, 200, 3

    def read_files(files):
        bufs = [np.frombuffer(d, dtype=np.uint8) for d in files]
        ptrs = (C.c_void_p * len(files))(*[b.ctypes.data for b in bufs])
        lens = (C.c_ulong * len(files))(*[len(d) for d in files])
        frames = np.full((len(files), nc * w * h), GUARD, dtype=np.uint8)
        err = C.create_string_buffer(512)
        return H.j2k_host_test_read_files(ptrs, lens, len(files), 1, frames.ctypes.data, w, h, nc, err, 512), frames, err.value.decode()

    files = [g3, cut(g3, 0.7), cut(g3, 0.35)]
    rcode, frames, err = read_files(files)
    assert rcode == 1, err
    for f, d in enumerate(files):
        one = _read(H, d, False, w, h, nc)
        assert one[0] == 0 and np.array_equal(frames[f], one[2]), f
        assert np.array_equal(frames[f].reshape(nc, h, w).astype(np.int32), oracle_ref(oracle, d)), f
    # a frame for the fallback reader, a frame of another geometry: false, nothing written -- the host reads frame by frame
    for other in (_with_coc(g3, (1,), -1), load("g6_300x200_rgb8_97_ict.j2k")):
        rcode, frames, err = read_files([g3, other, g3])
        assert rcode == 0 and (frames == GUARD).all(), err
    rcode, frames, err = read_files([g3, g3[:60]])  # a damaged frame
    assert rcode == -1 and err.startswith("Error reading file") and "frame 1: " in err and (frames == GUARD).all()
