"""The decode's output stage in isolation (run with -m gpu): decode_output_kernel -- inverse RCT / ICT, DC level shift, clamp,
replication of sub-sampled components and CopyChannel's depth conversion into the caller's channels -- through
j2k_hip_stage_decode_output, whose arguments are filled by the function a decode fills them with.  Every comparison is byte
for byte over the WHOLE channel buffer: the channels' samples against the reference, every other byte against the pattern
the buffer was filled with.  No tolerance, no case left out.

The reference (decode_output_cases.expected): Oracle.decode_output, the tail of the oracle's tile decode that the whole-file
tests pin to libopenjp2; np.repeat(...)[:h, :w] for the replication; Oracle.copy_channel_out for the depth conversion.
test_decode_output_refs.py anchors that reference on these very inputs without a GPU.

  * depth conversion: all 384 (precision 1..16, 8- or 16-bit samples, depth 1..sample bits), every sample value of each;
  * the clamp of the reversible path at and around both ends for precisions 1, 7, 8, 12, 16, +-2^30; through the inverse RCT
    with one, two or three of R, G, B beyond either end, sums (u + w) that are negative and not multiples of four;
  * the irreversible conversion: ties, zeros, denormals, the clamp's edges, +-2^31 and its neighbours, 3e9, 1e30, FLT_MAX,
    infinities, NaNs, random bit patterns, ordinary planes; through the inverse ICT with each of Y, U, V holding them in turn;
  * widths 1, 255, 256, 257, 513, 1000; 70 000 rows (the row loop's second step); a stride larger than the width;
  * sub-sampling factors 1..4 differing per component and direction with differing precisions, 4:2:0 and 4:2:2;
  * After Effects ARGB frames, padded planar rows, bottom-up rows, 3-byte pixels, fewer channels than components and the
    reverse, destinations smaller and larger than the image, 8- and 16-bit channels in one call;
  * what the hook refuses.
"""
import numpy as np
import pytest

import decode_output_cases as oc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def enc():
    from j2k_amd import api
    e = api.Encoder(0)
    yield e
    e.close()


def _check(enc, oracle, cases):
    assert cases
    for case in cases:
        oc.assert_buffers_equal(oc.run(enc, case), oc.expected(oracle, case), case)


def test_depth_conversion_every_triple_every_value(enc, oracle):
    """All 384 triples, every value.  Two edits of depth_out's doubling loop pass this test, and must, because they change
    no output: inside the loop t holds 2 pd bits with 2 pd < dst_depth, so `& dst_mask` removes nothing; and with `<=` for
    `<` the loop's extra step (taken when 2 pd == dst_depth) computes what the final fill computes without it, the final
    fill then shifting by 0 and OR-ing in t >> 2 pd = 0."""
    cases = oc.depth_cases()
    assert len(cases) * 4 == 384
    _check(enc, oracle, cases)


def test_clamp_reversible(enc, oracle):
    _check(enc, oracle, oc.clamp_rev_cases())


def test_float_conversion(enc, oracle):
    _check(enc, oracle, oc.float_cases())


def test_launch_shapes(enc, oracle):
    cases = oc.shape_cases()
    assert any(c["h"] > 65535 for c in cases) and any(c["stride"] and c["stride"] > c["w"] for c in cases)
    _check(enc, oracle, cases)


def test_subsampling(enc, oracle):
    _check(enc, oracle, oc.subsampling_cases())


def test_destination_geometry(enc, oracle):
    _check(enc, oracle, oc.geometry_cases())


# ------------------------------------------------------------------------------------------------ refusals
def _small():
    w, h = 6, 4
    chans, nbytes = oc.planar(w, h, [(8, 8), (16, 12), (8, 8)])
    comps = [np.arange(w * h, dtype=np.int32).reshape(h, w) - 12 for _ in range(3)]
    return oc.make_case("small", True, False, w, h, comps, [8, 12, 8], [(1, 1)] * 3, chans, nbytes)


def _refused(enc, case):
    from j2k_amd import api
    with pytest.raises(api.J2kHipError) as e:
        oc.run(enc, case)
    assert e.value.code == 1, e.value  # J2K_HIP_ERR_PARAM
    return str(e.value)


def test_hook_accepts_the_small_case(enc, oracle):
    """The case the refusals below are one change away from."""
    _check(enc, oracle, [_small()])


@pytest.mark.parametrize("bits, depth", [(12, 8), (32, 8), (0, 1), (8, 0), (8, 9), (16, 17), (16, 0)])
def test_hook_refuses_sample_types_and_depths(enc, bits, depth):
    for c in range(3):
        case = _small()
        case["chans"][c].update(sample_bits=bits, depth=depth)
        _refused(enc, case)


@pytest.mark.parametrize("prec", [0, 17, 32])
def test_hook_refuses_precisions(enc, prec):
    for c in range(3):
        case = _small()
        case["precs"][c] = prec
        _refused(enc, case)


def test_hook_refuses_unlike_components_under_the_colour_transform(enc, oracle):
    case = _small()
    case["precs"] = [8, 8, 8]
    case["mct"] = True
    _check(enc, oracle, [case])
    for c in range(3):
        bad = dict(case, precs=[8 + (i == c) for i in range(3)])
        _refused(enc, bad)
    for c in range(3):
        for sub in ((2, 1), (1, 2)):
            bad = dict(case, subs=[sub if i == c else (1, 1) for i in range(3)])
            bad["comps"] = [np.zeros((oc.cdiv(case["h"], sy), oc.cdiv(case["w"], sx)), np.int32) for sx, sy in bad["subs"]]
            _refused(enc, bad)
    _refused(enc, dict(case, comps=case["comps"][:2], precs=[8, 8], subs=[(1, 1)] * 2))


def test_hook_refuses_channels_that_leave_the_buffer(enc):
    base = _small()
    last = base["chans"][2]
    end = last["base"] + (base["h"] - 1) * last["rowbytes"] + base["w"]  # one past the last sample of the last channel
    ok = dict(base, nbytes=end)
    assert oc.run(enc, ok).size == end  # exactly fitting: accepted
    assert "outside" in _refused(enc, dict(base, nbytes=end - 1))
    for key, value in (("base", base["nbytes"]), ("base", base["nbytes"] - 1), ("rowbytes", base["nbytes"]), ("colbytes", base["nbytes"]),
                       ("rowbytes", -base["nbytes"]), ("colbytes", -base["nbytes"]), ("rowbytes", -(1 << 62)), ("colbytes", 1 << 62), ("base", 1 << 63)):
        for c in (0, 2):
            case = _small()
            case["chans"][c][key] = value
            assert "outside" in _refused(enc, case), (key, value, c)
    case = _small()  # a 16-bit channel whose last sample's second byte is the first byte past the end
    ch = case["chans"][1]
    case["nbytes"] = ch["base"] + (case["h"] - 1) * ch["rowbytes"] + 2 * case["w"] - 1
    case["chans"] = case["chans"][:2]
    assert "outside" in _refused(enc, case)


def test_hook_refuses_16_bit_channels_at_odd_addresses(enc):
    for key, delta in (("base", 1), ("rowbytes", 1), ("colbytes", 1), ("colbytes", 3)):
        case = _small()
        case["chans"][1][key] += delta
        case["nbytes"] += 64
        assert "odd" in _refused(enc, case), (key, delta)
    case = _small()  # an 8-bit channel may lie anywhere
    case["chans"][0]["base"] += 1
    case["chans"][0]["rowbytes"] += 1
    oc.run(enc, case)


def test_hook_refuses_component_planes_that_leave_their_buffer(enc):
    case = _small()
    assert "component plane" in _refused(enc, dict(case, stride=case["w"] - 1))
