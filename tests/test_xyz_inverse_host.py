"""CPU: the host side of j2k_hip_decode_set_xyz_to_rgb (include/j2k_hip.h) -- the tables j2k_hip_xyz_inverse_tables hands out
against the formula for every target and depth, the thresholds' strict order, the measured round trip of all 2^24 8-bit
colours through 12-bit X'Y'Z' codes and back, j2k_hip_read_profile, and the refusals that need no device."""
import ctypes as C
import os

import numpy as np
import pytest

import xyz_inverse_model as xim
import xyz_model
from conftest import GOLDEN_DIR
from j2k_amd import api

J2K_HIP_ERR_PARAM = 1


def ulps(a: np.ndarray, b: np.ndarray) -> int:
    """Largest distance of two arrays of non-negative binary32 values in units of the last place."""
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max()) if a.size else 0


def golden_file(*parts):
    return open(os.path.join(GOLDEN_DIR, *parts), "rb").read()


@pytest.mark.parametrize("target", [1, 2, 3])
def test_tables_against_the_formula_for_every_depth(target):
    """The matrix uses double multiplies and one rounding: bit-identical.  dl and the thresholds of targets 1 and 2 go through
    pow: libm's and numpy's may differ in the last double bit, which moves a binary32 rounding by one step and no further -- 1
    ulp.  Target 3's thresholds are a double division: bit-identical."""
    wm = (xim.N_XYZ_TO_709 * (52.37 / 48.0)).astype(np.float32)
    for depth in range(1, 17):
        dl, othr, m = api.xyz_inverse_tables(target, depth, depth)
        wl, wt, _ = xim.formula_tables(target, depth, depth)
        assert dl.dtype == othr.dtype == m.dtype == np.float32
        assert dl.shape == (1 << depth,) and othr.shape == ((1 << depth) - 1,) and m.shape == (3, 3)
        assert m.tobytes() == wm.tobytes()
        assert ulps(dl, wl) <= 1 and ulps(othr, wt) <= (0 if target == 3 else 1)
        assert dl[0] == 0 and dl[-1] == 1 and np.all(np.diff(dl) > 0)
    # the two depths are independent of each other, and dl of the target
    a, b = api.xyz_inverse_tables(target, 12, 8), api.xyz_inverse_tables(target, 8, 12)
    assert a[0].tobytes() == api.xyz_inverse_tables(1, 12, 3)[0].tobytes() and a[1].tobytes() == api.xyz_inverse_tables(target, 3, 8)[1].tobytes()
    assert b[0].size == 256 and b[1].size == 4095


@pytest.mark.parametrize("target", [1, 2, 3])
def test_thresholds_increase_strictly_in_binary32(target):
    """What makes `the number of k with othr[k] <= r` a search: every target, every destination depth 1..16, the library's
    tables and the formula's."""
    for depth in range(1, 17):
        for othr in (api.xyz_inverse_tables(target, 8, depth)[1], xim.formula_tables(target, 8, depth)[1]):
            assert othr[0] > 0 and othr[-1] < 1 and np.all(np.diff(othr) > 0), depth


def test_matrix_is_the_inverse_of_the_forward_one():
    """N * M = 1 to the precision of the literals (7 digits) and of binary32."""
    m = api.xyz_tables(1, 8, 8)[2].astype(np.float64)
    n = api.xyz_inverse_tables(1, 8, 8)[2].astype(np.float64)
    assert np.abs(n @ m - np.eye(3)).max() < 2e-6


def test_tables_refuse_what_has_no_table_and_skip_null_outputs():
    for args in ((0, 8, 12), (4, 8, 12), (1, 0, 12), (1, 17, 12), (1, 8, 0), (1, 8, 17)):
        with pytest.raises(api.J2kHipError) as ei:
            api.xyz_inverse_tables(*args)
        assert ei.value.code == J2K_HIP_ERR_PARAM
    L = api.load_library()
    assert L.j2k_hip_xyz_inverse_tables(4, 8, 8, None, None, None) == J2K_HIP_ERR_PARAM
    assert "xyz_to_rgb" in L.j2k_hip_last_error(None).decode()
    m = np.zeros(9, np.float32)
    assert L.j2k_hip_xyz_inverse_tables(2, 16, 16, None, None, m.ctypes.data) == 0
    assert m.tobytes() == xim.formula_tables(2, 8, 8)[2].tobytes()
    assert L.j2k_hip_xyz_inverse_tables(2, 16, 16, None, None, None) == 0


def test_anchors_of_the_model():
    """The D65 white of the DCI literature comes back as white, black as black, and a saturated X'Y'Z' primary leaves the gamut:
    a negative linear value gives 0, one above the last threshold the top."""
    for target in (1, 2, 3):
        for tables in (None, api.xyz_inverse_tables(target, 12, 8)):
            def back(xyz):
                return xim.rgb(np.array(xyz).reshape(3, 1), target, 12, 8, tables)[:, 0].tolist()
            assert back((3883, 3960, 4092)) == [255, 255, 255]
            assert back((0, 0, 0)) == [0, 0, 0]
            # b of a pure X is 0.0556434 * 52.37 / 48 = 0.0607 in linear light, g of a pure Z 0.0415560 * 52.37 / 48 = 0.0453:
            # 255 * (1.055 * x^(1 / 2.4) - 0.055) = 69.7 and 60.1; 255 * x^(1 / 2.4) = 79.4 and 70.3; 255 * x = 15.5 and 11.6
            assert back((4095, 0, 0)) == [255, 0, {1: 70, 2: 79, 3: 15}[target]]
            assert back((0, 4095, 0)) == [0, 255, 0]
            assert back((0, 0, 4095)) == [0, {1: 60, 2: 70, 3: 12}[target], 255]
    r, g, b = xim.linear(np.array([4095, 0, 0]).reshape(3, 1), 12, *xim.formula_tables(1, 12, 8)[::2])
    assert r[0] > 1 and g[0] < 0 and 0 < b[0] < 1


ROUND_TRIP = xim.ROUND_TRIP_8BIT  # (the measured figures live beside the model: the GPU file test bounds its error by them)

_colours = {}


def all_colours():
    if not _colours:
        v = np.arange(1 << 24, dtype=np.int64)
        _colours["src"] = np.stack([v & 255, (v >> 8) & 255, v >> 16])
    return _colours["src"]


def round_trip(target):
    src = all_colours()
    codes = xyz_model.codes(src, target, 8, 12, tables=api.xyz_tables(target, 8, 12))
    return np.abs(xim.rgb(codes, target, 12, 8, tables=api.xyz_inverse_tables(target, 12, 8)) - src)


@pytest.mark.parametrize("target", [1, 2, 3])
def test_round_trip_of_every_8_bit_colour_is_what_was_measured(target):
    err = round_trip(target)
    worst, exact = int(err.max()), int((err.max(axis=0) == 0).sum())
    print(f"target {target}: worst error {worst}, {exact} of {1 << 24} colours exact ({100.0 * exact / (1 << 24):.2f} %)")
    assert (worst, exact) == ROUND_TRIP[target]
    if worst:  # where the losses sit: every error above 1 has a dark channel in its source colour
        src = all_colours()
        assert src[:, err.max(axis=0) > 1].min(axis=0).max() < 64


def test_read_profile():
    assert api.read_profile(golden_file("ext", "d1_512x270_rgb12_cinema2k.j2k")) == 3
    assert api.read_profile(golden_file("ext", "d2_1024x540_rgb12_cinema4k_poc.j2k")) == 4
    assert api.read_profile(golden_file("g3_300x200_rgb8_53_rct.j2k")) == 0
    assert api.read_profile(golden_file("j1_64x48_rgb8_srgb.jp2")) == 0  # (through the JP2 boxes)
    with pytest.raises(api.J2kHipError):
        api.read_profile(b"\xff\x4f\xff\x51\x00")
    L = api.load_library()
    buf = np.frombuffer(golden_file("g3_300x200_rgb8_53_rct.j2k"), dtype=np.uint8)
    assert L.j2k_hip_read_profile(buf.ctypes.data, buf.size, None) == J2K_HIP_ERR_PARAM
    # the library's own cinema header says so too
    hdr = api.main_header(api.make_params(512, 270, 3, 12, dci_profile=3))
    assert hdr[2:4] == b"\xff\x51" and int.from_bytes(hdr[6:8], "big") == 3  # (SOC, SIZ, Lsiz, Rsiz)


def test_no_handle_is_refused_and_the_text_names_the_setting():
    L = api.load_library()
    v = C.c_uint32(7)
    assert L.j2k_hip_decode_set_xyz_to_rgb(None, 1) == J2K_HIP_ERR_PARAM
    assert "xyz_to_rgb" in L.j2k_hip_last_error(None).decode()
    assert L.j2k_hip_decode_get_xyz_to_rgb(None, C.byref(v)) == J2K_HIP_ERR_PARAM and v.value == 7
    assert "xyz_to_rgb" in L.j2k_hip_last_error(None).decode()


def test_exports_are_listed():
    for name in ("j2k_hip_decode_set_xyz_to_rgb", "j2k_hip_decode_get_xyz_to_rgb", "j2k_hip_xyz_inverse_tables", "j2k_hip_read_profile",
                 "j2k_hip_stage_rgba_output_xyz"):
        assert name in api.EXPORTS and hasattr(api.load_library(), name)
    assert api.load_library().j2k_hip_abi_version() == 9
