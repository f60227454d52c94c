"""CPU: the host side of j2k_hip_params.rgb_to_xyz (include/j2k_hip.h) -- the tables j2k_hip_xyz_tables hands out against
the formula, the numpy model (xyz_model.py) on anchor values, the refusals, and the headers, which do not depend on the field."""
import os

import numpy as np
import pytest

import xyz_model
from conftest import GOLDEN_DIR
from j2k_amd import api

J2K_HIP_ERR_PARAM = 1


def ulps(a: np.ndarray, b: np.ndarray) -> int:
    """Largest distance of two arrays of non-negative binary32 values in units of the last place."""
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())


@pytest.mark.parametrize("source", [1, 2, 3])
def test_tables_against_the_formula(source):
    """The matrix uses double multiplies and one rounding: bit-identical.  lin and thr go through pow: libm's and numpy's may
    differ in the last double bit, which moves a binary32 rounding by one step and no further -- 1 ulp."""
    for sd in (8, 12, 16):
        for dd in (8, 12, 16):
            lin, thr, m = api.xyz_tables(source, sd, dd)
            wl, wt, wm = xyz_model.formula_tables(source, sd, dd)
            assert lin.dtype == thr.dtype == m.dtype == np.float32
            assert lin.shape == (1 << sd,) and thr.shape == ((1 << dd) - 1,) and m.shape == (3, 3)
            assert m.tobytes() == wm.tobytes()
            assert ulps(lin, wl) <= 1 and ulps(thr, wt) <= 1
            assert np.all(np.diff(thr) > 0) and thr[0] > 0
            assert lin[0] == 0 and lin[-1] == 1


def test_tables_refuse_what_has_no_table():
    for args in ((0, 8, 12), (4, 8, 12), (1, 0, 12), (1, 17, 12), (1, 8, 0), (1, 8, 17)):
        with pytest.raises(api.J2kHipError) as ei:
            api.xyz_tables(*args)
        assert ei.value.code == J2K_HIP_ERR_PARAM


def test_null_outputs_are_skipped():
    L = api.load_library()
    m = np.zeros(9, np.float32)
    assert L.j2k_hip_xyz_tables(1, 16, 16, None, None, m.ctypes.data) == 0
    assert m.reshape(3, 3).tobytes() == xyz_model.formula_tables(1, 8, 8)[2].tobytes()
    assert L.j2k_hip_xyz_tables(1, 16, 16, None, None, None) == 0


def test_anchors_of_the_model():
    """Source 1 (sRGB), depth 12, the pure-numpy model from the formula."""
    def code(rgb, d):
        return xyz_model.codes(np.array(rgb).reshape(3, 1), 1, d, 12)[:, 0].tolist()
    assert code((65535, 65535, 65535), 16) == [3883, 3960, 4092]  # the D65 white of the DCI literature
    assert code((0, 0, 0), 16) == [0, 0, 0]
    assert code((1, 1, 1), 16) == [20, 21, 21]
    assert code((255, 0, 0), 8) == [2817, 2183, 868]
    assert code((0, 0, 255), 8) == [2050, 1441, 3883]
    # the same with the library's own tables
    for rgb, d in (((65535, 65535, 65535), 16), ((1, 1, 1), 16), ((255, 0, 0), 8), ((0, 0, 255), 8)):
        got = xyz_model.codes(np.array(rgb).reshape(3, 1), 1, d, 12, tables=api.xyz_tables(1, d, 12))[:, 0].tolist()
        assert got == code(rgb, d)


def test_model_is_monotone_on_the_grey_axis_and_linear_sources_agree():
    v = np.arange(65536)
    for source in (1, 2, 3):
        c = xyz_model.codes(np.stack([v, v, v]), source, 16, 12)
        assert np.all(np.diff(c, axis=1) >= 0) and c[:, 0].tolist() == [0, 0, 0]
    # linear light at 8 bits: white is the matrix's row sums through the 1/2.6 power
    c = xyz_model.codes(np.array([[255], [255], [255]]), 3, 8, 12)[:, 0]
    assert c.tolist() == [3883, 3960, 4092]


REFUSALS = [
    ("above 3", dict(rgb_to_xyz=4), {}),
    ("two channels", dict(rgb_to_xyz=1), dict(channels=2)),
    ("one channel", dict(rgb_to_xyz=2), dict(channels=1)),
    ("with rgb_to_sycc", dict(rgb_to_xyz=1, rgb_to_sycc=True), {}),
    ("comp_sub 2x1", dict(rgb_to_xyz=1, sub=[(1, 1), (2, 1), (2, 1)]), {}),
    ("comp_sub 2x2", dict(rgb_to_xyz=3, sub=[(1, 1), (2, 2), (2, 2)]), {}),
    ("comp_sub on alpha", dict(rgb_to_xyz=1, sub=[(1, 1), (1, 1), (1, 1), (1, 2)]), dict(channels=4)),
]


@pytest.mark.parametrize("what,kw,geo", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_name_the_field(what, kw, geo):
    with pytest.raises(api.J2kHipError) as ei:
        api.main_header(api.make_params(64, 48, geo.get("channels", 3), 12, num_resolutions=3, **kw))
    assert ei.value.code == J2K_HIP_ERR_PARAM and "rgb_to_xyz" in str(ei.value), str(ei.value)


def test_headers_do_not_depend_on_the_field():
    cases = [dict(width=97, height=61, channels=3, depth=12, reversible=True, num_resolutions=4),
             dict(width=512, height=270, channels=3, depth=12, dci_profile=3),
             dict(width=64, height=48, channels=4, depth=12, reversible=False, ycc=True, num_resolutions=3, tile_size=32, rates=[20.0, 5.0],
                  jp2=True, alpha_channel=3, cblk=(32, 32))]
    for kw in cases:
        for v in (1, 2, 3):
            a, b = api.make_params(**kw), api.make_params(rgb_to_xyz=v, **kw)
            assert api.main_header(a) == api.main_header(b)
            assert api.file_header(a, 12345) == api.file_header(b, 12345)


def test_compare_check_reads_the_field():
    data = open(os.path.join(GOLDEN_DIR, "g3_300x200_rgb8_53_rct.j2k"), "rb").read()
    api.compare_check(api.make_params(300, 200, 3, 8, rgb_to_xyz=1), data)
    for kw in (dict(rgb_to_xyz=4), dict(rgb_to_xyz=1, rgb_to_sycc=True)):
        with pytest.raises(api.J2kHipError) as ei:
            api.compare_check(api.make_params(300, 200, 3, 8, **kw), data)
        assert ei.value.code == J2K_HIP_ERR_PARAM and "rgb_to_xyz" in str(ei.value)
    with pytest.raises(api.J2kHipError) as ei:  # the file's own disagreement keeps its text
        api.compare_check(api.make_params(300, 200, 3, 12, rgb_to_xyz=1), data)
    assert "depth" in str(ei.value)
