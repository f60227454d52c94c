"""CPU: the float-world definition (tests/float_model.py, include/j2k_hip.h) returns every integer sample it is given.

These identities are what lets the GPU tests build float frames from the integers of committed goldens and expect the
goldens' bytes: the float of a grid point quantises back to the grid point, for every depth and in the promote form."""
import numpy as np
import pytest

import float_model as fm

F32 = np.float32


@pytest.mark.parametrize("d", [1, 2, 5, 8, 10, 12, 15, 16])
def test_grid_points_round_trip(d):
    p = np.arange(1 << d, dtype=np.int64)
    x = fm.to_float(p, d)  # float32(p) / float32(2^d - 1)
    assert x.dtype == F32
    assert np.array_equal(fm.quantise(x, d), p)


def test_promote_form_round_trips():
    v = np.arange(32769, dtype=np.int64)
    x = fm.to_float(v, 16, demoted=True)  # v / 32768
    assert np.array_equal(fm.quantise(x, 16, promote=True), fm.promote16(v))
    assert np.array_equal(fm.demote16(fm.promote16(v)), v)
    assert fm.promote16(32768) == 65535 and fm.to_float(32768, 16, demoted=True) == F32(1)


def test_decode_then_encode_is_the_identity_on_16_bit_samples():
    s = np.arange(65536, dtype=np.int64)
    assert np.array_equal(fm.quantise(fm.decode_floats(s, 16), 16), s)
    # the demoted form keeps what Demote keeps
    assert np.array_equal(fm.quantise(fm.decode_floats(s, 16, demote=True), 16, promote=True), fm.promote16(fm.demote16(s)))


@pytest.mark.parametrize("d", [1, 8, 10, 16])
def test_special_values(d):
    top = (1 << d) - 1
    tiny = np.array([1e-45, 1.17549435e-38 / 2, -1e-45], dtype=F32)  # denormals
    zeros = np.array([np.nan, -np.nan, -np.inf, -0.0, 0.0, -1.0, -1e30], dtype=F32)
    ones = np.array([np.inf, 1.0, np.nextafter(F32(1), F32(2)), 2.0, 3e38], dtype=F32)
    assert np.array_equal(fm.quantise(zeros, d), np.zeros(zeros.size, np.int64))
    assert np.array_equal(fm.quantise(tiny, d), np.zeros(tiny.size, np.int64))
    assert np.array_equal(fm.quantise(ones, d), np.full(ones.size, top, np.int64))
    if d == 16:
        assert np.array_equal(fm.quantise(zeros, 16, promote=True), np.zeros(zeros.size, np.int64))
        assert np.array_equal(fm.quantise(ones, 16, promote=True), np.full(ones.size, 65535, np.int64))


def test_rounding_is_half_up_in_float32():
    # the midpoint between two grid points and its float32 neighbours, where the product is exact (d = 1: scale 1).  The sum
    # is rounded to float32 too: 0.5 - 2^-25 + 0.5 is a tie between 1 - 2^-24 and 1.0 and goes to the even one, 1.0
    below, half = np.nextafter(F32(0.5), F32(0)), F32(0.5)
    below2 = np.nextafter(below, F32(0))
    assert fm.quantise(np.array([below2, below, half], dtype=F32), 1).tolist() == [0, 1, 1]
    # the opaque alpha fill is exactly 1.0f in both forms
    assert fm.to_float(65535, 16) == F32(1) and fm.to_float(255, 8) == F32(1)
    assert fm.decode_floats(65535, 16, demote=True) == F32(1)
