"""numpy model of float worlds (32-bit float samples of nominal range 0..1), written from the specification in
include/j2k_hip.h, not from the kernels: every expected value of the float tests comes from here.

Encode: a float sample x that stands for an integer of depth d (1..16) becomes
    t = x > 1 ? 1 : (x > 0 ? x : 0)                       NaN, -0.0, negatives and -inf give 0, +inf gives 1
    v = (unsigned)(t * (float)(2^d - 1) + 0.5f)           product and sum each rounded to binary32, the cast truncates
    v = promote16((unsigned)(t * 32768.0f + 0.5f))        with promote_ae16 (d = 16)
and from there on is the d-bit integer sample the library has always taken (depth conversion, DC shift, colour transform).

Decode: the integer ov of depth d that an integer destination would have received leaves as
    (float)ov / (float)(2^d - 1)                          an IEEE division, correctly rounded
    (float)ov / 32768.0f                                  with demote_ae16 (ov: the demoted sample, 0 .. 32768)

Everything below is float32 arithmetic: numpy rounds each float32 operation on its own, as the library's build does."""
from __future__ import annotations

import numpy as np

F32 = np.float32


def promote16(v):
    """After Effects' 15+1 -> 16 bit Promote (the result wraps to 16 bits)."""
    v = np.asarray(v).astype(np.int64)
    return np.where(v > 16384, ((v - 1) << 1) + 1, v << 1) & 0xffff


def demote16(v):
    """Demote: 16 -> 15+1 bit."""
    v = np.asarray(v).astype(np.int64)
    return np.where(v > 32768, ((v - 1) >> 1) + 1, v >> 1)


def clamp01(x):
    """t of the definition: the comparisons are false for NaN, so NaN gives 0."""
    x = np.asarray(x, dtype=F32)
    with np.errstate(invalid="ignore"):
        return np.where(x > F32(1), F32(1), np.where(x > F32(0), x, F32(0))).astype(F32)


def quantise(x, d: int, promote: bool = False):
    """The integer sample (int64 array) of depth d that the float sample x stands for."""
    assert 1 <= d <= 16 and (not promote or d == 16)
    t = clamp01(x)
    scale = F32(32768) if promote else F32((1 << d) - 1)
    prod = (t * scale).astype(F32)
    v = (prod + F32(0.5)).astype(F32).astype(np.int64)  # (values in 0 .. 65535.5: the cast truncates)
    return promote16(v) if promote else v


def to_float(ov, d: int, demoted: bool = False):
    """The float a destination of sample_bits 32 receives for the integer ov of depth d (demoted: ov is the demoted sample)."""
    ov = np.asarray(ov).astype(np.int64)
    div = F32(32768) if demoted else F32((1 << d) - 1)
    return (ov.astype(F32) / div).astype(F32)


def decode_floats(ints, d: int, demote: bool = False):
    """From what an integer destination of depth d holds (not demoted) to what the float destination holds."""
    return to_float(demote16(ints), d, True) if demote else to_float(ints, d)


def bits(a):
    """uint32 view of float32 values: what the tests compare."""
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.uint32)
