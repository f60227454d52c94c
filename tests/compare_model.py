"""numpy model of j2k_hip_compare, written from the definition in include/j2k_hip.h, not from the kernel: every expected
value of the compare tests comes from here.

Source sample S_c: the unsigned integer of `depth` bits that the encode's front end makes of a stored sample, before the DC
shift and any colour transform -- Promote, the float quantisation (float_model), CopyChannel's depth conversion
(rgba_model.depth_convert), and with rgb_to_sycc the integer Y / Cb / Cr formula with its decimation (sycc_model).
Decoded sample D_c: what the decode delivers, on the component's own grid.  e = D - S; the sums are exact Python integers, the
two doubles the header's formulas in IEEE double arithmetic (math.log10: the C library's)."""
from __future__ import annotations

import math

import numpy as np

import float_model as fm
import rgba_model
import sycc_model


def source_samples(stored, src_depth: int, depth: int, promote: bool = False) -> np.ndarray:
    """One channel as stored (uint8 / uint16 holding src_depth significant bits, or float32 standing for src_depth bits) ->
    int64 samples of `depth` bits."""
    stored = np.asarray(stored)
    if stored.dtype == np.float32:
        v = fm.quantise(stored, src_depth, promote)
    else:
        v = stored.astype(np.int64)
        if promote and stored.dtype.itemsize == 2:
            v = fm.promote16(v)
    return rgba_model.depth_convert(v, src_depth, depth, 32)


def source_components(channels, src_depths, depth: int, promote: bool = False, rgb_to_sycc=None):
    """The channels as stored -> [S_c], each on its own grid.  rgb_to_sycc = (sub_x, sub_y) of Cb and Cr: the channels are R, G,
    B[, A] of the full image; otherwise channel c is component c as it is."""
    s = [source_samples(ch, d, depth, promote) for ch, d in zip(channels, src_depths)]
    return sycc_model.sycc_planes(s, depth, tuple(rgb_to_sycc)) if rgb_to_sycc else s


def own_grid(delivered: np.ndarray, sub) -> np.ndarray:
    """What the decode delivered for a component on the image's grid -> the component's own grid: the sample at
    (x * sub_x, y * sub_y) (the decode replicates)."""
    return np.asarray(delivered)[::sub[1], ::sub[0]]


def diff(source: np.ndarray, decoded: np.ndarray, depth: int) -> dict:
    """j2k_hip_diff of one component: both arrays on the component's own grid."""
    s = np.asarray(source).astype(np.int64)
    d = np.asarray(decoded).astype(np.int64)
    assert s.shape == d.shape and s.ndim == 2
    e = d - s
    nz = np.flatnonzero(e.reshape(-1))
    sum_sq = sum(int(v) * int(v) for v in e.reshape(-1)[nz].tolist())  # (Python integers: no 64-bit wrap to argue about)
    samples = int(e.size)
    mse = float(sum_sq) / float(samples)
    top = float((1 << depth) - 1)
    return dict(samples=samples, differing=int(nz.size), sum_abs=int(np.abs(e).sum()), sum_sq=sum_sq,
                max_abs=int(np.abs(e).max()) if e.size else 0,
                first_x=int(nz[0] % e.shape[1]) if nz.size else 0, first_y=int(nz[0] // e.shape[1]) if nz.size else 0,
                mse=mse, psnr=10.0 * math.log10((top * top) / mse) if sum_sq else math.inf)


def diffs(sources, decodeds, depth: int) -> list:
    return [diff(s, d, depth) for s, d in zip(sources, decodeds)]
