"""The X'Y'Z' -> R'G'B' conversion of j2k_hip_decode_set_xyz_to_rgb in numpy, exactly as include/j2k_hip.h defines it: code ->
linear light by table, the scaled X Y Z -> R G B matrix with every product and sum rounded to binary32, the channel as the
number of thresholds <= the value.  The tables can be given in (the library's own: api.xyz_inverse_tables) or made from the
formula here.  `rgba` is the RGB mode of rgba_model.py with the conversion in it: what the RGBA output stage must deliver."""
import numpy as np

import rgba_model as rm
import xyz_model

N_XYZ_TO_709 = np.array([[3.2404542, -1.5371385, -0.4985314],
                         [-0.9692660, 1.8760108, 0.0415560],
                         [0.0556434, -0.2040259, 1.0572252]], dtype=np.float64)


# What the way there and back loses at 8 bits: R'G'B' -> 12-bit X'Y'Z' codes (j2k_hip_params.rgb_to_xyz, xyz_model.codes) -> R'G'B'
# (this conversion), over all 2^24 colours, per target: (largest channel error, colours that come back exactly).  Measured by
# test_xyz_inverse_host.py, which asserts them; DESIGN.md quotes them.  The losses sit in the dark colours, where a 12-bit
# code under a 2.6 power is coarser than the target's own 8-bit code; linear light loses nothing.
ROUND_TRIP_8BIT = {1: (4, 15776914), 2: (15, 14188488), 3: (0, 1 << 24)}


def formula_tables(target: int, comp_depth: int, dst_depth: int):
    """(dl, othr, matrix) from the definition: float32 arrays of 2^comp_depth, 2^dst_depth - 1 and 3 x 3 values."""
    c = np.arange(1 << comp_depth, dtype=np.float64)
    dl = np.power(c / float((1 << comp_depth) - 1), 2.6).astype(np.float32)
    top = (1 << dst_depth) - 1
    k = np.arange(1, top + 1, dtype=np.float64)
    othr = xyz_model.eotf(target, (k - 0.5) / float(top)).astype(np.float32)
    n = (N_XYZ_TO_709 * (52.37 / 48.0)).astype(np.float32)
    return dl, othr, n


def linear(xyz, comp_depth: int, dl, n):
    """(3, ...) X'Y'Z' codes of comp_depth bits -> [r, g, b] linear light, float32 (may be negative: out of gamut)."""
    n = np.asarray(n, dtype=np.float32).reshape(3, 3)
    top = (1 << comp_depth) - 1
    l = [np.asarray(dl, dtype=np.float32)[np.clip(np.asarray(xyz[c]).astype(np.int64), 0, top)] for c in range(3)]
    out = []
    for i in range(3):
        p = [(n[i, j] * l[j]).astype(np.float32) for j in range(3)]             # every product rounded to binary32
        out.append(((p[0] + p[1]).astype(np.float32) + p[2]).astype(np.float32))  # every sum too, left to right
    return out


def rgb(xyz, target: int, comp_depth: int, dst_depth: int, tables=None) -> np.ndarray:
    """xyz: (3, ...) integer X'Y'Z' codes of comp_depth bits -> (3, ...) R'G'B' codes of dst_depth bits (int64)."""
    dl, othr, n = tables if tables is not None else formula_tables(target, comp_depth, dst_depth)
    othr = np.asarray(othr, dtype=np.float32)
    return np.stack([np.searchsorted(othr, r, side="right").astype(np.int64) for r in linear(xyz, comp_depth, dl, n)])


def rgba(comps, precs, subs, width: int, height: int, depth: int, sample_bits: int, target: int, org=(0, 0), demote_ae16: bool = False,
         tables=None):
    """rgba_model.rgba(RGB, ...) with the conversion: comps[c] = unsigned samples of component c at precs[c] bits on its grid.
    R, G, B come from components 0..2 at their own precision; A (a fourth component, or the fill) is the RGB mode's."""
    assert precs[0] == precs[1] == precs[2]
    plain = rm.rgba(rm.RGB, comps, precs, subs, width, height, depth, min(sample_bits, 16), org)
    full = [rm.replicate(c, s, width, height, org, 1 << (p - 1)) for c, s, p in zip(comps[:3], subs[:3], precs[:3])]
    out = list(rgb(full, target, precs[0], depth, tables)) + [plain[3]]
    return [rm.demote(v) for v in out] if demote_ae16 else out
