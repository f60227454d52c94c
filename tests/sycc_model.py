"""numpy model of the RGB -> Y Cb Cr front end with chroma decimation (j2k_hip_params.rgb_to_sycc), written from the
specification in include/j2k_hip.h, not from the kernel: every expected value of the sub-sampling front-end tests comes from
here.

Input: R, G, B[, A] planes of unsigned samples at `depth` bits (after Promote and the depth conversion: rgba_model.depth_convert
and promote() below bring stored samples there).  Output: Y, Cb, Cr[, A], each on its own grid, unsigned at `depth` bits; the
front end's planes are these minus 2^(depth - 1).

All arithmetic is exact: Python-sized integers held in int64 (the largest intermediate, four chroma terms of 16-bit samples,
is below 2^34), `>>` on a negative int64 floors."""
from __future__ import annotations

import numpy as np

Y_R, Y_G, Y_B = 19595, 38470, 7471
CB_R, CB_G, CB_B = -11059, -21709, 32768
CR_R, CR_G, CR_B = 32768, -27439, -5329


def promote(v: np.ndarray) -> np.ndarray:
    """After Effects' 15+1 -> 16 bit Promote of a 16-bit sample (the result wraps to 16 bits)."""
    v = np.asarray(v).astype(np.int64)
    return np.where(v > 16384, ((v - 1) << 1) + 1, v << 1) & 0xffff


def box_sum(p: np.ndarray, sub) -> np.ndarray:
    """Sum over the sub_x x sub_y pixels of every chroma sample; a pixel beyond the right or bottom edge repeats the last column
    or row."""
    sx, sy = sub
    h, w = p.shape
    ch, cw = -(-h // sy), -(-w // sx)
    ys = np.minimum(np.arange(ch * sy), h - 1)
    xs = np.minimum(np.arange(cw * sx), w - 1)
    full = p[np.ix_(ys, xs)]
    return full.reshape(ch, sy, cw, sx).sum(axis=(1, 3))


def sycc_planes(planes, depth: int, sub=(1, 1)):
    """planes: [R, G, B] or [R, G, B, A], 2-D, unsigned at `depth` bits -> [Y, Cb, Cr[, A]] unsigned at `depth` bits; Cb and Cr
    on the grid of ceil(size / sub), Y and A at full size."""
    r, g, b = (np.asarray(p).astype(np.int64) for p in planes[:3])
    h, top = 1 << (depth - 1), (1 << depth) - 1
    k = {1: 0, 2: 1, 4: 2}[sub[0] * sub[1]]
    y = (Y_R * r + Y_G * g + Y_B * b + 32768) >> 16
    cbp = CB_R * r + CB_G * g + CB_B * b
    crp = CR_R * r + CR_G * g + CR_B * b
    cb = np.clip(h + ((box_sum(cbp, sub) + (1 << (15 + k))) >> (16 + k)), 0, top)
    cr = np.clip(h + ((box_sum(crp, sub) + (1 << (15 + k))) >> (16 + k)), 0, top)
    out = [y, cb, cr]
    if len(planes) >= 4:
        out.append(np.asarray(planes[3]).astype(np.int64))
    return out


def frontend_planes(planes, depth: int, sub=(1, 1)):
    """What the front end writes: sycc_planes minus the DC level 2^(depth - 1)."""
    return [p - (1 << (depth - 1)) for p in sycc_planes(planes, depth, sub)]
