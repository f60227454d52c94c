"""numpy model of the fused RGBA output stage, written from the specification in include/j2k_hip.h (j2k_hip_rgba_dst), not
from any implementation: every expected value of the RGBA tests comes from here.

Input: component samples as a decoder delivers them -- unsigned, each at its own precision, on its own (sub-sampled) grid.
Output: (R, G, B, A) planes of the window, A = None never: a mode without alpha fills it.

All float arithmetic is np.float32, one operation at a time in the stated order (numpy does not contract), and the cast to
int truncates (np.trunc)."""
from __future__ import annotations

import numpy as np

RGB, GREY, PALETTE, SYCC = 1, 2, 3, 4

F = np.float32
K_CR_R = F(2 * (1 - 0.299))
K_CB_B = F(2 * (1 - 0.114))
K_CR_G = F(2 * 0.299 * (1 - 0.299) / 0.587)
K_CB_G = F(2 * 0.114 * (1 - 0.114) / 0.587)
assert K_CR_R.view(np.uint32) == 0x3FB374BC and K_CB_B.view(np.uint32) == 0x3FE2D0E5
assert K_CR_G.view(np.uint32) == 1060557219 and K_CB_G.view(np.uint32) == 1051734690


def depth_convert(v: np.ndarray, src: int, dst: int, sample_bits: int) -> np.ndarray:
    """The reference's CopyChannel rule for unsigned samples (src bits -> dst bits in a sample type of sample_bits): shift down,
    or replicate the bits upwards; every intermediate is truncated to the sample type."""
    v = v.astype(np.int64)
    mask = (1 << sample_bits) - 1
    shift = dst - src
    if shift == 0:
        return v
    if shift < 0:
        return v >> (-shift)
    if src >= 8:
        if shift <= src:
            return (v << shift) | (v >> (src - shift))
        second = shift - src
        t = ((v << src) | v) & mask
        return (t << second) | (t >> (src * 2 - second))
    pd, t = src, v
    while pd * 2 < dst:
        t = ((t << pd) | t) & mask
        pd *= 2
    second = dst - pd
    return (t << second) | (t >> (pd - second))


def replicate(comp: np.ndarray, sub, width: int, height: int, org=(0, 0), outside: int = 0) -> np.ndarray:
    """A component on its own grid -> the window's grid: position (x, y) reads ((org_y + y) // sub_y, (org_x + x) // sub_x).
    With an image origin that is no multiple of the sub-sampling factor the component's grid can be one sample short of
    ceil(size / sub) (image columns 3..43 at sub 2: 20 samples for 41 columns); a position past it reads `outside` -- the
    decoder's planes hold a zero coefficient there, so the caller passes the DC level 2^(prec - 1), which is what
    j2k_hip_decode has delivered at such positions since it decodes sub-sampled components."""
    comp = np.asarray(comp)
    ys = (org[1] + np.arange(height)) // sub[1]
    xs = (org[0] + np.arange(width)) // sub[0]
    padded = np.full((max(comp.shape[0], int(ys.max()) + 1), max(comp.shape[1], int(xs.max()) + 1)), outside, dtype=np.int64)
    padded[:comp.shape[0], :comp.shape[1]] = comp
    return padded[np.ix_(ys, xs)]


def sycc(y: np.ndarray, cb: np.ndarray, cr: np.ndarray, depth: int):
    """Y, Cb, Cr at `depth` bits -> R, G, B at `depth` bits."""
    h = 1 << (depth - 1)
    top = (1 << depth) - 1
    sy = (y.astype(np.int64) - h).astype(F)
    scb = (cb.astype(np.int64) - h).astype(F)
    scr = (cr.astype(np.int64) - h).astype(F)
    fr = sy + K_CR_R * scr
    fg = (sy - K_CR_G * scr) - K_CB_G * scb
    fb = sy + K_CB_B * scb
    out = []
    for f in (fr, fg, fb):
        assert f.dtype == F
        t = (f + F(h)) + F(0.5)
        assert t.dtype == F
        out.append(np.clip(np.trunc(t).astype(np.int64), 0, top))
    return out


def demote(v: np.ndarray) -> np.ndarray:
    v = v.astype(np.int64)
    return np.where(v > 32768, ((v - 1) >> 1) + 1, v >> 1)


def rgba(mode: int, comps, precs, subs, width: int, height: int, depth: int, sample_bits: int, org=(0, 0), lut=None, lut_rgb=(0, 1, 2),
         demote_ae16: bool = False):
    """comps[c]: 2-D unsigned samples of component c at precs[c] bits on its grid (sub-sampling subs[c] = (sub_x, sub_y)).
    Returns [R, G, B, A] as int64 (height, width) planes."""
    full = [replicate(c, s, width, height, org, 1 << (p - 1)) for c, s, p in zip(comps, subs, precs)]
    conv = lambda c: depth_convert(full[c], precs[c], depth, sample_bits)
    alpha = None
    if mode == RGB:
        out = [conv(0), conv(1), conv(2)]
        alpha = conv(3) if len(full) >= 4 else None
    elif mode == GREY:
        g = conv(0)
        out = [g, g, g]
        alpha = conv(1) if len(full) >= 2 else None
    elif mode == PALETTE:
        lut = np.asarray(lut, dtype=np.int64)
        idx = full[0]
        ok = idx < lut.shape[0]
        safe = np.where(ok, idx, 0)
        out = []
        for k in range(3):
            e = np.where(ok, lut[safe, lut_rgb[k]], 0)
            out.append(e if sample_bits == 8 else (e << 8) | e)
    elif mode == SYCC:
        out = sycc(conv(0), conv(1), conv(2), depth)
    else:
        raise ValueError(mode)
    out.append(alpha if alpha is not None else np.full((height, width), (1 << depth) - 1, dtype=np.int64))
    if demote_ae16:
        assert sample_bits == 16 and depth == 16
        out = [demote(v) for v in out]
    return out


def file_rgba(mode: int, comps: list, width: int, height: int, depth: int, sample_bits: int, org=(0, 0), lut=None, lut_rgb=(0, 1, 2),
              demote_ae16: bool = False):
    """From OpjReplay.decode_comps' result (dicts with data, prec, sgnd, dx, dy): signed components are offset to unsigned as the
    decoder's output stage does; the first four count; sYCC reads three."""
    comps = comps[:4]
    if mode == SYCC:
        comps = comps[:3]
    data = [c["data"].astype(np.int64) + ((1 << (c["prec"] - 1)) if c["sgnd"] else 0) for c in comps]
    return rgba(mode, data, [c["prec"] for c in comps], [(c["dx"], c["dy"]) for c in comps], width, height, depth, sample_bits, org, lut,
                lut_rgb, demote_ae16)


def into_ae_frame(frame: np.ndarray, layout: dict, planes, alpha: bool = True) -> np.ndarray:
    """Write [R, G, B, A] planes (top-left part that fits) into a copy of an After Effects A,R,G,B frame (synth.ae_frame)."""
    out = frame.copy()
    sb = layout["sample_bytes"]
    h, w = planes[0].shape
    for p, off in zip(planes if alpha else planes[:3], (layout["channel_offsets"][k] for k in (1, 2, 3, 0))):
        view = np.lib.stride_tricks.as_strided(out[off:].view(np.uint8 if sb == 1 else np.uint16), shape=(h, w),
                                               strides=(layout["rowbytes"], layout["colbytes"]), writeable=True)
        view[...] = p.astype(view.dtype)
    return out
