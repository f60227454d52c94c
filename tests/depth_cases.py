"""Inputs and the model of the sample-depth tests (test_depth_model.py anywhere; test_depth_matrix.py and test_depth_encode.py
on the GPU): every (sample type, channel depth, file depth) the C ABI accepts on the encode side.

A stored sample of a channel of depth d in a container of sample_bits bits is an integer 0 .. 2^d - 1 (right-justified: what
j2k_hip_plane.depth says); larger stored values are outside the ABI's contract and never fed.  The codec sees
    Promote (promote_ae16, 16-bit samples of depth 16)  ->  CopyChannel d -> prec  ->  DC shift  ->  RCT / ICT
and convert() below is the one numpy CopyChannel of the test tree (rgba_model.depth_convert with DESTTYPE = int: nothing is
truncated below 32 bits).  test_depth_model.py holds it to the oracle's C text on all of PAIRS before any device is involved.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import float_model as fm
import rgba_model
from j2k_amd import synth

# (sample_bits, d, prec): 128 + 256 triples
PAIRS = [(8, d, prec) for d in range(1, 9) for prec in range(1, 17)] + [(16, d, prec) for d in range(1, 17) for prec in range(1, 17)]
# float channels standing for integers of depth d: (d, prec)
FLOAT_PAIRS = [(d, prec) for d in range(1, 17) for prec in range(1, 17)]
PRECS = list(range(1, 17))
# channel depths that share one launch of the strided front end and of the compare kernel (four channels of unequal depth)
GROUPS = {16: [(1, 2, 3, 4), (5, 6, 7, 8), (9, 10, 11, 12), (13, 14, 15, 16)], 8: [(1, 2, 3, 4), (5, 6, 7, 8)]}
# channel c holds the ramp rotated by ROT[c] samples: odd, all different, below the 256 samples of the 8-bit ramp
ROT = (1, 37, 101, 203)


def depths(sample_bits: int):
    return range(1, sample_bits + 1)


def pairs_of(prec: int):
    """(sample_bits, d) of the PAIRS with this file depth: 24."""
    return [(sb, d) for (sb, d, p) in PAIRS if p == prec]


def dtype_of(sample_bits: int):
    return {8: np.uint8, 16: np.uint16}[sample_bits]


WIDTH = 512  # columns of every integer frame: the fused level-1 kernel's second strip of such a frame is a FAST one


def shape(sample_bits: int):
    """(rows, columns) of the ramp: 128 x 512 holds the 65536 values of a 16-bit container once, 16 x 512 the 256 values of an
    8-bit container 32 times.  512 columns and at least 16 rows because dwt_fused_kernel takes its vector-load (FAST) form
    only for a strip whose 256 columns from column 2 * (124 * wave - 2) on lie inside the frame: of the three strips of a
    512-column frame the second (columns 244..499) is FAST, the first and the third are edge strips
    (test_depth_model.py::test_frames_reach_fast_and_edge_strips holds the launch model to that)."""
    return ((1 << sample_bits) * (32 if sample_bits == 8 else 1) // WIDTH, WIDTH)


def ramp(sample_bits: int, d: int) -> np.ndarray:
    """The exhaustive input of one channel: every value of the container in turn, masked to the d bits a channel of depth d
    may hold, so every legal stored value occurs (equally often).  shape(sample_bits), int64."""
    assert 1 <= d <= sample_bits
    rows, cols = shape(sample_bits)
    return (np.arange(rows * cols, dtype=np.int64) & ((1 << d) - 1)).reshape(rows, cols)


def channel(sample_bits: int, d: int, c: int) -> np.ndarray:
    """Channel c of a frame: the ramp rotated by ROT[c] (a channel swap or an offset slip shows), and one more row that holds
    0 or 2^d - 1 by the bits of (column mod 16) -- bit c for channel c -- so that pixels of every full-range corner (all
    channels 0, all 2^d - 1 and the fourteen between) reach the colour transforms.  129 x 512 or 17 x 512, int64."""
    r = ramp(sample_bits, d)
    body = np.roll(r.reshape(-1), ROT[c]).reshape(r.shape)
    corner = np.where((np.arange(r.shape[1]) >> c) & 1, (1 << d) - 1, 0)
    return np.concatenate([body, corner[None, :]])


def channels(sample_bits: int, ds) -> np.ndarray:
    """(len(ds), H, W) int64: channel c at depth ds[c]."""
    return np.stack([channel(sample_bits, d, c) for c, d in enumerate(ds)])


def convert(v, d: int, prec: int) -> np.ndarray:
    """CopyChannel<int, SRC> in numpy, any d and prec in 1..16: int64."""
    return rgba_model.depth_convert(np.asarray(v), d, prec, 32)


def promote(v) -> np.ndarray:
    """After Effects' 15+1 -> 16 bit Promote() of a 16-bit sample (the result wraps to 16 bits)."""
    return fm.promote16(v)


def samples(stored, ds, prec: int, promoted: bool = False) -> np.ndarray:
    """Stored integer channels (depth ds[c]) -> (nc, H, W) int64 unsigned samples of prec bits as the codec sees them."""
    return np.stack([convert(promote(ch) if promoted else ch, d, prec) for ch, d in zip(stored, ds)])


def float_ramp(d: int, promoted: bool = False) -> np.ndarray:
    """The exhaustive input of one float channel of depth d: p / (2^d - 1) for every p, in float32 arithmetic; promoted
    (d = 16): Demote(v) / 32768 for every 16-bit v.  2-D float32, at most 256 x 256."""
    p = np.arange(1 << d, dtype=np.int64)
    x = fm.to_float(fm.demote16(p), 16, True) if promoted else fm.to_float(p, d)
    cols = min(p.size, 256)
    return x.reshape(p.size // cols, cols)


def float_channels(d: int, nc: int, promoted: bool = False) -> np.ndarray:
    """(nc, H, W) float32: channel c holds the float ramp rotated by ROT[c]."""
    r = float_ramp(d, promoted)
    return np.stack([np.roll(r.reshape(-1), ROT[c]).reshape(r.shape) for c in range(nc)])


def float_samples(x, d: int, prec: int, promoted: bool = False) -> np.ndarray:
    """Float channels standing for depth d -> (nc, H, W) int64 samples of prec bits."""
    return np.stack([convert(fm.quantise(ch, d, promoted), d, prec) for ch in x])


def planes(w: int, h: int, nc: int, prec: int, seed: int) -> np.ndarray:
    """(nc, h, w) int32 unsigned samples of any prec >= 1: a gradient plus LCG noise, by synth.planes' formula written so that
    it also works below 8 bits.  Two samples of every component are then overwritten, one with 0 and one with 2^prec - 1;
    from prec 8 on every other sample equals synth.planes(w, h, nc, prec, seed)."""
    nbits = max(prec - 4, 1)
    s = synth.lcg_stream(seed, nc * h * w).reshape(nc, h, w)
    x = np.arange(w, dtype=np.int64)[None, None, :]
    y = np.arange(h, dtype=np.int64)[None, :, None]
    c = np.arange(nc, dtype=np.int64)[:, None, None]
    grad = ((3 * x + 5 * y + 977 * c) << prec) // 1024
    noise = (s >> np.uint32(32 - nbits)).astype(np.int64)
    pl = (grad + noise) & ((1 << prec) - 1)
    for k in range(nc):
        pl[k, 0, k] = 0
        pl[k, h - 1, w - 1 - k] = (1 << prec) - 1
    return pl.astype(np.int32)


def frontend_words(oracle, smp, prec: int, rev: bool, mct: bool) -> np.ndarray:
    """Unsigned samples of prec bits (nc, H, W) -> the front end's output words, int32 (float32 bit patterns for 9/7): the
    oracle's DC shift and RCT / ICT, composed as test_gpu_parity.py::test_frontend_matches_oracle composes them."""
    ref = np.ascontiguousarray(np.asarray(smp).astype(np.int32))
    nc = ref.shape[0]
    ptrs = (C.POINTER(C.c_int32) * nc)(*[ref[c].ctypes.data_as(C.POINTER(C.c_int32)) for c in range(nc)])
    oracle.L.j2ko_dc_mct.argtypes = [C.POINTER(C.POINTER(C.c_int32)), C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int]
    oracle.L.j2ko_dc_mct(ptrs, nc, ref[0].size, prec, int(rev), int(mct))
    return ref


def level1_words(oracle, smp, prec: int, rev: bool, mct: bool) -> np.ndarray:
    """The same through one level of the oracle's 5/3 or 9/7 transform (what dwt_variant_cases.reference does): int32 view."""
    fe = frontend_words(oracle, smp, prec, rev, mct)
    pl = fe if rev else fe.view(np.float32)
    f = oracle.dwt53 if rev else oracle.dwt97
    return np.stack([f(pl[c], 1, 0, 0) for c in range(pl.shape[0])]).view(np.int32)


def interleaved(chans, sample_bits: int, row_pad: int = 0):
    """[R, G, B, A] planes (fewer: the missing ones stay 0xff bytes) -> (buffer, layout) of an After Effects A,R,G,B frame of
    8-bit, 16-bit or (sample_bits 32) float samples, the layout synth.ae_frame describes."""
    dt = {8: np.uint8, 16: np.uint16, 32: np.float32}[sample_bits]
    sb = sample_bits // 8
    h, w = chans[0].shape
    rowbytes = 4 * sb * w + row_pad
    buf = np.full(h * rowbytes, 0xff, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(buf.view(dt), shape=(h, w, 4), strides=(rowbytes, 4 * sb, sb), writeable=True)
    for slot, ch in zip((1, 2, 3, 0), chans):
        view[:, :, slot] = np.asarray(ch).astype(dt)
    return buf, dict(sample_bytes=sb, colbytes=4 * sb, rowbytes=rowbytes, channel_offsets=(0, sb, 2 * sb, 3 * sb))


def strided(chans, dt, step: int = 2, lead: int = 1):
    """Channels -> (store, views): views[c] = store[c, :, lead::step], every step-th sample of a padded row (colbytes above
    the sample size, the rows of a plane begin `lead` samples in)."""
    chans = [np.asarray(ch) for ch in chans]
    h, w = chans[0].shape
    store = np.zeros((len(chans), h, lead + w * step + 1), dtype=dt)
    if np.dtype(dt) == np.float32:
        store[...] = np.nan
    else:
        store[...] = np.iinfo(dt).max  # (what lies between the samples is never a legal small-depth value)
    views = [store[c, :, lead::step][:, :w] for c in range(len(chans))]
    for v, ch in zip(views, chans):
        v[...] = ch.astype(dt)
    return store, views


def dense(chans, dt):
    """Channels -> (buffer, offsets, arrays): contiguous planes, each at a multiple of 16 bytes of one buffer."""
    arrs = [np.ascontiguousarray(np.asarray(ch).astype(dt)) for ch in chans]
    offs, pos = [], 0
    for a in arrs:
        offs.append(pos)
        pos += -(-a.nbytes // 16) * 16
    buf = np.zeros(max(pos, 16), np.uint8)
    for a, o in zip(arrs, offs):
        buf[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
    return buf, offs, arrs
