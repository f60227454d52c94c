"""Case table, CPU reference and launch model of the forward-transform parity tests (test_dwt_variants.py on the GPU,
test_dwt_variant_refs.py anywhere).

A Case is one input of Encoder.stage_transform: a frame, its channel views and the coding parameters.  The tuning knobs a
case runs under are kept beside it (a dict), never inside it: the reference does not depend on them.

reference(oracle, case) composes the oracle exactly as test_gpu_parity.py::test_frontend_matches_oracle does (copy_channel,
Promote in numpy where asked, j2ko_dc_mct), then transforms every tile-component rectangle on its own with the tile's
origin as the lifting phase and pastes the result back: the dense (ncomp, H, W) array the hook returns.

knobs(), run_hook() and check() are the GPU tests' calls (test_dwt_variants.py, test_dwt_sweep.py): one copy of them.

The launch model (level_launch, fused_launch) repeats the wave-uniform decisions of dwt.hip in a few lines of Python, so
that the CPU tests can assert that a case still reaches the path its name claims.  It mirrors, by the names in dwt.hip:
  Geo<PAIRS>                    valid pairs 124 / 60, halo lanes 1 / 2
  dwt_level_kernel              `if (k0 >= npx ...) return` and `const bool fast = PAIRS == 2 && ...`
  dwt_fused_kernel              the same two with `px * a.fe.pixb`, `a.fe.rowbytes`, `a.comp_stride`
  launch_variant                the 128, 64, .., 4 ladder of dwt_min_waves and dwt_ppc
  launch_fused                  big / wpb / the 20..10 fill search / the 16, 8, 4 ladder / fused_ppc / gen, ae, SPEC
  level_grid, block_map         the 1-D form from 8 (chunk, job) rows on, its last group of eight partly invalid
  encoder.cpp fuse_frontend     fused or not; prepare_geometry: plane stride = width rounded up to 64, one job per tile
"""
from __future__ import annotations

import contextlib
import ctypes as C
from collections import OrderedDict, namedtuple

import numpy as np
import pytest

import depth_cases
from j2k_amd import synth

# kernels.h: the defaults every test restores
DEFAULTS = dict(no_fuse=0, dwt_pairs=2, dwt_ppc=0, dwt_min_waves=2048, fused_wpb=0, fused_ppc=0, fused_generic=0, dwt_xcd=1)

# views: "ae" = synth.ae_frame (interleaved ARGB32 / ARGB64), "planar" = one plane per channel, 8-bit samples in the even
# channels and 16-bit samples in the odd ones.  bits = container bits of the ae samples; prec = FileInfo.depth.
Case = namedtuple("Case", "name w h nc rev mct bits prec promote pad levels tile views")
Input = namedtuple("Input", "buf chans samples")
Chan = namedtuple("Chan", "off colbytes rowbytes sample_bytes depth")


def kid(kn: dict) -> str:
    return ",".join(f"{k}={v}" for k, v in sorted(kn.items())) or "defaults"


# ------------------------------------------------------------------------------------------------ inputs
def convert(v, src_depth, prec):
    """CopyChannel in numpy, any pair of depths: the test tree's one copy of it (depth_cases.convert)."""
    return depth_cases.convert(v, src_depth, prec)


def promote(v):
    """The After Effects 15+1 -> 16 bit Promote()."""
    return np.where(v > 16384, ((v - 1) << 1) + 1, v << 1)


_inputs: OrderedDict = OrderedDict()


def make_input(case: Case) -> Input:
    """(frame bytes, channel views, the samples the codec is to see as numpy computes them -- without the oracle)."""
    key = case._replace(name="", rev=True, mct=False, levels=0, tile=0)
    if key in _inputs:
        _inputs.move_to_end(key)
        return _inputs[key]
    w, h, nc = case.w, case.h, case.nc
    seed = 1000 + 7 * w + 3 * h + nc
    if case.views == "planar":
        assert not case.promote and case.pad % 2 == 0
        parts, chans, smp, off = [], [], [], 0
        for c in range(nc):
            sb = 1 + (c & 1)
            pl = synth.planes(w, h, 1, 8 * sb, seed + c)[0]
            rowbytes = w * sb + case.pad
            a = np.zeros((h, rowbytes), np.uint8)
            a[:, :w * sb] = np.ascontiguousarray(pl.astype(np.uint8 if sb == 1 else "<u2")).view(np.uint8).reshape(h, w * sb)
            a = a.ravel()
            if a.size & 1:
                a = np.append(a, np.uint8(0))  # (the next 16-bit plane stays 2-byte aligned)
            chans.append(Chan(off, sb, rowbytes, sb, 8 * sb))
            parts.append(a)
            smp.append(convert(pl, 8 * sb, case.prec))
            off += a.size
        inp = Input(np.concatenate(parts), chans, np.stack(smp).astype(np.int32))
    else:
        pl = synth.planes(w, h, nc, 15 if case.promote else case.bits, seed)
        if case.promote:
            assert case.bits == 16
            pl[:, ::7, ::5] = 32768  # the After Effects white
        frame, lay = synth.ae_frame(pl, case.bits, row_pad_bytes=case.pad)
        sb, offs = lay["sample_bytes"], lay["channel_offsets"]
        assert sb * 8 == case.bits
        order = [offs[1], offs[2], offs[3], offs[0]]
        chans = [Chan(order[c], lay["colbytes"], lay["rowbytes"], sb, 8 * sb) for c in range(nc)]
        v = promote(pl) if case.promote else pl
        inp = Input(frame, chans, convert(v, case.bits, case.prec).astype(np.int32))
    inp.buf.setflags(write=False)
    inp.samples.setflags(write=False)
    _inputs[key] = inp
    while len(_inputs) > 24:
        _inputs.popitem(last=False)
    return inp


def plane_views(api, chans):
    """The j2k_hip_plane array of the channel views over the frame at device address d."""
    def at(d):
        arr = (api.Plane * len(chans))()
        for c, ch in enumerate(chans):
            arr[c].base, arr[c].colbytes, arr[c].rowbytes = d + ch.off, ch.colbytes, ch.rowbytes
            arr[c].sample_bits, arr[c].depth = 8 * ch.sample_bytes, ch.depth
        return arr
    return at


def tiles(case: Case):
    t = case.tile
    if not t:
        return [(0, 0, case.w, case.h)]
    return [(x, y, min(x + t, case.w), min(y + t, case.h)) for y in range(0, case.h, t) for x in range(0, case.w, t)]


# ------------------------------------------------------------------------------------------------ reference
def frontend_reference(oracle, case: Case) -> np.ndarray:
    """int32 words (float32 bit patterns for 9/7) of the front end's output, as test_frontend_matches_oracle composes it."""
    inp = make_input(case)
    src = inp.buf
    if case.promote:
        src = promote(inp.buf.view(np.uint16).astype(np.uint32)).astype(np.uint16).view(np.uint8)
    planes = [oracle.copy_channel(src, ch.off, case.w, case.h, ch.colbytes, ch.rowbytes, ch.sample_bytes, ch.depth, case.prec)
              for ch in inp.chans]
    ref = np.ascontiguousarray(np.stack(planes).astype(np.int32))
    ptrs = (C.POINTER(C.c_int32) * case.nc)(*[ref[c].ctypes.data_as(C.POINTER(C.c_int32)) for c in range(case.nc)])
    oracle.L.j2ko_dc_mct.argtypes = [C.POINTER(C.POINTER(C.c_int32)), C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int]
    oracle.L.j2ko_dc_mct(ptrs, case.nc, case.w * case.h, case.prec, int(case.rev), int(case.mct))
    return ref


_refs: OrderedDict = OrderedDict()


def reference(oracle, case: Case) -> np.ndarray:
    """(ncomp, H, W) int32 (5/3) or float32 (9/7): every tile's rectangle holds that tile-component's Mallat layout."""
    key = case._replace(name="")
    if key in _refs:
        _refs.move_to_end(key)
        return _refs[key]
    fe = frontend_reference(oracle, case)
    planes = fe if case.rev else fe.view(np.float32)
    out = np.empty_like(planes)
    f = oracle.dwt53 if case.rev else oracle.dwt97
    for (x0, y0, x1, y1) in tiles(case):
        for c in range(case.nc):
            out[c, y0:y1, x0:x1] = f(planes[c, y0:y1, x0:x1], case.levels, x0, y0)
    out.setflags(write=False)
    _refs[key] = out
    while len(_refs) > 48:
        _refs.popitem(last=False)
    return out


def _cd(a, l):
    return -(-a >> l)


def subband(case: Case, tile, lx, ly) -> str:
    x0, y0, x1, y1 = tile
    for l in range(1, case.levels + 1):
        wl, hl = _cd(x1, l) - _cd(x0, l), _cd(y1, l) - _cd(y0, l)
        if lx >= wl or ly >= hl:
            return ("HL" if ly < hl else ("LH" if lx < wl else "HH")) + str(l)
    return f"LL{case.levels}"


def difference(case: Case, kn: dict, got: np.ndarray, ref: np.ndarray, extra: str = "", origin=(0, 0)):
    """None when got equals ref bit for bit (the int32 view: -0.0 is not 0.0), else the message of the failure."""
    g, r = got.view(np.int32), ref.view(np.int32)
    if g.shape == r.shape and np.array_equal(g, r):
        return None
    if g.shape != r.shape:
        return f"{case.name} [{kid(kn)}] {extra}: shape {g.shape} against {r.shape}"
    bad = np.argwhere(g != r)
    c, y, x = (int(v) for v in bad[0])
    t = next(t for t in tiles(case) if t[0] <= x < t[2] and t[1] <= y < t[3])
    return (f"{case.name} [{kid(kn)}] {extra}: {len(bad)} of {g.size} words differ, first at (component {c}, y {y}, x {x}) in tile "
            f"{tiles(case).index(t)} {t}, sub-band {subband(case, (t[0] + origin[0], t[1] + origin[1], t[2] + origin[0], t[3] + origin[1]), x - t[0], y - t[1])}: got {got[c, y, x]!r} (0x{int(g[c, y, x]) & 0xffffffff:08x}), "
            f"reference {ref[c, y, x]!r} (0x{int(r[c, y, x]) & 0xffffffff:08x})")


# ------------------------------------------------------------------------------------------------ the GPU tests' calls
def _api():
    from j2k_amd import api
    return api


@contextlib.contextmanager
def knobs(kn: dict):
    """The tuning knobs of kn for the calls inside, the defaults again behind them."""
    api = _api()
    try:
        for k, v in kn.items():
            api.tune(k, v)
        yield
    finally:
        for k in kn:
            api.tune(k, DEFAULTS[k])


def run_hook(enc, case, kn, cuts=None, descending=False):
    api = _api()
    inp = make_input(case)
    p = api.make_params(case.w, case.h, case.nc, case.prec, reversible=case.rev, ycc=case.mct, promote=case.promote,
                        num_resolutions=case.levels + 1, tile_size=case.tile)
    with knobs(kn):
        return enc.stage_transform(inp.buf, plane_views(api, inp.chans), p, cuts, descending)


def check(oracle, enc, case, kn, cuts=None, descending=False):
    got = run_hook(enc, case, kn, cuts, descending)
    extra = "" if cuts is None else f"cuts {cuts} {'descending' if descending else 'ascending'}"
    msg = difference(case, kn, got, reference(oracle, case), extra)
    if msg:
        pytest.fail(msg, pytrace=False)


# ------------------------------------------------------------------------------------------------ launch model
Job = namedtuple("Job", "rw rh casx casy src_off ll_off z_off px0")
# waves_per_simd fallbacks of dwt.hip: fused_waves_per_simd (the code object's own value may differ: the model is asked
# with every value 1..8 where it matters)
FUSED_OCC = {(True, 1): 7, (True, 3): 5, (True, 4): 4, (False, 1): 6, (False, 3): 3, (False, 4): 3}


def is_fused(case: Case, kn: dict) -> bool:
    """encoder.cpp: fuse_frontend (make_frontend_args: interleaved needs rowbytes % pixel bytes == 0)."""
    if case.views != "ae" or kn.get("no_fuse", 0) or case.levels < 1:
        return False
    pix = 4 * case.bits // 8
    return (pix * case.w + case.pad) % pix == 0 and case.nc in (1, 3, 4)


def hook_jobs(case: Case, l: int, fused: bool):
    """prepare_geometry's job table of level l: one job per tile-component, or per tile for the fused level 1."""
    S = -(-case.w // 64) * 64
    plane = S * case.h
    jobs = []
    for (x0, y0, x1, y1) in tiles(case):
        for c in range(1 if fused and l == 0 else case.nc):
            ax0, ax1, ay0, ay1 = _cd(x0, l), _cd(x1, l), _cd(y0, l), _cd(y1, l)
            if ax1 - ax0 <= 0 or ay1 - ay0 <= 0:
                continue
            off = c * plane + y0 * S + x0
            jobs.append(Job(ax1 - ax0, ay1 - ay0, ax0 & 1, ay0 & 1, off, off, off, x0))
    return jobs, S, plane


def stage_dwt_jobs(w, h, l, x0, y0, nplanes):
    """j2k_hip_stage_dwt's job table: identical jobs, contiguous planes, stride = width."""
    ax0, ax1, ay0, ay1 = _cd(x0, l), _cd(x0 + w, l), _cd(y0, l), _cd(y0 + h, l)
    if ax1 - ax0 <= 0 or ay1 - ay0 <= 0:
        return []
    return [Job(ax1 - ax0, ay1 - ay0, ax0 & 1, ay0 & 1, c * w * h, c * w * h, c * w * h, 0) for c in range(nplanes)]


def _launch(jobs, pairs, wpb, ppc, xcd, aligned):
    valid, halo, ncol = (124, 1, 4) if pairs == 2 else (60, 2, 2)  # Geo<PAIRS>
    strips = []
    for j in jobs:
        npx = (j.rw + j.casx + 1) >> 1
        row = []
        for wv in range(-(-npx // valid)):  # (waves with k0 >= npx leave at once)
            first_i = 2 * (wv * valid - halo * pairs)
            row.append(pairs == 2 and j.casx == 0 and j.rh >= 16 and first_i >= 0 and first_i + 64 * ncol <= j.rw and
                       (((j.rw + 1) >> 1) & 1) == 0 and (j.rw & 1) == 0 and aligned(j, first_i))
        strips.append(row)
    max_rw, max_rh = max(j.rw for j in jobs), max(j.rh for j in jobs)
    npy = (max_rh + 2) >> 1
    chunks = -(-npy // ppc)
    rows = chunks * len(jobs)
    job_npy = [(j.rh + j.casy + 1) >> 1 for j in jobs]
    return dict(
        ppc=ppc, chunks=chunks, rows=rows, strips=strips,
        fast=any(any(r) for r in strips), edge=any(not all(r) for r in strips),
        wg_mixed=wpb == 4 and any(any(r[i:i + 4]) and not all(r[i:i + 4]) for r in strips for i in range(0, len(r), 4)),
        xcd_form=bool(xcd) and rows >= 8,                      # level_grid
        xcd_partial=bool(xcd) and rows >= 8 and rows % 8 != 0,  # block_map: m.valid false in the last group of eight
        short_last_chunk=any(n > ppc and n % ppc != 0 for n in job_npy),
        small_job=any(j.rw < max_rw and j.rh < max_rh for j in jobs))


def level_launch(jobs, kn: dict, src_stride: int):
    """launch_variant + dwt_level_kernel.  Pointers are taken as aligned (hipMalloc)."""
    k = dict(DEFAULTS, **kn)
    pairs = 1 if k["dwt_pairs"] == 1 else 2
    valid = 124 if pairs == 2 else 60
    npx, npy = (max(j.rw for j in jobs) + 2) >> 1, (max(j.rh for j in jobs) + 2) >> 1
    waves_x = -(-npx // valid)
    ppc = 128
    while ppc > 4 and waves_x * -(-npy // ppc) * len(jobs) < k["dwt_min_waves"]:
        ppc >>= 1
    if k["dwt_ppc"] > 0:
        ppc = k["dwt_ppc"]
    return _launch(jobs, pairs, 1, ppc, k["dwt_xcd"],
                   lambda j, fi: j.src_off % 4 == 0 and src_stride % 4 == 0 and j.ll_off % 2 == 0 and j.z_off % 2 == 0 and src_stride % 2 == 0)


def fused_variant(case: Case, kn: dict) -> str:
    """launch_fused: which of generic / GEN / SPEC1 / SPEC2 serves the case."""
    rs = case.bits - case.prec
    if (case.promote and case.bits == 16) or rs < 0:
        return "GEN"
    if rs == 0 and case.nc >= 3 and not dict(DEFAULTS, **kn)["fused_generic"]:  # (synth.ae_frame: R, G, B behind A)
        return "SPEC1" if case.bits == 16 else "SPEC2"
    return "generic"


def fused_launch(case: Case, kn: dict, occ: int | None = None):
    """launch_fused + dwt_fused_kernel for the level-1 launch of a fused case."""
    k = dict(DEFAULTS, **kn)
    jobs, S, plane = hook_jobs(case, 0, True)
    npx, npy = (max(j.rw for j in jobs) + 2) >> 1, (max(j.rh for j in jobs) + 2) >> 1
    waves_x = -(-npx // 124)
    slots = 1024 * (occ or FUSED_OCC[(case.rev, case.nc)])
    big = waves_x * -(-npy // 16) * len(jobs) >= 2 * slots
    wpb = (4 if k["fused_wpb"] > 1 else 1) if k["fused_wpb"] > 0 else (4 if big else 1)
    ppc = 16
    if big:
        ppc = 8
    else:
        best = 0.0
        for c in range(20, 9, -1):
            wv = waves_x * -(-npy // c) * len(jobs)
            fill = wv / (-(-wv // slots) * slots)
            if fill > best + 0.01:
                best, ppc = fill, c
        if best < 0.85:
            ppc = 16
            while ppc > 4 and waves_x * -(-npy // ppc) * len(jobs) < 2048:
                ppc >>= 1
    if k["fused_ppc"] > 0:
        ppc = k["fused_ppc"]
    pixb = 4 * case.bits // 8
    rowbytes = pixb * case.w + case.pad
    m = _launch(jobs, 2, wpb, ppc, k["dwt_xcd"],
                lambda j, fi: ((j.px0 + fi) * pixb) % 16 == 0 and rowbytes % 16 == 0 and j.ll_off % 2 == 0 and j.z_off % 2 == 0 and
                S % 2 == 0 and plane % 2 == 0)
    m.update(wpb=wpb, variant=fused_variant(case, kn))
    return m


def hook_launches(case: Case, kn: dict):
    """The model of every DWT launch of stage_transform(case) under the knobs, level 1 first."""
    fused = is_fused(case, kn)
    out = []
    for l in range(case.levels):
        if l == 0 and fused:
            out.append(fused_launch(case, kn))
        else:
            jobs, S, _ = hook_jobs(case, l, False)
            if jobs:
                out.append(level_launch(jobs, kn, S))
    return out


# ------------------------------------------------------------------------------------------------ the tables
def _name(**kw):
    return "-".join(f"{k}{v}" for k, v in kw.items())


def ae_case(w, h, nc, rev, mct, bits, prec, promote=False, pad=0, levels=1, tile=0):
    return Case(f"{w}x{h}{'+pad%d' % pad if pad else ''}{'/t%d' % tile if tile else ''}-{'53' if rev else '97'}-c{nc}{'m' if mct else ''}"
                f"-{bits}to{prec}{'p' if promote else ''}-L{levels}", w, h, nc, rev, mct, bits, prec, promote, pad, levels, tile, "ae")


def planar_case(w, h, nc, rev, mct, prec, pad=0, levels=1, tile=0):
    return Case(f"{w}x{h}{'+pad%d' % pad if pad else ''}{'/t%d' % tile if tile else ''}-{'53' if rev else '97'}-c{nc}{'m' if mct else ''}"
                f"-planar8,16to{prec}-L{levels}", w, h, nc, rev, mct, 0, prec, False, pad, levels, tile, "planar")


# --- fused kernel: sample formats.  (bits, prec, promote, fused_generic)
FORMATS = [(8, 8, False, 0), (8, 8, False, 1), (8, 10, False, 0), (8, 12, False, 0), (8, 16, False, 0),
           (16, 16, False, 0), (16, 16, False, 1), (16, 10, False, 0), (16, 12, False, 0), (16, 16, True, 0), (16, 12, True, 0)]
CHANNELS = [(1, False), (3, False), (3, True), (4, False), (4, True)]  # (channels, mct)
Fmt = namedtuple("Fmt", "rev nc mct bits prec promote generic")
FUSED_FORMATS = [Fmt(rev, nc, mct, *f) for rev in (True, False) for (nc, mct) in CHANNELS for f in FORMATS]
FUSED_KNOBS = [dict(fused_wpb=wpb, fused_ppc=ppc) for wpb in (1, 4) for ppc in (0, 1, 3, 8, 20)]


def fmt_id(f: Fmt) -> str:
    return f"{'53' if f.rev else '97'}-c{f.nc}{'m' if f.mct else ''}-{f.bits}to{f.prec}{'p' if f.promote else ''}{'-generic' if f.generic else ''}"


def fused_shapes(f: Fmt):
    """The frames one format is run on: (w, h, pad, tile, levels).  An untiled frame narrower or lower than 2^levels is
    refused by the encoder (as by the reference), so 1 x 40, 40 x 1 and their like appear as the edge tiles of small tiled
    frames -- 41 x 41 in tiles of 40 (1 x 40, 40 x 1, 1 x 1 at even origins), 11 x 13 in tiles of 8 (3 x 8, 8 x 5, 3 x 5),
    10 x 10 in tiles of 9 (1 x 9, 9 x 1, 1 x 1 at ODD origins: the doubled single sample of 5/3) -- and 2 x 2, 3 x 5
    untiled with the one level they admit."""
    pads = (4,) if f.bits == 8 else (4, 8)  # (ARGB64 with 4 bytes of padding is no interleaved frame: it runs unfused)
    shapes = []
    for levels in (1, 3):
        shapes += [(1016, 40, 0, 0, levels)] + [(1016, 40, p, 0, levels) for p in pads] + [(301, 37, 0, 0, levels)]
        shapes += [(41, 41, 0, 40, levels), (11, 13, 0, 8, levels), (10, 10, 0, 9, levels)]
    return shapes + [(2, 2, 0, 0, 1), (3, 5, 0, 0, 1)]


def fused_cases(f: Fmt):
    return [ae_case(w, h, f.nc, f.rev, f.mct, f.bits, f.prec, f.promote, pad, levels, tile) for (w, h, pad, tile, levels) in fused_shapes(f)]


def fused_knobs(f: Fmt, kn: dict) -> dict:
    return dict(kn, fused_generic=1) if f.generic else dict(kn)


# --- tiles: (w, h, tile) x num_resolutions 1..4 x a few formats, fused and unfused
TILE_FRAMES = [(301, 199, 64), (301, 199, 100), (301, 199, 75), (1100, 70, 512)]
TILE_FORMATS = [(3, True, 8, 8, False), (4, True, 16, 12, False), (1, False, 16, 16, True)]  # (nc, mct, bits, prec, promote)
TILE_MODES = {"fused": {}, "fused_wpb4": dict(fused_wpb=4), "no_fuse": dict(no_fuse=1)}


def tile_cases(rev):
    out = []
    for (w, h, t) in TILE_FRAMES:
        for levels in range(4):
            for (nc, mct, bits, prec, pr) in TILE_FORMATS:
                out.append(ae_case(w, h, nc, rev, mct, bits, prec, pr, 0, levels, t))
            out.append(planar_case(w, h, 3, rev, True, 12, 2, levels, t))  # channel views of unequal sample size: frontend.hip
            out.append(planar_case(w, h, 4, rev, False, 10, 0, levels, t))
    return out


# --- level kernel under its knobs.  dwt_ppc > 0 overrides the dwt_min_waves ladder, so the ladder values go with dwt_ppc = 0.
LEVEL_KNOBS = [dict(dwt_pairs=pairs, dwt_xcd=xcd, **k) for pairs in (1, 2) for xcd in (0, 1)
               for k in ([dict(dwt_ppc=p) for p in (1, 3, 7, 128)] + [dict(dwt_ppc=0, dwt_min_waves=m) for m in (1, 2048, 1 << 30)])]
# the ladder 128, 64, 32, 16, 8, 4 walked on 513 x 515 (3 planes): thresholds between the wave counts of neighbouring steps
LADDER_KNOBS = [dict(dwt_min_waves=m) for m in (1, 28, 60, 120, 220, 1 << 30)]
# test_gpu_parity.py's DWT list plus two with fast strips (1000 x 37: three; 748 x 33: two, the second ending at the edge)
DWT_SHAPES = [(64, 64, 1, 0, 0), (300, 200, 5, 0, 0), (301, 199, 3, 0, 0), (128, 128, 5, 128, 128), (97, 61, 4, 33, 7),
              (1, 40, 2, 0, 0), (40, 1, 2, 1, 1), (2, 2, 1, 1, 0), (3, 5, 2, 0, 1), (1000, 37, 5, 0, 0), (513, 515, 6, 0, 0), (748, 33, 2, 0, 0)]
DWT_PLANES = 3  # (with 3 jobs the (chunk, job) rows of most launches are no multiple of 8)
LEVEL_HOOK_CASES = [c for rev in (True, False) for c in
                    (ae_case(301, 199, 3, rev, True, 8, 8, False, 0, 3, 75), ae_case(1100, 70, 4, rev, True, 16, 12, False, 0, 3, 512),
                     planar_case(301, 199, 3, rev, True, 12, 2, 3, 100))]

# --- partitions
PARTITION_FRAMES = [(1016, 70, 0), (301, 199, 100)]


def partition_case(frame, rev):
    w, h, t = frame
    return ae_case(w, h, 3, rev, True, 8, 8, False, 0, 3, t)


def level_pairs(case: Case, l: int) -> int:
    """Row pairs of the tallest job of level l."""
    return max((j.rh + j.casy + 1) >> 1 for j in hook_jobs(case, l, False)[0])


def cut_sets(case: Case):
    n0 = level_pairs(case, 0)
    return {"every": [list(range(1, level_pairs(case, l))) for l in range(case.levels)],
            "first": [[1]], "last": [[n0 - 1]], "2,3,17": [[2, 3, 17]],
            "per-level": [[2, 3, 17], [1, 5, level_pairs(case, 1) - 1], [3]]}


# --- what the names claim (test_dwt_variant_refs.py holds the model to it): (case, knobs, claims).  A claim holds when one
# of the case's launches shows it; every (case, knobs) here is one that test_dwt_variants.py runs.
def claimed():
    def wide(pad=0):
        return ae_case(1016, 40, 3, True, True, 8, 8, False, pad, 1, 0)

    def wide64(pad=0):
        return ae_case(1016, 40, 4, False, True, 16, 16, False, pad, 3, 0)
    out = []
    for c in (wide(), wide64()):
        out += [(c, dict(fused_wpb=4, fused_ppc=3), {"is_fused", "fast", "edge", "wg_mixed", "short_last_chunk", "plain_grid"}),
                (c, dict(fused_wpb=4, fused_ppc=8), {"is_fused", "fast", "edge", "wg_mixed", "short_last_chunk", "plain_grid"}),
                (c, dict(fused_wpb=1, fused_ppc=1), {"is_fused", "fast", "edge", "xcd_partial"}),
                (c, dict(fused_wpb=4, fused_ppc=1), {"is_fused", "fast", "edge", "wg_mixed", "xcd_partial"})]
    out += [(wide(4), dict(fused_wpb=4, fused_ppc=0), {"no_fast", "edge", "is_fused"}),
            (wide64(8), dict(fused_wpb=4, fused_ppc=0), {"no_fast", "edge", "is_fused"}),
            (wide64(4), dict(fused_wpb=4, fused_ppc=0), {"not_fused", "fast", "edge"}),
            (ae_case(301, 37, 3, True, True, 8, 8, False, 0, 1, 0), dict(fused_wpb=1, fused_ppc=8), {"no_fast", "edge", "short_last_chunk"})]
    for t in (64, 100, 75):
        c = ae_case(301, 199, 3, True, True, 8, 8, False, 0, 3, t)
        more = ({"odd_origin"} if t == 75 else set()) | ({"xcd_partial"} if t != 100 else set())
        out += [(c, {}, {"small_job", "is_fused"} | more), (c, dict(no_fuse=1), {"small_job", "not_fused"} | more)]
    c = ae_case(1100, 70, 3, True, True, 8, 8, False, 0, 3, 512)
    out += [(c, dict(fused_wpb=4), {"fast", "edge", "wg_mixed", "is_fused"}), (c, dict(no_fuse=1), {"fast", "edge", "not_fused"})]
    out += [(planar_case(301, 199, 3, True, True, 12, 2, 3, 75), {}, {"not_fused", "small_job", "odd_origin", "xcd_partial"})]
    return out


def claim_facts(case: Case, kn: dict) -> set:
    ls = hook_launches(case, kn)
    facts = {k for k in ("fast", "edge", "wg_mixed", "xcd_partial", "short_last_chunk", "small_job") if any(m[k] for m in ls)}
    facts.add("is_fused" if is_fused(case, kn) else "not_fused")
    if not ls[0]["fast"]:  # (of the level-1 launch)
        facts.add("no_fast")
    if not ls[0]["xcd_form"]:  # (of the level-1 launch)
        facts.add("plain_grid")
    if any(j.casx and j.casy for j in hook_jobs(case, 0, False)[0]):
        facts.add("odd_origin")
    return facts
