#!/usr/bin/env python3
"""What "verify after write" costs on the GPU (j2k_hip_compare_device) next to the decode it contains and to the host loop it
replaces, in one process:

  1. one 4096 x 2160 RGB 16-bit 9/7 frame, encoded here, its source frame resident on the device: j2k_hip_decode_device into
     device planes and j2k_hip_compare_device against the source, interleaved (decode, compare, decode, compare ...), the
     median call time of N calls each -- the difference is what the compare adds to the decode;
  2. the host alternative: j2k_hip_decode into host planes plus a numpy comparison (the source samples already converted:
     the front end's conversions on the host are not even counted);
  3. the reduction kernel alone (j2k_hip_stage_compare) at 8192 x 8192 x 3: dense 16-bit planes and an ARGB64 frame against
     16-bit decoded planes, achieved bytes per second (source bytes + decoded bytes over the call's wall time, results on the
     host included) next to j2k_hip_debug_membw's copy figures of the same run (bytes read + bytes written per second).

usage: compare_bench.py [calls-per-leg]      one JSON line per row, then a table"""
import ctypes as C
import json
import os
import sys
import time

_q = os.environ.get("GPU_MAX_HW_QUEUES", "")  # (as bench.py and the tests: the band-pipelined encode of the frame wants a queue per stream)
if not _q.isdigit() or int(_q) < 24:
    os.environ["GPU_MAX_HW_QUEUES"] = "24"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from j2k_amd import api, synth  # noqa: E402

W, H, PREC = 4096, 2160, 16
SW = SH = 8192


def median_ms(fn, n):
    runs = []
    for it in range(n + 1):  # (the first call grows the handle's buffers: not timed)
        t0 = time.perf_counter()
        fn()
        if it:
            runs.append((time.perf_counter() - t0) * 1e3)
    runs.sort()
    return runs[len(runs) // 2], runs[0]


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    enc = api.Encoder(0)
    L = enc.L
    rows = []

    # ---- 1 + 2: a file against its source frame
    planes = synth.planes(W, H, 3, PREC, 45678)
    frame, lay = synth.ae_frame(planes, PREC)
    p = api.make_params(W, H, 3, PREC, reversible=False, ycc=True, num_resolutions=6, comment="")
    cs = enc.encode_host(frame, lay, p)
    file = np.frombuffer(cs, dtype=np.uint8)
    d_frame = enc.upload(frame)
    d_out = enc.malloc(3 * W * H * 2)
    outp = (api.OutPlane * 3)()
    for c in range(3):
        api._set_outplane(outp[c], d_out + c * W * H * 2, 2, W * 2, 16, PREC, W, H)
    src_planes = api.planes_from_layout(d_frame, lay, 3)
    diffs = enc._diffs(3)

    def decode_device():
        enc._check(L.j2k_hip_decode_device(enc.h, file.ctypes.data, file.size, 1, outp, 3))

    def compare_device():
        enc._check(L.j2k_hip_compare_device(enc.h, C.byref(p), src_planes, file.ctypes.data, file.size, diffs, 3))

    host_out = np.zeros((3, H, W), np.uint16)
    host_result = {}

    def host_alternative():
        dec = enc.decode_planar(cs, out=host_out)
        res = []
        for c in range(3):
            e = dec[c].astype(np.int64) - planes[c]
            a = np.abs(e)
            nz = np.flatnonzero(e)
            res.append((int(nz.size), int(a.sum()), int((e * e).sum()), int(a.max()), int(nz[0]) if nz.size else 0))
        host_result["r"] = res

    for rep in (1, 2):
        for name, fn in (("decode_device", decode_device), ("compare_device", compare_device)):
            ms, best = median_ms(fn, N)
            rows.append(dict(leg=name, repeat=rep, ms_call=round(ms, 3), ms_min=round(best, 3)))
            print(json.dumps(rows[-1]), flush=True)
    got = [d.as_dict() for d in diffs]
    ms, best = median_ms(host_alternative, max(3, N // 3))
    rows.append(dict(leg="decode to host + numpy", repeat=1, ms_call=round(ms, 3), ms_min=round(best, 3)))
    print(json.dumps(rows[-1]), flush=True)
    for c in range(3):  # (a bench that measured a wrong compare would mislead)
        n, sa, sq, mx, first = host_result["r"][c]
        assert (got[c]["differing"], got[c]["sum_abs"], got[c]["sum_sq"], got[c]["max_abs"]) == (n, sa, sq, mx), (c, got[c], host_result["r"][c])
        assert (got[c]["first_x"], got[c]["first_y"]) == (first % W, first // W)
    print(json.dumps(dict(psnr_db=[round(d["psnr"], 3) for d in got], file_mb=round(len(cs) / 1e6, 2))), flush=True)
    enc.free(d_frame)
    enc.free(d_out)
    del frame, planes, host_out

    # ---- 3: the reduction kernel alone
    rng = np.random.default_rng(1)
    n = SW * SH
    ps = api.make_params(SW, SH, 3, 16)
    src = rng.integers(0, 65536, size=3 * n, dtype=np.uint16)
    dec = src.copy()
    dec[::97] ^= 1  # (every workgroup meets a difference and goes through its atomics)
    per_comp = [len(range((-c * n) % 97, n, 97)) for c in range(3)]
    d_src, d_dec = enc.upload(src), enc.upload(dec)
    planar = (api.Plane * 3)()
    for c in range(3):
        planar[c].base, planar[c].colbytes, planar[c].rowbytes, planar[c].sample_bits, planar[c].depth = d_src + c * n * 2, 2, SW * 2, 16, 16
    stage = []

    def run_stage(name, planes_arr, decoded, nbytes):
        def call():
            enc._check(L.j2k_hip_stage_compare(enc.h, C.byref(ps), planes_arr, decoded, diffs, 3))
        ms, best = median_ms(call, N)
        row = dict(leg=name, ms_call=round(ms, 4), ms_min=round(best, 4), gbytes_per_s=round(nbytes / (ms * 1e6), 1), gbytes_per_s_best=round(nbytes / (best * 1e6), 1))
        print(json.dumps(row), flush=True)
        stage.append(row)

    run_stage("stage planar16 x3, 1 in 97 differs", planar, d_dec, 2 * 3 * n * 2)
    assert [d.differing for d in diffs] == per_comp and [d.sum_sq for d in diffs] == per_comp, ([d.differing for d in diffs], per_comp)
    run_stage("stage planar16 x3, identical", planar, d_src, 2 * 3 * n * 2)
    assert all(d.differing == 0 for d in diffs)
    enc.free(d_src)
    del src
    # an ARGB64 frame: R, G, B of the same values out of interleaved pixels (four samples are loaded, three compared)
    argb = np.zeros((n, 4), np.uint16)
    for c in range(3):
        argb[:, c + 1] = dec[c * n:(c + 1) * n]
    d_argb = enc.upload(argb)
    inter = api.planes_from_layout(d_argb, dict(sample_bytes=2, colbytes=8, rowbytes=8 * SW, channel_offsets=(0, 2, 4, 6)), 3)
    run_stage("stage ARGB64, identical", inter, d_dec, n * 8 + 3 * n * 2)
    assert all(d.differing == 0 for d in diffs)
    enc.free(d_argb)
    enc.free(d_dec)
    bw = {}
    for mode in (0, 2, 4):
        g = C.c_double()
        enc._check(L.j2k_hip_debug_membw(enc.h, 3 * SW, SH, 0, mode, 20, C.byref(g)))
        bw[mode] = round(g.value, 1)
    print(json.dumps(dict(membw_copy_gbytes_per_s=bw)), flush=True)

    dec_ms = [r["ms_call"] for r in rows if r["leg"] == "decode_device"]
    cmp_ms = [r["ms_call"] for r in rows if r["leg"] == "compare_device"]
    print(f"\n{W} x {H} RGB{PREC} 9/7 5 levels, {len(cs) / 1e6:.2f} MB, source frame on the device, median of {N} calls per leg, two repeats")
    print(f"  j2k_hip_decode_device            {dec_ms[0]:8.3f}  {dec_ms[1]:8.3f} ms")
    print(f"  j2k_hip_compare_device           {cmp_ms[0]:8.3f}  {cmp_ms[1]:8.3f} ms   (+{cmp_ms[0] - dec_ms[0]:.3f}, +{cmp_ms[1] - dec_ms[1]:.3f} ms)")
    print(f"  j2k_hip_decode to host + numpy   {rows[-1]['ms_call']:8.3f} ms")
    print(f"  PSNR per component: {[round(d['psnr'], 3) for d in got]} dB")
    print(f"{SW} x {SH} x 3 reduction alone (j2k_hip_stage_compare, wall time of the call):")
    for r in stage:
        print(f"  {r['leg']:<38} {r['ms_call']:8.4f} ms  {r['gbytes_per_s']:7.1f} GB/s  (best {r['gbytes_per_s_best']:7.1f})")
    print(f"  j2k_hip_debug_membw copy of {3 * SW} x {SH} floats, read + written: mode 0 {bw[0]} GB/s, mode 2 {bw[2]} GB/s, mode 4 {bw[4]} GB/s")
    enc.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
