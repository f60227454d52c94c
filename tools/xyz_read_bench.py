#!/usr/bin/env python3
"""What reading a cinema frame as R'G'B' costs (j2k_hip_decode_set_xyz_to_rgb), in one process: one 4096 x 2160 12-bit X'Y'Z'
frame (dci_profile = 4, rgb_to_xyz = 1, encoded here by the library itself) decoded through j2k_hip_decode_rgba_device into a
packed A,R,G,B frame resident on the device, with

  off   xyz_to_rgb = 0: the plain RGBA pass (one depth conversion per channel)
  on    xyz_to_rgb = 1: table, matrix and threshold search per pixel

alternating in one loop (off, on, off, ...) after a warm-up round, for an 8-bit destination (ARGB32: both tables in LDS) and
a 16-bit one (ARGB64: both tables in global memory).  Per variant: the call's wall time, and the output kernel alone
(j2k_hip_stats.ms_frontend: the device events around the call's last launch); medians with the spread (min .. max) of N calls.
For the kernel alone: algorithmic bytes (12 B read + 4 or 8 B written per pixel) over its time.

--parent-lib PATH: the `off` figures again from another build of the library (the parent commit's, which has no setting),
measured TWICE in child processes started with J2K_HIP_LIB=PATH -- the two runs show the box's run-to-run spread -- and then
the `off` figures of this build once more in a child of its own.  Nothing on the off path changed, so they must agree within
that spread.

usage: xyz_read_bench.py [calls-per-variant] [--parent-lib PATH] [--off-only]      JSON lines, then a table"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

_q = os.environ.get("GPU_MAX_HW_QUEUES", "")  # (as bench.py and the tests)
if not _q.isdigit() or int(_q) < 24:
    os.environ["GPU_MAX_HW_QUEUES"] = "24"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from j2k_amd import api, synth  # noqa: E402

W, H = 4096, 2160
KEYS = ("ms_call", "ms_output")


def summary(runs):
    out = {}
    for k in KEYS:
        v = sorted(r[k] for r in runs)
        out[k] = dict(median=round(v[len(v) // 2], 4), min=round(v[0], 4), max=round(v[-1], 4))
    return out


def measure(n, off_only):
    enc = api.Encoder(0)
    planes = synth.planes(W, H, 3, 16, 24680)
    frame, lay = synth.ae_frame(planes, 16)
    cs = enc.encode_host(frame, lay, api.make_params(W, H, 3, 12, num_resolutions=7, dci_profile=4, comment="", rgb_to_xyz=1))
    buf = np.frombuffer(cs, dtype=np.uint8)
    can_set = hasattr(enc.L, "j2k_hip_decode_set_xyz_to_rgb")
    variants = [("off", 0)] + ([] if off_only or not can_set else [("on", 1)])
    results = {}
    for bits in (8, 16):
        sb = bits // 8
        d = enc.upload(np.zeros(W * H * 4 * sb, dtype=np.uint8))
        dst = api.RgbaDst()
        dst.struct_size = C.sizeof(api.RgbaDst)
        for p, slot in ((dst.a, 0), (dst.r, 1), (dst.g, 2), (dst.b, 3)):
            p.base, p.colbytes, p.rowbytes = d + slot * sb, 4 * sb, W * 4 * sb
            p.sample_bits, p.depth, p.width, p.height = bits, bits, W, H
        runs = {name: [] for name, _ in variants}
        for it in range(n + 1):  # (round 0 grows the handle's buffers and uploads the tables: not counted)
            for name, target in variants:
                if can_set:
                    enc.set_xyz_to_rgb(target)
                t0 = time.perf_counter()
                rc = enc.L.j2k_hip_decode_rgba_device(enc.h, buf.ctypes.data, len(cs), 1, None, C.byref(dst))
                t1 = time.perf_counter()
                if rc != 0:
                    raise SystemExit(f"{name}: status {rc}: {enc.L.j2k_hip_last_error(enc.h).decode()}")
                if it:
                    runs[name].append(dict(ms_call=(t1 - t0) * 1e3, ms_output=enc.stats()["ms_frontend"]))
        enc.free(d)
        for name, _ in variants:
            results[f"{name}{bits}"] = summary(runs[name])
    if can_set:
        enc.set_xyz_to_rgb(0)
    enc.close()
    return dict(lib=os.environ.get("J2K_HIP_LIB", "in-tree"), calls=n, file_bytes=len(cs), variants=results)


def child(n, lib):
    env = dict(os.environ)
    if lib:
        env["J2K_HIP_LIB"] = lib
    out = subprocess.run([sys.executable, os.path.abspath(__file__), str(n), "--off-only", "--json"], env=env, check=True,
                         capture_output=True, text=True, timeout=600).stdout
    return json.loads(out.strip().splitlines()[-1])


def main():
    args = sys.argv[1:]
    n = int(args[0]) if args and args[0].isdigit() else 15
    parent = args[args.index("--parent-lib") + 1] if "--parent-lib" in args else None
    res = measure(n, "--off-only" in args)
    print(json.dumps(res), flush=True)
    if "--json" in args:
        return
    rows = [("this build", res)]
    if parent:  # (each in a fresh process, one after the other: this process's handle is closed)
        for label in ("parent, run 1", "parent, run 2"):
            rows.append((label, child(n, parent)))
            print(json.dumps(rows[-1][1]), flush=True)
        rows.append(("this build, off only", child(n, None)))
        print(json.dumps(rows[-1][1]), flush=True)
    print(f"\n# {W} x {H} x 3, 12-bit X'Y'Z', dci_profile 4, {res['file_bytes']} bytes; {n} calls per variant; ms: median (min .. max)")
    print(f"{'':24s}{'variant':8s}{'call':>28s}{'output kernel':>28s}{'GB/s':>8s}")
    for label, r in rows:
        for name, s in r["variants"].items():
            bits = 8 if name.endswith("8") else 16
            gbs = W * H * (12 + 4 * bits // 8) / (s["ms_output"]["median"] * 1e6)
            cell = lambda k: f"{s[k]['median']:9.3f} ({s[k]['min']:.3f} .. {s[k]['max']:.3f})"
            print(f"{label:24s}{name:8s}{cell('ms_call'):>28s}{cell('ms_output'):>28s}{gbs:8.0f}")


if __name__ == "__main__":
    main()
