#!/usr/bin/env python3
"""What the cinema colour front end (j2k_hip_params.rgb_to_xyz) costs, in one process: one 4096 x 2160 ARGB64 frame resident
on the device, dci_profile = 4, encoded through j2k_hip_encode_device with

  xyz0          rgb_to_xyz = 0: the front end fused into the level-1 DWT kernel (ms_frontend ~ 0, its work is in ms_dwt)
  xyz0_unfused  rgb_to_xyz = 0 with the knob no_fuse = 1: frontend_kernel as a pass of its own -- the same bytes as the
                X'Y'Z' kernel moves, without the tables and the threshold search
  xyz1          rgb_to_xyz = 1: frontend_xyz_kernel as a pass of its own, then the unfused level 1

alternating in one loop (xyz0, xyz0_unfused, xyz1, xyz0, ...) after a warm-up round.  The times are the call's own device
events (j2k_hip_stats: ms_frontend brackets the front-end pass, ms_dwt the DWT launches) and its wall time ms_total, which
ends in the call's synchronise; medians with the spread (min .. max) of N calls per variant.  For the front-end kernels alone:
algorithmic bytes (8 B read + 12 B written per pixel) over ms_frontend.

--parent-lib PATH: the rgb_to_xyz = 0 figures again from another build of the library (the parent commit's), measured in a
child process started with J2K_HIP_LIB=PATH; nothing on that path changed, so they must agree within the spread.

usage: xyz_bench.py [calls-per-variant] [--parent-lib PATH] [--plain-only]      JSON lines, then a table"""
import json
import os
import subprocess
import sys

_q = os.environ.get("GPU_MAX_HW_QUEUES", "")  # (as bench.py and the tests)
if not _q.isdigit() or int(_q) < 24:
    os.environ["GPU_MAX_HW_QUEUES"] = "24"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from j2k_amd import api, synth  # noqa: E402

W, H = 4096, 2160
KEYS = ("ms_frontend", "ms_dwt", "ms_t1", "ms_total")


def summary(runs):
    out = {}
    for k in KEYS:
        v = sorted(r[k] for r in runs)
        out[k] = dict(median=round(v[len(v) // 2], 4), min=round(v[0], 4), max=round(v[-1], 4))
    return out


def measure(n, plain_only):
    enc = api.Encoder(0)
    planes = synth.planes(W, H, 3, 16, 24680)
    frame, lay = synth.ae_frame(planes, 16)
    d = enc.upload(frame)
    variants = [("xyz0", dict(), 0), ("xyz0_unfused", dict(), 1)]
    if not plain_only:
        variants.append(("xyz1", dict(rgb_to_xyz=1), 0))
    params = {name: api.make_params(W, H, 3, 12, num_resolutions=7, dci_profile=4, comment="", **kw) for name, kw, _ in variants}
    runs = {name: [] for name, _, _ in variants}
    sizes = {}
    for it in range(n + 1):  # (round 0 grows the handle's buffers and uploads the tables: not counted)
        for name, _, no_fuse in variants:
            api.tune("no_fuse", no_fuse)
            try:
                _, length, _ = enc.encode_device(d, lay, params[name], download=False)
            finally:
                api.tune("no_fuse", 0)
            st = enc.stats()
            assert st["bands"] == 0
            sizes[name] = length
            if it:
                runs[name].append({k: st[k] for k in KEYS})
    enc.free(d)
    enc.close()
    return {name: dict(summary(r), codestream_bytes=sizes[name]) for name, r in runs.items()}


def main():
    args = sys.argv[1:]
    parent = None
    if "--parent-lib" in args:
        i = args.index("--parent-lib")
        parent = args[i + 1]
        del args[i:i + 2]
    plain_only = "--plain-only" in args
    args = [a for a in args if a != "--plain-only"]
    n = int(args[0]) if args else 15
    res = measure(n, plain_only)
    px = W * H
    for name, r in res.items():
        row = dict(variant=name, lib=os.path.basename(api.LIBPATH), calls=n, **r)
        if name != "xyz0":
            row["frontend_gbytes_per_s"] = round(20.0 * px / (r["ms_frontend"]["median"] * 1e6), 1)
        print(json.dumps(row), flush=True)
    if plain_only:
        return 0
    if parent:
        child = subprocess.run([sys.executable, os.path.abspath(__file__), str(n), "--plain-only"], env=dict(os.environ, J2K_HIP_LIB=parent),
                               capture_output=True, text=True, timeout=600)
        sys.stdout.write(child.stdout)
        if child.returncode != 0:
            sys.stdout.write(child.stderr[-2000:])
            return 1
    print(f"\n{W} x {H} ARGB64 on the device, dci_profile 4, j2k_hip_encode_device, median (min .. max) of {n} calls per variant, ms")
    for name, r in res.items():
        cells = "  ".join(f"{k[3:]} {r[k]['median']:8.3f} ({r[k]['min']:.3f} .. {r[k]['max']:.3f})" for k in KEYS)
        print(f"  {name:<13} {cells}")
    for name in ("xyz0_unfused", "xyz1"):
        if name in res:
            ms = res[name]["ms_frontend"]["median"]
            print(f"  {name}: front-end kernel alone {ms:.3f} ms = {20.0 * px / (ms * 1e6):.0f} GB/s of algorithmic bytes (8 B read + 12 B written per pixel)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
