"""Decode of bench.py's decode-leg frame into a packed 16-bit A,R,G,B device frame: j2k_hip_decode_device (three strided
channel stores per pixel) beside j2k_hip_decode_rgba_device (one 8-byte store per pixel, alpha filled), each with the output
stage's own device time (j2k_hip_stats.ms_frontend: the events around the last launch).

    python tools/rgba_read_time.py [--size 8192] [--runs 12] [--warmup 3] [--demote]

The frame is bench.py --full's: size x size, three 16-bit components, 9/7 with the component transform, 6 resolutions, seed
23456, encoded here by the library itself.  Run it on the parent commit too (a library without the RGBA entry points: only
the planar line is printed) -- the baseline of the comparison is the parent, never the code under test.  One line per call:
median, min and max of the wall time of `runs` calls after `warmup`, and the same of the output stage's device time."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # (behind PYTHONPATH: another build's package wins)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "24")  # as bench.py and the tests set it

from j2k_amd import api, synth  # noqa: E402


def spread(v):
    return f"median {statistics.median(v):8.3f}  min {min(v):8.3f}  max {max(v):8.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--demote", action="store_true", help="the RGBA call with demote_ae16")
    args = ap.parse_args()
    S, prec = args.size, 16
    e = api.Encoder(0)
    pl = synth.planes(S, S, 3, prec, 23456)
    frame, lay = synth.ae_frame(pl, prec)
    cs = e.encode_host(frame, lay, api.make_params(S, S, 3, prec, reversible=False, ycc=True, num_resolutions=6, comment=""))
    buf = np.frombuffer(cs, dtype=np.uint8)
    d = e.upload(np.zeros(frame.nbytes, dtype=np.uint8))
    offs = lay["channel_offsets"]  # A,R,G,B

    def outplane(p, off):
        p.base, p.colbytes, p.rowbytes = d + off, lay["colbytes"], lay["rowbytes"]
        p.sample_bits, p.depth, p.width, p.height = 16, 16, S, S

    planes = (api.OutPlane * 3)()
    for c in range(3):
        outplane(planes[c], offs[1 + c])
    calls = [("j2k_hip_decode_device      (R, G, B: three 2-byte stores per pixel)",
              lambda: e.L.j2k_hip_decode_device(e.h, buf.ctypes.data, len(cs), 1, planes, 3))]
    if hasattr(api, "RgbaDst"):
        dst = api.RgbaDst()
        dst.struct_size, dst.demote_ae16 = C.sizeof(api.RgbaDst), int(args.demote)
        for p, off in ((dst.r, offs[1]), (dst.g, offs[2]), (dst.b, offs[3]), (dst.a, offs[0])):
            outplane(p, off)
        calls.append(("j2k_hip_decode_rgba_device (A, R, G, B: one 8-byte store per pixel" + (", Demote" if args.demote else "") + ")",
                      lambda: e.L.j2k_hip_decode_rgba_device(e.h, buf.ctypes.data, len(cs), 1, None, C.byref(dst))))
    print(f"# {S} x {S} x 3, 16 bit, 9/7 + ICT, {len(cs)} bytes; {args.runs} runs after {args.warmup}; times in ms")
    frames = []
    for name, call in calls:
        wall, stage = [], []
        for i in range(args.warmup + args.runs):
            t0 = time.perf_counter()
            rc = call()
            t1 = time.perf_counter()
            if rc != 0:
                raise SystemExit(f"{name}: status {rc}: {e.L.j2k_hip_last_error(e.h).decode()}")
            if i >= args.warmup:
                wall.append((t1 - t0) * 1e3)
                stage.append(e.stats()["ms_frontend"])
        print(f"{name}\n    call         {spread(wall)}\n    output stage {spread(stage)}")
        frames.append(e.d2h(d, frame.nbytes).view(np.uint16).reshape(S, S, 4))
    if len(frames) == 2 and not args.demote:  # the same R, G, B, and a full-scale A
        print("R, G, B equal:", bool(np.array_equal(frames[0][:, :, 1:], frames[1][:, :, 1:])), " A == 65535:", bool((frames[1][:, :, 0] == 65535).all()))
    e.free(d)
    e.close()


if __name__ == "__main__":
    main()
