#!/usr/bin/env python3
"""A sequence to a byte budget beside the calls it is made of.  Per workload -- F frames of W x H RGB16
9/7, noisy and near-flat frames in turn, the total a twentieth of the raw size, without and with a frame cap at 1.5 x the
mean -- the legs, alternating in one process, medians of five:
  (a) j2k_hip_encode_sequence_budget_device;
  (b) j2k_hip_encode_sequence_device under layer_slopes at the thresholds (a) found, one call per run of frames with one
      threshold -- the same bytes, the hashes are checked; (a) - (b) is the whole cost of the search;
  (c) j2k_hip_encode_sequence_device under layer_rates at the same total split evenly;
with curve_launches and exact_plans of (a), and the PSNR minimum, mean and spread over the frames of (a) and (c).
usage: budget_bench.py [--rounds N] [--work WxH:F,WxH:F]   (output: stdout; kept as profiles/sequence_budget.txt)
       budget_bench.py --curve-only   (one workload, the budget call alone a few times: for a kernel trace of rate_curve_kernel)"""
import argparse
import hashlib
import math
import os
import statistics
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "24")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from j2k_amd import api, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--work", default="2048x1080:24,4096x2160:8")
ap.add_argument("--curve-only", action="store_true")
args = ap.parse_args()


def fmt(v):
    return f"{statistics.median(v):8.2f} ms (min {min(v):.2f}, max {max(v):.2f})"


def psnr(diffs, prec=16):
    sq, n = sum(d["sum_sq"] for d in diffs), sum(d["samples"] for d in diffs)
    return math.inf if sq == 0 else 10 * math.log10(((1 << prec) - 1) ** 2 / (sq / n))


def runs(index):
    """[(first, end, index)] of neighbouring frames with one index."""
    out, a = [], 0
    for f in range(1, len(index) + 1):
        if f == len(index) or index[f] != index[a]:
            out.append((a, f, index[a]))
            a = f
    return out


print(f"GPU_MAX_HW_QUEUES={os.environ['GPU_MAX_HW_QUEUES']} (one hardware queue per stream of the handle: the timings below depend on it), "
      f"medians of {args.rounds}", flush=True)
for work in args.work.split(","):
    size, F = work.split(":")
    W, H = (int(x) for x in size.split("x"))
    F = int(F)
    mk = lambda **how: api.make_params(W, H, 3, 16, reversible=False, ycc=True, num_resolutions=6, comment="", **how)
    enc = api.Encoder(0)
    try:
        frames, dptrs, lay = [], [], None
        for f in range(F):
            fr, lay = synth.ae_frame(synth.planes(W, H, 3, 16, 1000 + f, "A" if f % 3 == 0 else "B"), 16)
            frames.append(fr)
            dptrs.append(enc.upload(fr))
        raw = W * H * 3 * 2
        total = F * raw // 20
        for capped in (False, True):
            frame_max = 3 * (total // F) // 2 if capped else 0
            files, index, res = enc.encode_sequence_budget_device(dptrs, lay, mk(), total, frame_max)
            want = [hashlib.sha256(x).hexdigest() for x in files]
            print(f"== {F} frames of {W} x {H} RGB16 9/7, total {total} bytes" + (f", frame cap {frame_max}" if capped else "") +
                  f": {sum(len(x) for x in files)} bytes written, indices {sorted(set(index))}, {res}", flush=True)
            if args.curve_only:
                for _ in range(3):
                    enc.encode_sequence_budget_device(dptrs, lay, mk(), total, frame_max, download=False)
                continue
            legs_b = [(a, b, mk(slopes=[api.slope_grid(c)])) for a, b, c in runs(index)]
            got = []
            for a, b, p in legs_b:
                got += [hashlib.sha256(x[2]).hexdigest() for x in enc.encode_sequence_device(dptrs[a:b], lay, p)]
            assert got == want, "the slopes calls do not write the budget call's files"
            rated = [x[2] for x in enc.encode_sequence_device(dptrs, lay, mk(rates=[20.0]))]
            ta, tb, tc = [], [], []
            for _ in range(args.rounds):
                t0 = time.perf_counter()
                enc.encode_sequence_budget_device(dptrs, lay, mk(), total, frame_max, download=False)
                ta.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                for a, b, p in legs_b:
                    enc.encode_sequence_device(dptrs[a:b], lay, p, download=False)
                tb.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                enc.encode_sequence_device(dptrs, lay, mk(rates=[20.0]), download=False)
                tc.append((time.perf_counter() - t0) * 1e3)
            print(f"  (a) budget call                    {fmt(ta)}")
            print(f"  (b) slopes at (a)'s thresholds     {fmt(tb)}   in {len(legs_b)} call(s)")
            print(f"  (c) layer_rates, even split        {fmt(tc)}")
            print(f"  (a) - (b), the search              {statistics.median(ta) - statistics.median(tb):8.2f} ms: {res['curve_launches']} curve launches, {res['exact_plans']} exact plans beyond one per frame")
            for name, fs in (("(a)", files), ("(c)", rated)):
                q = [psnr(enc.compare(fs[f], mk(), frame=frames[f], layout=lay)) for f in range(F)]
                print(f"  PSNR {name}: min {min(q):.2f} mean {statistics.mean(q):.2f} spread {max(q) - min(q):.2f} dB; bytes min {min(len(x) for x in fs)} max {max(len(x) for x in fs)} sum {sum(len(x) for x in fs)}", flush=True)
    except api.J2kHipError as x:
        print(f"== {F} frames of {W} x {H}: not run ({x})", flush=True)
    finally:
        enc.close()
