#!/usr/bin/env python3
"""Layers at given slopes beside the search they replace: per-frame time of
  (a) layer_rates at one ratio,
  (b) layer_slopes at the thresholds (a) reported -- the same bytes, the hash is checked --
  (c) no rate control,
alternating in one process, one frame at a time and with three frames in flight, with ms_t2_host of each, for the metric
frame (8192 x 8192 RGB16 9/7) and for 2048 x 1080 and 512 x 512 frames; (b) with the cut on the device (the default) and on the
host (rate_dev = -1).  A library without the field (an earlier build: J2K_HIP_LIB) runs (a) and (c) alone.
usage: slopes_bench.py [--ratio R] [--rounds N] [--sizes WxH,WxH,...]   (output: stdout; kept as profiles/slopes.txt)"""
import argparse
import hashlib
import os
import statistics
import sys
import threading
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "24")  # one hardware queue per stream of the handles in flight (before HIP starts)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from j2k_amd import api, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ratio", type=float, default=20.0)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--sizes", default="8192x8192,2048x1080,512x512")
args = ap.parse_args()
HAVE = hasattr(api.Params, "layer_slopes") and hasattr(api.load_library(), "j2k_hip_encode_get_layer_slopes")


def med(v):
    return statistics.median(v), min(v), max(v)


def fmt(v):
    m, lo, hi = med(v)
    return f"{m:8.2f} ms (min {lo:.2f}, max {hi:.2f})"


for size in args.sizes.split(","):
    W, H = (int(x) for x in size.split("x"))
    pl = synth.planes(W, H, 3, 16, 23456)
    frame, lay = synth.ae_frame(pl, 16)
    del pl
    mk = lambda **how: api.make_params(W, H, 3, 16, reversible=False, ycc=True, num_resolutions=6, comment="", **how)
    enc = api.Encoder(0)
    d = enc.upload(frame)
    _, _, ref = enc.encode_device(d, lay, mk(rates=[args.ratio]))
    want = hashlib.sha256(ref).hexdigest()
    variants = [("a rates", mk(rates=[args.ratio]), 0), ("c none", mk(), 0)]
    if HAVE:
        slopes = enc.layer_slopes(0)
        variants[1:1] = [("b slopes, device", mk(slopes=slopes), 0), ("b slopes, host", mk(slopes=slopes), -1)]
        for name, p, rd in variants[1:3]:
            api.tune("rate_dev", rd)
            got = enc.encode_device(d, lay, p)[2]
            api.tune("rate_dev", 0)
            assert hashlib.sha256(got).hexdigest() == want, name
    print(f"== {W} x {H} RGB16 9/7, ratio {args.ratio:g}: {len(ref)} bytes, sha256 {want[:16]}, {enc.stats()['num_codeblocks']} code-blocks"
          + (f", thresholds {slopes}" if HAVE else " (library without layer_slopes)"), flush=True)
    # one frame at a time: the variants in turn, `rounds` times, two frames each time (the first discarded)
    times = {n: [] for n, _, _ in variants}
    t2 = {n: [] for n, _, _ in variants}
    for name, p, rd in variants:  # warm every path's arenas
        api.tune("rate_dev", rd)
        enc.encode_device(d, lay, p, download=False)
    for _ in range(args.rounds):
        for name, p, rd in variants:
            api.tune("rate_dev", rd)
            enc.encode_device(d, lay, p, download=False)
            t0 = time.perf_counter()
            enc.encode_device(d, lay, p, download=False)
            times[name].append((time.perf_counter() - t0) * 1e3)
            t2[name].append(enc.stats()["ms_t2_host"])
    api.tune("rate_dev", 0)
    for name, _, _ in variants:
        print(f"  one at a time   {name:18s} {fmt(times[name])}   ms_t2_host {fmt(t2[name])}", flush=True)
    # three frames in flight: three handles on three host threads, the variants in turn
    encs = [api.Encoder(0) for _ in range(3)]
    per = 4
    flight = {n: [] for n, _, _ in variants}
    for name, p, rd in variants:
        api.tune("rate_dev", rd)
        for e in encs:
            e.encode_device(d, lay, p, download=False)
    for _ in range(args.rounds):
        for name, p, rd in variants:
            api.tune("rate_dev", rd)

            def worker(e):
                for _ in range(per):
                    e.encode_device(d, lay, p, download=False)
            ths = [threading.Thread(target=worker, args=(e,)) for e in encs]
            t0 = time.perf_counter()
            for t in ths:
                t.start()
            for t in ths:
                t.join()
            flight[name].append((time.perf_counter() - t0) * 1e3 / (per * len(encs)))
    api.tune("rate_dev", 0)
    for name, _, _ in variants:
        print(f"  three in flight {name:18s} {fmt(flight[name])} per frame", flush=True)
    for e in encs:
        e.close()
    enc.free(d)
    enc.close()
