#!/usr/bin/env python3
"""What a code-block style costs or saves on the metric frame (8192 x 8192 RGB16, 9/7, 5 levels, resident in HBM): the frame is
encoded one at a time on one handle, then with three frames in flight (three handles, a thread each, as bench.py does), under
styles 0, bypass, bypass|termall and bypass|reset|termall.  Per style: ms_t1 and ms_total of a frame alone, the decisions and
the bytes of the file, and the frames-in-flight rate.

usage: style_bench.py [size] [frames per leg]        every style runs in a child process of its own under `timeout`
       style_bench.py --one STYLE [size] [frames]    one style, in this process: one JSON line"""
import json
import os
import subprocess
import sys
import threading
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "24")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STYLES = [0, 1, 1 | 4, 1 | 2 | 4]
STEP_SECONDS = 240  # per style: synthesis of the frame (~20 s), a dozen encodes, margin


def one(style: int, S: int, N: int) -> dict:
    import ctypes as C
    from j2k_amd import api, synth
    frame, lay = synth.ae_frame(synth.planes(S, S, 3, 16, 23456), 16)
    p = api.make_params(S, S, 3, 16, reversible=False, ycc=True, num_resolutions=6, comment="", cblk_style=style)
    encs = [api.Encoder(0) for _ in range(3)]
    d = encs[0].upload(frame)
    del frame
    res = dict(style=style)
    # a frame at a time
    t1, tot = [], []
    for i in range(N + 2):
        _, n, _ = encs[0].encode_device(d, lay, p, download=False)
        st = encs[0].stats()
        if i >= 2:
            t1.append(st["ms_t1"]); tot.append(st["ms_total"])
    res.update(ms_t1=round(sorted(t1)[len(t1) // 2], 3), ms_total=round(sorted(tot)[len(tot) // 2], 3), num_symbols=int(st["num_symbols"]),
               codestream_bytes=int(st["codestream_bytes"]))
    # three frames in flight
    planes = api.planes_from_layout(d, lay, 3)

    def worker(e, count):
        dptr, n = C.c_void_p(), C.c_size_t()
        for _ in range(count):
            e._check(e.L.j2k_hip_encode_device(e.h, C.byref(p), planes, C.byref(dptr), C.byref(n), None, 0))
    for count in (2, N):  # warm-up, then the timed leg
        ths = [threading.Thread(target=worker, args=(e, count)) for e in encs]
        t0 = time.perf_counter()
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        dt = time.perf_counter() - t0
    res.update(inflight3_ms_per_frame=round(dt * 1e3 / (3 * N), 3), inflight3_mpix_s=round(3 * N * S * S / dt / 1e6, 1))
    encs[0].free(d)
    for e in encs:
        e.close()
    return res


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        style = int(sys.argv[2])
        S = int(sys.argv[3]) if len(sys.argv) > 3 else 8192
        N = int(sys.argv[4]) if len(sys.argv) > 4 else 8
        print(json.dumps(one(style, S, N)), flush=True)
        return 0
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    print("style  ms_t1  ms_total  num_symbols  codestream_bytes  3 in flight: ms/frame  Mpixel/s", flush=True)
    for style in STYLES:
        # a fresh process per style, each under its own time limit; the first one that fails ends the run
        r = subprocess.run(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--one", str(style), str(S), str(N)],
                           stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            print(f"style {style}: exit status {r.returncode}; stopping", flush=True)
            return r.returncode
        m = json.loads(r.stdout.strip().splitlines()[-1])
        print(f"{style:5d}  {m['ms_t1']:.3f}  {m['ms_total']:.3f}  {m['num_symbols']}  {m['codestream_bytes']}  {m['inflight3_ms_per_frame']:.3f}  {m['inflight3_mpix_s']:.1f}",
              flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
