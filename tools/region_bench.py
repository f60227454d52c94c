#!/usr/bin/env python3
"""What a region decode saves on the metric frame (8192 x 8192 RGB16, 9/7, 5 levels, encoded in this process): the full
decode (j2k_hip_decode) and, beside it in the same run, windows of 512^2, 1024^2, 2048^2 and of the whole image through
j2k_hip_decode_region, each at the centre and at the top-left corner, into planar host channels of the window's size that
are kept from call to call.  Per row: the median call time of the repeats, the stage times of the median call's
j2k_hip_stats and num_codeblocks.  The yardstick is the full decode of the same file in the same process.

usage: region_bench.py [size] [repeats]      one JSON line per row, then a table"""
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "24")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from j2k_amd import api, synth  # noqa: E402


def main():
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    enc = api.Encoder(0)
    frame, lay = synth.ae_frame(synth.planes(S, S, 3, 16, 23456), 16)
    p = api.make_params(S, S, 3, 16, reversible=False, ycc=True, num_resolutions=6, comment="")
    cs = enc.encode_host(frame, lay, p)
    del frame
    rows = []

    def leg(label, rect):
        out, runs = None, []
        for it in range(N + 1):  # (the first call allocates the destination and grows the handle's buffers: not timed)
            t0 = time.perf_counter()
            out = enc.decode_planar(cs, out=out) if rect is None else enc.decode_region_planar(cs, rect, out=out)
            ms = (time.perf_counter() - t0) * 1e3
            if it:
                runs.append((ms, enc.stats()))
        runs.sort(key=lambda r: r[0])
        ms, st = runs[len(runs) // 2]
        row = dict(window=label, rect=rect, ms_call=round(ms, 2), ms_min=round(runs[0][0], 2), ms_t2_host=round(st["ms_t2_host"], 2),
                   ms_upload=round(st["ms_upload"], 2), ms_t1=round(st["ms_t1"], 2), ms_dwt=round(st["ms_dwt"], 3), ms_output=round(st["ms_frontend"], 3),
                   num_codeblocks=int(st["num_codeblocks"]))
        print(json.dumps(row), flush=True)
        rows.append(row)
        return out

    whole = leg("full decode", None)
    for side in (512, 1024, 2048, S):
        if side > S:
            continue
        for where, o in (("centre", (S - side) // 2), ("corner", 0)):
            if side == S and where == "corner":
                continue
            got = leg(f"{side}^2 {where if side < S else 'whole image'}", (o, o, side, side))
            assert np.array_equal(got, whole[:, o:o + side, o:o + side]), (side, where)  # (a bench that measured a wrong decode would mislead)
    full = rows[0]["ms_call"]
    print(f"\n{S} x {S} RGB16 9/7 5 levels, {len(cs) / 1e6:.1f} MB, median of {N} calls")
    print("window                 ms/call  of full   t2 host  upload  gather+t1    idwt  output  code-blocks")
    for r in rows:
        print(f"{r['window']:<22} {r['ms_call']:7.2f}  {r['ms_call'] / full:6.2f}x  {r['ms_t2_host']:7.2f} {r['ms_upload']:7.2f}  {r['ms_t1']:9.2f} {r['ms_dwt']:7.3f} {r['ms_output']:7.3f}  {r['num_codeblocks']:11d}")
    enc.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
