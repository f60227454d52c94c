#!/usr/bin/env python3
"""What a draft read of the first L quality layers saves: one 4096 x 2160 RGB 10-bit 9/7 frame, encoded in this process with six
layers (compression ratios RATES, OpenJPEG's cp_disto_alloc semantics), decoded through j2k_hip_decode into planar host
channels kept from call to call with the handle's layer limit at 0 (all layers) and at 1 .. 6, in one process.  The legs are
run twice, interleaved (0, 1 .. 6, 0, 1 .. 6): a drift of the box shows as a difference between the two repeats of a leg.

Per leg and repeat: the median call time of N calls, the stage times of the median call's j2k_hip_stats (ms_t1 = gather +
Tier-1), the code-blocks decoded, the coding passes and codeword bytes handed to Tier-1 (j2k_hip_debug_decode_work), which
Tier-1 kernel ran, and the PSNR of the decoded frame against the source.  The yardstick is L = 0 of the same process.  L = 6 must give the bytes of L = 0.

usage: decode_layers_bench.py [repeats-per-leg]      one JSON line per row, then a table"""
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "24")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from j2k_amd import api, synth  # noqa: E402

W, H, PREC = 4096, 2160, 10
RATES = [160.0, 80.0, 40.0, 20.0, 10.0, 5.0]


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    enc = api.Encoder(0)
    planes = synth.planes(W, H, 3, PREC, 45678)
    frame, lay = synth.ae_frame(planes, PREC)
    p = api.make_params(W, H, 3, PREC, reversible=False, ycc=True, num_resolutions=6, comment="", rates=RATES)
    cs = enc.encode_host(frame, lay, p)
    del frame
    assert api.read_info(cs)["layers"] == len(RATES)
    rows, outs = [], {}

    def leg(L, rep):
        enc.set_max_layers(L)
        out, runs = outs.get(L), []
        for it in range(N + 1):  # (the first call allocates the destination and grows the handle's buffers: not timed)
            t0 = time.perf_counter()
            out = enc.decode_planar(cs, out=out)
            ms = (time.perf_counter() - t0) * 1e3
            if it:
                runs.append((ms, enc.stats()))
        outs[L] = out
        passes, cw_bytes = enc.decode_work()
        lane_blocks, wave_blocks = enc.decode_kernels()
        runs.sort(key=lambda r: r[0])
        ms, st = runs[len(runs) // 2]
        d = out.astype(np.float64) - planes
        mse = float(np.mean(d * d))
        row = dict(layers=L, repeat=rep, ms_call=round(ms, 2), ms_min=round(runs[0][0], 2), ms_t2_host=round(st["ms_t2_host"], 2),
                   ms_upload=round(st["ms_upload"], 2), ms_t1=round(st["ms_t1"], 2), ms_dwt=round(st["ms_dwt"], 3), ms_output=round(st["ms_frontend"], 3),
                   num_codeblocks=int(st["num_codeblocks"]), passes=passes, codeword_bytes=cw_bytes, lane_blocks=lane_blocks, wave_blocks=wave_blocks,
                   psnr_db=round(10.0 * np.log10(((1 << PREC) - 1) ** 2 / mse), 2) if mse else None)
        print(json.dumps(row), flush=True)
        rows.append(row)

    for rep in (1, 2):
        for L in range(0, len(RATES) + 1):
            leg(L, rep)
    enc.set_max_layers(0)
    assert outs[len(RATES)].tobytes() == outs[0].tobytes()  # (a bench that measured a wrong decode would mislead)
    assert all(not np.array_equal(outs[L], outs[L + 1]) for L in range(1, len(RATES)))
    full = {rep: next(r for r in rows if r["layers"] == 0 and r["repeat"] == rep) for rep in (1, 2)}
    print(f"\n{W} x {H} RGB{PREC} 9/7 5 levels, {len(RATES)} layers at ratios {RATES}, {len(cs) / 1e6:.2f} MB, median of {N} calls per leg")
    print("layers rep  ms/call  of L=0   t2 host  upload  gather+t1  of L=0    idwt  output  code-blocks      passes  codeword MB  kernel   PSNR dB")
    for r in rows:
        f = full[r["repeat"]]
        kern = "lanes" if r["lane_blocks"] and not r["wave_blocks"] else "waves" if not r["lane_blocks"] else "lanes+tail"
        print(f"{r['layers']:6d} {r['repeat']:3d}  {r['ms_call']:7.2f}  {r['ms_call'] / f['ms_call']:5.2f}x  {r['ms_t2_host']:7.2f} {r['ms_upload']:7.2f}  {r['ms_t1']:9.2f}  "
              f"{r['ms_t1'] / f['ms_t1']:5.2f}x {r['ms_dwt']:7.3f} {r['ms_output']:7.3f}  {r['num_codeblocks']:11d} {r['passes']:11d}  {r['codeword_bytes'] / 1e6:11.2f}  "
              f"{kern:<10} {r['psnr_db']}")
    enc.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
