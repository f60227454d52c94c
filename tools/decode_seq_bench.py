#!/usr/bin/env python3
"""Sequence decode throughput from ONE host thread: N distinct frames per j2k_hip_decode_sequence_device call (their
code-blocks share the gather, Tier-1, inverse DWT and output launches) beside a loop of N single-frame
j2k_hip_decode_device calls on the same handle, device destinations in both.  Prints frames/s, ms per frame, the Tier-1 kernel
taken and GPU_MAX_HW_QUEUES as found (the variable is left alone); every output is checked against the single-frame decode.
usage: tools/decode_seq_bench.py [CASE ...]   (C5, DCI4K, C3)"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from j2k_amd import api, synth  # noqa: E402

CASES = {"C5": (4096, 2160, 3, 10, False), "C3": (8192, 8192, 3, 16, False), "DCI4K": (4096, 2160, 3, 12, False)}  # as tools/decode_inflight.py
FRAMES = {"C5": (1, 2, 4, 8, 16), "DCI4K": (1, 2, 4, 8, 16), "C3": (1, 2, 3)}
REPEATS = {"C5": 3, "DCI4K": 3, "C3": 2}


def kernel_name(enc):
    lane, wave = enc.decode_kernels()
    return "lanes" if lane and not wave else ("waves" if wave and not lane else f"lanes + tail of {wave}")


def main():
    print(f"GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES', '(unset)')}", flush=True)
    enc = api.Encoder(0)
    L = enc.L
    # the frames are encoded here: not band-pipelined, whose streams want more hardware queues than the runtime's default
    # (the variable is the host's; this tool measures what one thread gets with whatever it finds)
    api.tune("bands", -1)
    for name in (sys.argv[1:] or ["C5", "DCI4K", "C3"]):
        w, h, nc, prec, rev = CASES[name]
        nmax = max(FRAMES[name])
        p = api.make_params(w, h, nc, prec, reversible=rev, ycc=True, comment="")
        if name == "DCI4K":
            p = api.make_params(w, h, nc, prec, num_resolutions=7, dci_profile=4, comment="")
        files, refs = [], []
        for f in range(nmax):  # distinct frames
            frame, lay = synth.ae_frame(synth.planes(w, h, nc, prec, 7 + f), prec)
            files.append(enc.encode_host(frame, lay, p))
            refs.append(enc.decode_planar(files[-1]))
            del frame
        api.sequence_check(files)
        item = refs[0].itemsize
        per = nc * h * w * item
        d_out = enc.malloc(nmax * per)
        planes = (api.OutPlane * (nmax * nc))()
        for k in range(nmax * nc):
            api._set_outplane(planes[k], d_out + k * h * w * item, item, w * item, 8 * item, min(prec, 8 * item), w, h)
        bufs = [np.frombuffer(d, dtype=np.uint8) for d in files]
        fa, _keep = api._seq_files(files)

        def outputs_ok(n):
            got = enc.d2h(d_out, n * per).view(refs[0].dtype).reshape((n,) + refs[0].shape)
            return all(np.array_equal(got[f], refs[f]) for f in range(n))

        def clear(n):
            enc.h2d(d_out, np.zeros(n * per, dtype=np.uint8))

        for n in FRAMES[name]:
            def one_call():
                enc._check(L.j2k_hip_decode_sequence_device(enc.h, fa, n, 1, None, planes, nc))

            def loop():
                for f in range(n):
                    enc._check(L.j2k_hip_decode_device(enc.h, bufs[f].ctypes.data, len(files[f]), 1, C.cast(C.byref(planes, f * nc * C.sizeof(api.OutPlane)), C.POINTER(api.OutPlane)), nc))

            for label, fn in (("sequence call", one_call), ("single-frame loop", loop)):
                clear(n)
                fn()  # warm-up: arenas
                kern = kernel_name(enc)
                ok = outputs_ok(n)
                reps = max(1, REPEATS[name] * (4 if n <= 2 else 1))
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                dt = time.perf_counter() - t0
                print(f"{name} frames={n:2d} {label:17s}: {n * reps / dt:7.1f} frames/s = {n * reps * w * h / dt / 1e6:7.0f} Mpixel/s, "
                      f"{dt / (n * reps) * 1e3:6.2f} ms per frame, Tier-1 {kern}{'' if ok else '  ** OUTPUT DIFFERS **'}", flush=True)
        enc.free(d_out)
        del files, refs
    enc.close()


if __name__ == "__main__":
    main()
