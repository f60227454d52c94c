"""The model of a sequence encode to a byte budget (j2k_hip_encode_sequence_budget_device).  Plain
helpers: no fixtures, no tests.

  * the public grid of slope thresholds, from the sixteen constants as the header prints them;
  * the rate curve of a call read as frames -- body bytes and header bits per frame and candidate -- from
    rate_model.makelayer_plain and rate_model.header_bits: what rate_curve_kernel must return, integer for integer;
  * brute force over given length tables: the set of every valid cap of a frame and of every valid shared index.
"""
import math
import struct

import numpy as np

import rate_model as rm

K_MIN, K_MAX, ALL = -2048, 2047, -2049
NCAND = K_MAX - ALL + 1  # 4097: position p of a table stands for the index ALL + p

MANTISSAS = [float.fromhex(h) for h in
             """0x1.0000000000000p+0 0x1.0b5586cf9890fp+0 0x1.172b83c7d517bp+0 0x1.2387a6e756238p+0
                0x1.306fe0a31b715p+0 0x1.3dea64c123422p+0 0x1.4bfdad5362a27p+0 0x1.5ab07dd485429p+0
                0x1.6a09e667f3bcdp+0 0x1.7a11473eb0187p+0 0x1.8ace5422aa0dbp+0 0x1.9c49182a3f090p+0
                0x1.ae89f995ad3adp+0 0x1.c199bdd85529cp+0 0x1.d5818dcfba487p+0 0x1.ea4afa2a490dap+0""".split()]


def grid(k):
    """T(k); -1.0 for ALL."""
    if k == ALL:
        return -1.0
    assert K_MIN <= k <= K_MAX, k
    return math.ldexp(MANTISSAS[k % 16], k // 16)  # (Python's % and // are mod and floor)


def candidates(base, step, K):
    return [min(base + j * step, K_MAX) for j in range(K)]


class Curve:
    """The cuts of a call's blocks on the grid, each worked out once (rate_model.Tables of the call, with the weights the
    blocks really take)."""

    def __init__(self, tb):
        self.tb = tb
        self.memo = {}

    def block(self, b, k):
        """(passes, body bytes, header bits) of block b cut at grid index k, one layer."""
        key = (b, k)
        if key not in self.memo:
            n = rm.makelayer_plain(self.tb.rate[b], self.tb.disto[b], 0, grid(k))
            nbytes = rm.u32(self.tb.rate[b][n - 1]) if n else 0
            self.memo[key] = (n, nbytes, rm.header_bits(n, nbytes))
        return self.memo[key]

    def frame(self, f, nb1, k):
        """(body bytes, header bits) of frame f = blocks [f * nb1, (f + 1) * nb1) at grid index k."""
        body = bits = 0
        for b in range(f * nb1, (f + 1) * nb1):
            _, nbytes, hb = self.block(b, k)
            body += nbytes
            bits += hb
        return body, bits

    def sums(self, nframes, cap, base, step, K):
        """What rate_curve_kernel returns: (nframes, K, 2) uint64."""
        assert self.tb.n % nframes == 0
        nb1 = self.tb.n // nframes
        out = np.zeros((nframes, K, 2), np.uint64)
        for f in range(nframes):
            for j, c in enumerate(candidates(base, step, K)):
                out[f, j] = self.frame(f, nb1, max(c, int(cap[f])))
        return out


# ---- brute force over length tables: table[p] = len(ALL + p), p = 0 .. 4096
def valid_caps(table, frame_max):
    """Every index c with len(c) <= frame_max and (c == ALL or len(c - 1) > frame_max); frame_max 0: {ALL}."""
    if not frame_max:
        return {ALL}
    t = np.asarray(table, dtype=np.int64)
    assert t.size == NCAND
    fits = t <= frame_max
    ok = fits.copy()
    ok[1:] &= ~fits[:-1]
    return {ALL + int(p) for p in np.flatnonzero(ok)}


def shared_sums(tables, caps):
    """B(c) for every c: the frames' lengths at max(c, cap_f), summed."""
    total = np.zeros(NCAND, np.int64)
    for t, cap in zip(tables, caps):
        t = np.asarray(t, dtype=np.int64)
        at = np.maximum(np.arange(NCAND), cap - ALL)
        total += t[at]
    return total


def valid_shared(tables, caps, total_bytes):
    """Every shared index valid under the given caps; total_bytes 0: {ALL}."""
    if not total_bytes:
        return {ALL}
    return valid_caps(shared_sums(tables, caps), total_bytes)


# ---- the case file of tests/native/budget_host.cpp
def write_case(path, call, nframes, pricer, settings):
    """The call's tables read as nframes frames, the pricer (0: the estimate, 1: + a constant per frame, 2: + a wobble keyed
    by frame and index) and the settings [(total_bytes, frame_max_bytes)]."""
    with open(path, "wb") as f:
        n = len(call["npasses"])
        f.write(b"RBG1" + struct.pack("<III", n, nframes, pricer))
        for i in range(n):
            k = int(call["npasses"][i])
            f.write(struct.pack("<dII", float(call["weight"][i]), int(call["numbps"][i]), k))
            f.write(call["pass_rate"][i, :k].astype("<u4").tobytes() + call["pass_dist"][i, :k].astype("<i4").tobytes())
        f.write(struct.pack("<I", len(settings)))
        for total, frame_max in settings:
            f.write(struct.pack("<QQ", total, frame_max))


def read_output(text):
    """The program's lines -> (tables {frame: [4097 lengths]}, curve samples [(f, index, body, bits)], results [dict])."""
    tables, samples, results = {}, [], []
    for line in text.splitlines():
        w = line.split()
        if not w:
            continue
        if w[0] == "L":
            tables[int(w[1])] = [int(v) for v in w[2:]]
        elif w[0] == "C":
            samples.append(tuple(int(v) for v in w[1:5]))
        elif w[0] == "R":
            r = dict(setting=int(w[1]), run=int(w[2]), status=int(w[3]), total_limit=int(w[4]), frame_limit=int(w[5]), shared=int(w[6]),
                     launches=int(w[7]), plans=int(w[8]), smallest=int(w[9]))
            bar = w.index("|")
            rest = [int(v) for v in w[bar + 1:]]
            r["cap"], r["index"] = rest[:len(rest) // 2], rest[len(rest) // 2:]
            results.append(r)
    return tables, samples, results
