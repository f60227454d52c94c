"""Code-blocks, slot capacities and launches for the tests of the Tier-1 encode slots at their capacity edge
(test_t1_capacity.py on the GPU through j2k_hip_stage_t1_slots, test_t1_capacity_refs.py on the CPU), and the block families
that hold the slot rule (cblk_capacities) to the oracle's decision counts.  Plain helpers: no fixtures, no tests.

Every block is coded reversibly and 9/7 (step IRR_STEP) under each of STYLES.  For a (reversible, style) pair -- a `combo` --
the oracle gives every block's decisions and codeword, and from them need_sym = round_up(decisions, 16) and need_out =
round_up(length, 16): what the kernels' checked stores are read to need (the modeller flushes 1 KiB at a time and drains in
16-byte lanes, the coders flush 16-byte units and drain 4-byte words).  A `lane` is a block with a pair of capacities:

  fit        (need, need), (need + 16, need), (need, need + 16), (rule, rule): the rule's value at Mb = the block's own
             bit-planes, the smallest slot a frame could give the block
  short_sym  decisions short by 16 bytes, by 1 KiB (one flush), and for blocks of more than 1 KiB of decisions cut to 16 and
             to 1008 bytes (short before the first flush); the codeword slot at need_out
  short_out  codeword short by 16 bytes, and for those long blocks cut to 16 bytes; the decision slot at need_sym

One kind of shortage per lane.  A launch is a list of lanes: `launches(combo)` gives the all-fitting one, one with decision
shortages, one with codeword shortages and one with both; in the three overflow launches short and fitting lanes alternate,
so every coder workgroup of 64 lanes holds both.  guard_of(launch) sizes the guard stripes so that a kernel with no check at
all would still write inside the arena: guard >= (need - cap) + 1024 for every lane.

The blocks: BASE (the shapes that reach every store path) and EDGE_SEEDS, small blocks of noise (edge_block) found by
search_edge_seeds: walking the seeds 0, 1, .. and keeping a seed whenever it meets, for some combo, a condition no block
before it met there -- decisions mod 1024 at or above 1008 (just below a flush), at or below 16 (just behind one), a
codeword length that is 0, 1 or 15 mod 16.  It took the seeds 0 .. EDGE_TRIED - 1 to meet all of them in all six combos.
EXACT_SEEDS are two more such blocks whose decisions are an exact multiple of 1024 (reversibly the first, under 9/7 the second:
search_exact_seed from seed 1000 on, 811 and 159 seeds): only there does the modeller's last flush end exactly at the end of
a slot of need_sym bytes, so only there does that check's `<=` differ from `<`.
"""
import numpy as np

from t1_families import layout, signs

ALL_FIVE = 1 | 2 | 4 | 16 | 32
STYLES = (0, 1 | 4, ALL_FIVE)
COMBOS = [(rev, style) for rev in (True, False) for style in STYLES]
IRR_STEP = 0.37
KFLUSH = 1024  # the modeller's flush unit

BASE_SEED = 20261021
EDGE_SEEDS = (0, 1, 2, 3, 4, 12, 13, 20, 36, 39, 63)  # search_edge_seeds(oracle)
EDGE_TRIED = 64
EXACT_SEEDS = (1810, 1158)  # search_exact_seed(oracle, True), search_exact_seed(oracle, False)


def round_up(v, m):
    return (v + m - 1) // m * m


def edge_block(seed):
    """Noise of 6 .. 10 bits in a block of 8 .. 24 columns and rows, all drawn from the seed: a few thousand decisions."""
    rng = np.random.default_rng(seed)
    w, h, bits = (int(v) for v in rng.integers((8, 8, 6), (25, 25, 11)))
    return rng.integers(-(1 << bits) + 1, 1 << bits, size=(h, w)).astype(np.int64)


def base_blocks():
    """(name, (h, w) int64 samples).  64 x 64 noise: many decision flushes, hundreds of codeword units; sparse: the sample-wise
    halves of the modeller; one sample set: fills, a codeword under 16 bytes, decisions just behind the first flush;
    32 x 32: the transposed bit-plane path; 16 x 16 and 37 x 13: rows read in place; 4 x 4, 1 x 64, 64 x 1: degenerate."""
    rng = np.random.default_rng(BASE_SEED)
    one = np.zeros((64, 64), dtype=np.int64)
    one[37, 21] = 1
    out = [
        ("noise64", rng.integers(-(1 << 16) + 1, 1 << 16, size=(64, 64))),
        ("sparse64", np.where(rng.random((64, 64)) < 0.02, rng.integers(1, 1 << 10, size=(64, 64)), 0) * signs(rng, (64, 64))),
        ("one64", one),
        ("noise32", rng.integers(-(1 << 12) + 1, 1 << 12, size=(32, 32))),
        ("noise16", rng.integers(-(1 << 10) + 1, 1 << 10, size=(16, 16))),
        ("lap37x13", np.rint(rng.laplace(0, 1 << 7, size=(13, 37)))),
        ("noise4x4", rng.integers(-(1 << 16) + 1, 1 << 16, size=(4, 4))),
        ("noise1x64", rng.integers(-(1 << 12) + 1, 1 << 12, size=(64, 1))),
        ("noise64x1", rng.integers(-(1 << 12) + 1, 1 << 12, size=(1, 64))),
    ]
    return [(n, np.asarray(b, dtype=np.int64)) for n, b in out]


def blocks():
    """[(name, samples, orientation)]: BASE, then the searched blocks."""
    bs = base_blocks() + [(f"edge{s}", edge_block(s)) for s in EDGE_SEEDS] + [(f"exact{s}", edge_block(s)) for s in EXACT_SEEDS]
    return [(n, b, i % 4) for i, (n, b) in enumerate(bs)]


def as_plane_values(b, rev):
    """What goes into the encoder's coefficient plane for the samples b: themselves, or 0.61 b as float32 under 9/7."""
    return b.astype(np.int32) if rev else (b * 0.61).astype(np.float32)


def scaled(oracle, b, rev):
    """The block as the Tier-1 coder sees it: int32 with 6 fractional bits (9/7: the oracle's own quantiser, value by value)."""
    v = as_plane_values(b, rev)
    if rev:
        return (v.astype(np.int64) << 6).astype(np.int32)
    quant = oracle.L.j2ko_quant97
    return np.array([[quant(float(x), IRR_STEP) if x else 0 for x in row] for row in v], dtype=np.int32).reshape(v.shape)


def code(oracle, b, orient, rev, style):
    """The oracle's result of one block, with its decisions (symbols: a byte each, context << 1 | bit, as the modeller stores
    them), nsym, need_sym and need_out."""
    r = oracle.t1_block(scaled(oracle, b, rev), orient, style=style, want_symbols=True)
    r["nsym"] = int(len(r["symbols"]))
    r["len"] = len(r["data"])
    r["need_sym"], r["need_out"] = round_up(r["nsym"], 16), round_up(r["len"], 16)
    return r


_refs = {}


def refs(oracle, combo):
    """The oracle's results of blocks() under the combo, computed once per session and left unchanged."""
    if combo not in _refs:
        rev, style = combo
        out = []
        for name, b, o in blocks():
            r = code(oracle, b, o, rev, style)
            r["name"], r["area"] = name, b.size
            out.append(r)
        _refs[combo] = out
    return _refs[combo]


# ---- the edge conditions and the search that meets them
EDGE_CONDITIONS = ("sym_below", "sym_above", "len0", "len1", "len15")


def edge_conditions_of(r):
    m, l = r["nsym"] % KFLUSH, r["len"] % 16
    met = set()
    if r["nsym"] > KFLUSH and m >= KFLUSH - 16:
        met.add("sym_below")
    if r["nsym"] > KFLUSH and m <= 16:
        met.add("sym_above")
    if r["len"]:
        met |= {f"len{k}" for k in (0, 1, 15) if l == k}
    return met


def search_edge_seeds(oracle, limit=4096):
    """(seeds kept, seeds tried): see the module docstring.  The base blocks count first."""
    missing = {(c, k) for c in COMBOS for k in EDGE_CONDITIONS}
    for c in COMBOS:
        for i, (_, b) in enumerate(base_blocks()):
            missing -= {(c, k) for k in edge_conditions_of(code(oracle, b, i % 4, *c))}
    kept = []
    nbase = len(base_blocks())
    for seed in range(limit):
        if not missing:
            return kept, seed
        b = edge_block(seed)
        o = (nbase + len(kept)) % 4  # the orientation of the place it would take
        got = {(c, k) for c in COMBOS for k in edge_conditions_of(code(oracle, b, o, *c))}
        if got & missing:
            missing -= got
            kept.append(seed)
    return kept, (None if missing else limit)


def search_exact_seed(oracle, rev, start=1000, limit=20000):
    """The first seed from `start` on whose edge_block has more than 1024 decisions and an exact multiple of it (the count
    depends on neither style nor orientation)."""
    for seed in range(start, limit):
        n = code(oracle, edge_block(seed), 0, rev, 0)["nsym"]
        if n > KFLUSH and n % KFLUSH == 0:
            return seed
    return None


# ---- lanes and launches
def rule_caps(api, r, style):
    """The slot a frame gives the block in a band of exactly the block's bit-planes (the smallest Mb that can hold it)."""
    return api.cblk_capacities(r["area"], max(r["numbps"], 1), style)


def lanes_of(api, rs, style):
    """Every (block, sym_cap, out_cap, kind) of the combo's blocks."""
    out = []
    for i, r in enumerate(rs):
        ns, no = r["need_sym"], r["need_out"]
        assert ns >= 16 and no >= 16, r["name"]  # (no empty block among the cases)
        rule_s, rule_o = rule_caps(api, r, style)
        long = r["nsym"] > KFLUSH
        for sc, oc in ((ns, no), (ns + 16, no), (ns, no + 16), (rule_s, rule_o)):
            out.append(dict(block=i, sym_cap=sc, out_cap=oc, kind="fit"))
        short_s = [ns - KFLUSH, ns - 16] + ([16, KFLUSH - 16] if long else [])
        for sc in sorted({c for c in short_s if 16 <= c < ns}):
            out.append(dict(block=i, sym_cap=sc, out_cap=no, kind="short_sym"))
        short_o = [no - 16] + ([16] if long else [])
        for oc in sorted({c for c in short_o if 16 <= c < no}):
            out.append(dict(block=i, sym_cap=ns, out_cap=oc, kind="short_out"))
    return out


def _mix(shorts, fits):
    """Short and fitting lanes in turn: every run of 64 holds 32 of each (the last, shorter run at least one pair)."""
    out = []
    for k, s in enumerate(shorts):
        out += [s, fits[k % len(fits)]]
    return out


LAUNCH_KINDS = ("fit", "short_sym", "short_out", "mixed")


def launches(api, rs, style):
    """{kind: lanes}: the all-fitting launch first, then the three overflow launches."""
    lanes = lanes_of(api, rs, style)
    fits = [l for l in lanes if l["kind"] == "fit"]
    ss = [l for l in lanes if l["kind"] == "short_sym"]
    so = [l for l in lanes if l["kind"] == "short_out"]
    both = [x for pair in zip(ss, so * (len(ss) // len(so) + 1)) for x in pair]
    return {"fit": fits, "short_sym": _mix(ss, fits), "short_out": _mix(so, fits), "mixed": _mix(both, fits)}


def shortage(rs, lane):
    r = rs[lane["block"]]
    return max(r["need_sym"] - lane["sym_cap"], 0), max(r["need_out"] - lane["out_cap"], 0)


def guard_of(rs, lanes):
    """The guard stripe of a launch: the largest shortage of a lane plus 1 KiB, in 16-byte units."""
    return round_up(max(max(shortage(rs, l)) for l in lanes) + KFLUSH, 16)


def launch_plane(lanes, rev):
    """(plane, rectangles, orientations, step sizes) of a launch: a 64 x 64 cell per lane (the modeller rewrites its block)."""
    bl = blocks()
    coef, rects, orients = layout([(bl[l["block"]][1], bl[l["block"]][2]) for l in lanes])
    return as_plane_values(coef, rev), rects, orients, [1.0 if rev else IRR_STEP] * len(lanes)


# ---- the slot rule against the oracle: block families of p bit-planes
RULE_SHAPES = [(64, 64), (32, 32), (4, 4), (1, 64), (64, 63)]  # (w, h); 64 x 63: full stripes and a partial one, no 1 KiB of rounding to spare
RULE_MBS = range(1, 13)


def old_capacities(area, Mb, style):
    """A literal copy of the rule as it stood before the fix (encoder.cpp, cblk_capacities)."""
    symcap = round_up(area * 3 * Mb // 2 + area + 64, 1024)
    style_room = 8 * (3 * Mb) if style else 0
    return symcap, round_up(symcap // 4 + 64 + style_room, 16)


def decisions_bound(w, h, p):
    """The most decisions a w x h block of p bit-planes can have: one zero-coding or refinement decision
    per sample and plane, one sign per sample, and two more for every stripe column whose run-length mode breaks -- at most
    every other column of a full stripe, once."""
    return (p + 1) * w * h + 2 * ((w + 1) // 2) * (h // 4)


def rule_families(w, h, p, seed):
    """[(name, magnitudes)] of p bit-planes (non-negative; the caller signs them)."""
    rng = np.random.default_rng(seed)
    top = (1 << p) - 1
    out = [("noise", rng.integers(0, top + 1, size=(h, w))), ("all_top", np.full((h, w), top))]
    for r in range(4):
        b = np.zeros((h, w), dtype=np.int64)
        b[r::4, :] = top
        out.append((f"row{r}", b))
    # rows lit one plane after another: row y turns significant in plane y mod p, counted from the top
    out.append(("rows_by_plane", np.repeat((top >> (np.arange(h) % p))[:, None], w, axis=1)))
    yy, xx = np.mgrid[0:h, 0:w]
    out.append(("checker", np.where((yy + xx) & 1, top, 0)))
    out.append(("checker_low", np.where((yy + xx) & 1, top, top >> 1)))
    for q, name in ((0.5, "bernoulli_half"), (0.25, "bernoulli_quarter")):
        b = np.where(rng.random((h, w)) < q, rng.integers(1 << (p - 1), top + 1, size=(h, w)), rng.integers(0, top + 1, size=(h, w)) >> 1)
        b.flat[-1] = top  # (the mask holds its p planes)
        out.append((name, b))
    # the worst case of the argument: in the top plane row 0 of every other column of every full stripe (each breaks a run
    # at its first sample, and keeps the columns beside it out of run-length mode); every other sample follows a plane later
    b = np.full((h, w), top >> 1, dtype=np.int64)
    for s in range(0, h - 3, 4):
        b[s, 0::2] = top
    out.append(("run_breaks", b))
    out[0][1].flat[0] = top  # (the noise holds its p planes)
    return [(n, np.asarray(b, dtype=np.int64)) for n, b in out]


# ---- 1- and 2-bit frames at one guard bit: does a frame's block outgrow the slot the old rule gave it?
SEARCH_FRAMES = 2000


def search_small_frames(oracle, nframes=SEARCH_FRAMES):
    """(frames tried, blocks seen, [(frame, block row, decisions, old slot)] that exceed the old slot, the largest
    decisions / old slot seen).  Frames of 1 and 2 bits, one or three components, 64 x 64, two or three resolutions, random
    masks of four densities, checkers and stripes; the bands' Mb at guard_bits = 1 (one below the oracle's, which counts two
    guard bits)."""
    import guard_cases as gc
    found, worst, seen = [], 0.0, 0
    for k in range(nframes):
        rng = np.random.default_rng(1000 + k)
        prec, nc, numres = 1 + k % 2, (1, 3)[(k // 2) % 2], 2 + (k // 4) % 2
        kind = (k // 8) % 6
        top = (1 << prec) - 1
        if kind < 4:
            pl = np.where(rng.random((nc, 64, 64)) < (0.5, 0.25, 0.1, 0.9)[kind], top, 0)
        elif kind == 4:
            yy, xx = np.mgrid[0:64, 0:64]
            pl = np.stack([np.where(((yy >> (k % 3)) + (xx >> (k % 2)) + c) & 1, top, 0) for c in range(nc)])
        else:
            pl = np.stack([np.where((np.arange(64)[:, None] + c + rng.integers(0, 2, size=(1, 64))) % (2 + k % 3) == 0, top, 0) for c in range(nc)])
        rows = gc.classify_planes(oracle, pl.astype(np.int32), prec, True, numres, 0, want_symbols=True)
        for b in rows:
            Mb = b["Mb"] - 1
            if Mb < 1:
                continue
            seen += 1
            n, cap = len(b["t1"]["symbols"]), old_capacities(b["w"] * b["h"], Mb, 0)[0]
            worst = max(worst, n / cap)
            if n > cap:
                found.append((k, (b["comp"], b["res"], b["orient"]), n, cap))
    return nframes, seen, found, worst
