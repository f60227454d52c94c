"""GPU: a sequence to a byte budget, the whole call (j2k_hip_encode_sequence_budget_device and its host-frame form; DESIGN.md
section 22).  The yardstick for every byte is the encode under layer_slopes, which is older than this call: len_f(c) is the
length of frame f's file under layers = 1, layer_slopes = { slope_grid(c) }.

Sequences of 4 to 6 frames from synth.planes with different seeds, near-flat frames (distribution "B"; one of them without its
two noise bits) beside noisy ones ("A"; one of them with its noise in the top bits), so that the bytes at a common slope differ
several-fold: 64 x 64 grey 8-bit 5/3 with 3 resolutions; 128 x 128 grey 8-bit 5/3;
200 x 150 rgb10 9/7 + ICT with 5 resolutions; 300 x 200 rgb16 9/7 in tiles of 128; 97 x 61 with rgb_to_sycc 4:2:0.

Per sequence a table of len_f(c) for c within 24 of an interior index c0 (the threshold a ratio-8 encode of the noisiest frame
ends at, on the grid) is built first, and every limit is chosen from it: the sum at c0, that sum less one, a total between two
neighbouring sums, the noisiest frame's length at c0 as a cap with no total, a cap that binds the noisiest frame with a total
that binds the rest (seven eighths of what the cap alone leaves), and no limit at all.  For each: the files are the slopes encodes of the reported indices byte for byte
(J2K_HIP_SLOPE_ALL: the file without rate control), the lengths sum to result.total_bytes within the limits, both boundary
properties hold against the table, frame_index is max(shared_index, cap), a second call and the host-frame call through copy
sinks return the same, the files decode alike with the oracle's decoder and with this library's (sub-sampled files, which the
oracle's decoder does not read: alike with this library's decode of the layer_slopes file), and rate_dev = -1 -- the final layers
cut on the host over the downloaded pass tables -- writes the same files.  A budget below the
coarsest length is refused naming its field with outputs and sinks untouched, after which the handle writes a golden's committed
bytes.  HipCodec::WriteFiles writes the C call's files and throws with every file empty;
a plain sequence call still writes committed bytes; and, on the 200 x 150 sequence at a tenth of the raw size, the budget call's
PSNR spread over the frames is no larger and its lowest PSNR no lower than per-frame layer_rates at the same total.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR, golden_case
from j2k_amd import api, build, synth

pytestmark = pytest.mark.gpu

ALL, K_MAX = api.SLOPE_ALL, api.SLOPE_K_MAX
WINDOW = 24
J2K_HIP_ERR_OVERFLOW = 4

CASES = {
    "grey64": dict(w=64, h=64, nc=1, prec=8, kw=dict(reversible=True, num_resolutions=3), frames=[(1, "Anoise"), (2, "Bflat"), (3, "A"), (4, "B")]),
    "grey128": dict(w=128, h=128, nc=1, prec=8, kw=dict(reversible=True), frames=[(5, "Bflat"), (6, "Anoise"), (7, "B"), (8, "A"), (9, "B")]),
    "rgb10": dict(w=200, h=150, nc=3, prec=10, kw=dict(reversible=False, ycc=True, num_resolutions=5),
                  frames=[(10, "Anoise"), (11, "Bflat"), (12, "B"), (13, "A"), (14, "B"), (15, "A")]),
    "rgb16_tiles": dict(w=300, h=200, nc=3, prec=16, kw=dict(reversible=False, tile_size=128), frames=[(16, "Bflat"), (17, "Anoise"), (18, "B"), (19, "A")]),
    "sycc420": dict(w=97, h=61, nc=3, prec=8, kw=dict(reversible=False, sub=[(1, 1), (2, 2), (2, 2)], rgb_to_sycc=True),
                    frames=[(20, "Anoise"), (21, "Bflat"), (22, "A"), (23, "B")]),
}


@pytest.fixture(scope="module")
def enc():
    e = api.Encoder(0)
    yield e
    api.tune("rate_dev", 0)
    e.close()


def golden_params(g):
    kw = g["params"]
    return api.make_params(g["width"], g["height"], g["ncomp"], g["prec"], reversible=kw.get("reversible", True), ycc=kw.get("mct", False),
                           tile_size=kw.get("tile", 0), num_resolutions=kw.get("numres", 6), cblk=tuple(kw.get("cblk", (64, 64))),
                           comment=g.get("comment", ""))


class Sequence:
    """A case's frames on the device and its table of lengths, made once and never changed."""

    def __init__(self, enc, case):
        self.enc, self.case = enc, case
        c = case
        self.mk = lambda **how: api.make_params(c["w"], c["h"], c["nc"], c["prec"], comment="", **c["kw"], **how)
        self.planes = [synth.planes(c["w"], c["h"], c["nc"], c["prec"], seed, dist[0]) for seed, dist in c["frames"]]
        for k, (_, dist) in enumerate(c["frames"]):
            if dist == "Bflat":  # the near-flat frame: distribution B without its two noise bits, the gradient alone
                self.planes[k] = self.planes[k] & ~3
            if dist == "Anoise":  # the noise frame: distribution A with its noise moved up to the top bits
                self.planes[k] = (self.planes[k] << 4) & ((1 << c["prec"]) - 1)
        packed = [synth.ae_frame(pl, c["prec"]) for pl in self.planes]
        self.frames, self.lay = [f for f, _ in packed], packed[0][1]
        self.dptrs = [enc.upload(f) for f in self.frames]
        self.F = len(self.frames)
        self.files = {}  # (f, index) -> bytes
        self.decoded = {}  # (f, index) -> samples of that file
        plain = [len(x[2]) for x in enc.encode_sequence_device(self.dptrs, self.lay, self.mk())]
        self.noisy = int(np.argmax(plain))
        enc.encode_device(self.dptrs[self.noisy], self.lay, self.mk(rates=[8.0]))
        t = enc.layer_slopes(0)[0]
        assert t > 0, "the ratio-8 encode cuts nothing: no interior threshold"
        self.c0 = int(round(16 * math.log2(t)))
        for c_ in range(self.c0 - WINDOW, self.c0 + WINDOW + 1):
            self.row(c_)

    def close(self):
        for d in self.dptrs:
            self.enc.free(d)

    def row(self, c):
        """All frames at index c in one slopes call (byte-identical to frame-by-frame calls: test_slopes_goldens.py)."""
        if (0, c) not in self.files:
            for f, x in enumerate(self.enc.encode_sequence_device(self.dptrs, self.lay, self.mk(slopes=[api.slope_grid(c)]))):
                self.files[(f, c)] = x[2]
        return [len(self.files[(f, c)]) for f in range(self.F)]

    def length(self, f, c):
        return self.row(c)[f]

    def reference_samples(self, oracle, f, c, data):
        """The samples the layer_slopes file `data` of frame f at index c decodes to, once per (f, c)."""
        if (f, c) not in self.decoded:
            if "sub" in self.case["kw"]:
                self.decoded[(f, c)] = self.enc.decode_planar(data).astype(np.int32)
            else:
                self.decoded[(f, c)] = oracle.decode(data)
        return self.decoded[(f, c)]

    def total(self, c, caps=None):
        return sum(self.length(f, max(c, caps[f]) if caps else c) for f in range(self.F))

    def limits(self):
        c0, n = self.c0, self.noisy
        out = {"sum": (self.total(c0), 0), "sum-1": (self.total(c0) - 1, 0)}
        for c in range(c0, c0 + WINDOW):
            if self.total(c) > self.total(c + 1) + 1:
                out["between"] = ((self.total(c) + self.total(c + 1)) // 2, 0)
                break
        out["cap"] = (0, self.length(n, c0))
        out["both"] = (None, self.length(n, c0 + 2))  # (the total: seven eighths of what this cap alone leaves, test_limits_from_the_table)
        out["none"] = (0, 0)
        return out


_sequences = {}


@pytest.fixture(scope="module")
def sequences(enc):
    def get(name):
        if name not in _sequences:
            _sequences[name] = Sequence(enc, CASES[name])
        return _sequences[name]
    yield get
    for s in _sequences.values():
        s.close()
    _sequences.clear()


def check_outcome(seq, total, frame_max, files, index, res):
    """The contract, against the table (an index outside the window costs the one extra slopes encode it needs)."""
    F = seq.F
    lens = [len(x) for x in files]
    assert lens == [seq.length(f, index[f]) for f in range(F)]
    assert sum(lens) == res["total_bytes"] and (not total or sum(lens) <= total) and (not frame_max or max(lens) <= frame_max), (lens, total, frame_max)
    shared = res["shared_index"]
    assert all(index[f] >= shared for f in range(F)) and ALL <= shared <= K_MAX
    assert res["capped_frames"] == sum(index[f] > shared for f in range(F))
    if not frame_max:
        assert index == [shared] * F
    if not total:
        assert shared == ALL
    caps = []
    for f in range(F):
        if index[f] > shared:  # its cap: a boundary of frame_max
            assert seq.length(f, index[f]) <= frame_max < seq.length(f, index[f] - 1), (f, index[f])
            caps.append(index[f])
        else:  # some cap at or below the shared index; exactly there when the index below does not fit the frame
            below_fits = shared == ALL or not frame_max or seq.length(f, shared - 1) <= frame_max
            caps.append(ALL if below_fits else shared)
    if total and shared != ALL:
        assert seq.total(shared - 1, caps) > total, (shared, caps)
    return caps


@pytest.mark.parametrize("name", list(CASES))
def test_limits_from_the_table(enc, oracle, sequences, name):
    seq = sequences(name)
    plain = [x[2] for x in enc.encode_sequence_device(seq.dptrs, seq.lay, seq.mk())]
    whole = seq.row(ALL)
    at_c0 = seq.row(seq.c0)
    print(name, "c0", seq.c0, "lengths at ALL", whole, "at c0", at_c0)
    assert [len(x) for x in plain] == whole
    assert max(at_c0) >= 3 * min(at_c0), at_c0  # at a common slope the frames' bytes differ several-fold
    limits = seq.limits()
    assert "between" in limits
    for kind, (total, frame_max) in limits.items():
        if kind == "both":
            # a cap that binds the noise frame and a total that binds the rest: the cap alone first (its files are held to the
            # table like every other call's), then a total below what those files take, which the shared index has to meet
            alone = enc.encode_sequence_budget_device(seq.dptrs, seq.lay, seq.mk(), 0, frame_max)
            check_outcome(seq, 0, frame_max, *alone)
            total = 7 * alone[2]["total_bytes"] // 8
        files, index, res = enc.encode_sequence_budget_device(seq.dptrs, seq.lay, seq.mk(), total, frame_max)
        print(name, kind, (total, frame_max), "->", index, res)
        # the files, byte for byte
        for f in range(seq.F):
            want = enc.encode_device(seq.dptrs[f], seq.lay, seq.mk(slopes=[api.slope_grid(index[f])]))[2]
            assert files[f] == want, (kind, f, index[f])
            if index[f] == ALL:
                assert files[f] == plain[f]
            # ... and a file: this library's decoder and the oracle's agree on every sample (the oracle's decoder does not read
            # sub-sampled components: there this library's decode of the layer_slopes file, from an encode of its own, stands in)
            got = enc.decode_planar(files[f]).astype(np.int32)
            ref = seq.reference_samples(oracle, f, index[f], want)
            assert got.shape == ref.shape and np.array_equal(got, ref), (kind, f, index[f])
        assert enc.layer_slopes(0) == [api.slope_grid(index[-1])]
        check_outcome(seq, total, frame_max, files, index, res)
        if kind == "none":
            assert index == [ALL] * seq.F and res["exact_plans"] == 0 and res["curve_launches"] == 0
        if kind == "cap":
            assert index[seq.noisy] > ALL and res["capped_frames"] >= 1
        if kind == "both":
            assert res["shared_index"] > ALL and index[seq.noisy] > res["shared_index"], (index, res)
        if kind in ("sum", "sum-1", "between"):
            assert ALL < res["shared_index"] and abs(res["shared_index"] - seq.c0) <= WINDOW
        # deterministic, and the same from host frames through copy sinks
        again = enc.encode_sequence_budget_device(seq.dptrs, seq.lay, seq.mk(), total, frame_max)
        assert again[0] == files and again[1] == index and again[2] == res
        host = enc.encode_sequence_budget(seq.frames, seq.lay, seq.mk(), total, frame_max)
        assert host[0] == files and host[1] == index and host[2] == res
        # rate_dev = -1: the search as before, the final layers cut by the host over the downloaded pass tables -- the same files
        api.tune("rate_dev", -1)
        try:
            assert enc.encode_sequence_budget_device(seq.dptrs, seq.lay, seq.mk(), total, frame_max)[:2] == (files, index), kind
        finally:
            api.tune("rate_dev", 0)


@pytest.mark.parametrize("name", ["grey64", "rgb10"])
def test_a_budget_that_cannot_be_met(enc, golden, sequences, name):
    seq = sequences(name)
    coarsest = seq.row(K_MAX)
    nf = seq.F
    for total, frame_max, field in ((sum(coarsest) - 1, 0, "total_bytes"), (0, max(coarsest) - 1, "frame_max_bytes")):
        ptrs, lens, index = (C.c_void_p * nf)(*([0xA5A5] * nf)), (C.c_size_t * nf)(*([0xA5A5] * nf)), (C.c_int32 * nf)(*([0xA5A5] * nf))
        with pytest.raises(api.J2kHipError) as x:
            enc.encode_sequence_budget_device(seq.dptrs, seq.lay, seq.mk(), total, frame_max, outputs=(ptrs, lens, index))
        assert x.value.code == J2K_HIP_ERR_OVERFLOW and field in str(x.value), str(x.value)
        assert str(sum(coarsest) if total else max(coarsest)) in str(x.value), str(x.value)
        assert list(ptrs) == [0xA5A5] * nf and list(lens) == [0xA5A5] * nf and list(index) == [0xA5A5] * nf
        with pytest.raises(api.J2kHipError) as x:
            enc.encode_sequence_budget(seq.frames, seq.lay, seq.mk(), total, frame_max, capacity=4096, fill=0xA5)
        assert x.value.code == J2K_HIP_ERR_OVERFLOW and field in str(x.value), str(x.value)
        assert all(pos == 0 and (buf == 0xA5).all() for buf, pos in x.value.sinks) and x.value.index == [0xA5] * nf
        # the handle takes its next call
        g, pl, _, cs = golden_case(golden, "g3_300x200_rgb8_53_rct")
        frame, lay = synth.ae_frame(pl, g["prec"])
        assert enc.encode_host(frame, lay, golden_params(g)) == cs
    # one byte more fits: the coarsest candidate is the answer, or a finer one of the same length
    files, index, res = enc.encode_sequence_budget_device(seq.dptrs, seq.lay, seq.mk(), sum(coarsest), 0)
    assert [len(x) for x in files] == coarsest or sum(len(x) for x in files) <= sum(coarsest)
    check_outcome(seq, sum(coarsest), 0, files, index, res)


def test_refusals_come_before_any_device_work(enc, sequences):
    seq = sequences("grey64")
    for how, word in ((dict(layers=2), "layers"), (dict(rates=[20.0]), "layer_rates"), (dict(slopes=[1.0]), "layer_slopes"), (dict(cblk_style=1), "cblk_style"),
                      (dict(guard_bits=0x100), "guard_bits")):
        before = enc.stats()
        with pytest.raises(api.J2kHipError) as x:
            enc.encode_sequence_budget_device(seq.dptrs, seq.lay, seq.mk(**how), 10000, 0)
        assert x.value.code == 1 and word in str(x.value)
        assert enc.stats() == before
    bad = api.make_budget(10000, 0)
    bad.flags = 1
    with pytest.raises(api.J2kHipError) as x:
        enc.encode_sequence_budget_device(seq.dptrs, seq.lay, seq.mk(), budget=bad)
    assert x.value.code == 1 and "flags" in str(x.value)
    files, index, res = enc.encode_sequence_budget_device(seq.dptrs, seq.lay, seq.mk(guard_bits=3), seq.total(seq.c0), 0)
    assert sum(len(x) for x in files) <= seq.total(seq.c0) and len(set(index)) == 1


def test_a_plain_sequence_call_writes_the_committed_bytes(enc, golden):
    """Nothing moves in the older calls: two golden frames through j2k_hip_encode_sequence_device are the committed files, and
    the statistics that count work are those of the frames."""
    for name in ("g3_300x200_rgb8_53_rct", "g6_300x200_rgb16_97_ict"):
        g, pl, _, cs = golden_case(golden, name)
        frame, lay = synth.ae_frame(pl, g["prec"])
        p = golden_params(g)
        d = enc.upload(frame)
        try:
            assert enc.encode_device(d, lay, p)[2] == cs
            one = enc.stats()
            assert [x[2] for x in enc.encode_sequence_device([d, d], lay, p)] == [cs, cs]
            two = enc.stats()
        finally:
            enc.free(d)
        assert one["codestream_bytes"] == len(cs) and one["num_codeblocks"] == len(api.frame_blocks(p))
        for k in ("num_codeblocks", "num_symbols", "codestream_bytes"):
            assert two[k] == 2 * one[k], k


def _psnr(diffs, prec):
    sq, n = sum(d["sum_sq"] for d in diffs), sum(d["samples"] for d in diffs)
    return math.inf if sq == 0 else 10 * math.log10(((1 << prec) - 1) ** 2 / (sq / n))


def test_quality_is_more_even_than_under_equal_rates(enc, sequences):
    """The point of the call: the 200 x 150 sequence in a tenth of its raw size.  Per-frame layer_rates at the same total split
    evenly presses every frame to one length; the budget call holds one threshold and lets the bytes follow the content, so
    its PSNR spread over the frames is no larger and its worst frame no worse."""
    seq = sequences("rgb10")
    c = seq.case
    raw = c["w"] * c["h"] * c["nc"] * c["prec"] // 8
    total = seq.F * raw // 10
    files, index, res = enc.encode_sequence_budget_device(seq.dptrs, seq.lay, seq.mk(), total, 0)
    assert sum(len(x) for x in files) <= total and len(set(index)) == 1
    rated = [x[2] for x in enc.encode_sequence_device(seq.dptrs, seq.lay, seq.mk(rates=[10.0]))]
    psnr = lambda fs: [_psnr(enc.compare(fs[f], seq.mk(), frame=seq.frames[f], layout=seq.lay), c["prec"]) for f in range(seq.F)]
    a, b = psnr(files), psnr(rated)
    print("budget: bytes", [len(x) for x in files], "psnr", [round(v, 2) for v in a], "| rates: bytes", [len(x) for x in rated], "psnr", [round(v, 2) for v in b])
    assert max(a) - min(a) <= max(b) - min(b)
    assert min(a) >= min(b)


def test_the_codec_writes_the_c_calls_files(enc):
    """HipCodec::WriteFiles through the test hook: the files of j2k_hip_encode_sequence_budget under the same parameters,
    whatever settings.method and settings.layers say; a budget that cannot be met throws and leaves every OutputFile empty."""
    path = os.path.join(os.path.dirname(api.LIBPATH), "libj2k_host.so")
    if not os.path.exists(path):
        build.build_host()
    H = C.CDLL(path)
    H.j2k_host_test_write_files.restype = C.c_long
    H.j2k_host_test_write_files.argtypes = [C.POINTER(C.c_void_p), C.c_uint, C.c_uint, C.c_uint, C.c_long] + [C.c_int] * 6 + [C.c_uint, C.c_ulonglong, C.c_ulonglong,
                                            C.c_void_p, C.c_ulong, C.POINTER(C.c_ulong), C.c_char_p, C.c_ulong]
    w, h, nc, prec = 128, 96, 3, 8
    planes = [synth.planes(w, h, nc, prec, seed, dist) for seed, dist in ((31, "A"), (32, "B"), (33, "A"))]
    packed = [synth.ae_frame(pl, prec) for pl in planes]
    frames, lay = [f for f, _ in packed], packed[0][1]
    p = api.make_params(w, h, nc, prec, reversible=False, ycc=True, num_resolutions=0, cblk=(0, 0), comment=None)
    plain = enc.encode_sequence_budget(frames, lay, p)[0]
    total, frame_max = sum(len(x) for x in plain) // 3, max(len(x) for x in plain) // 2
    want, index, res = enc.encode_sequence_budget(frames, lay, p, total, frame_max)
    assert res["shared_index"] > ALL

    def write_files(total, frame_max):
        n, stride = len(frames), 1 << 20
        out, lens, err = np.zeros(n * stride, np.uint8), (C.c_ulong * n)(), C.create_string_buffer(512)
        ptrs = (C.c_void_p * n)(*[f.ctypes.data for f in frames])
        rc = H.j2k_host_test_write_files(ptrs, n, w, h, lay["rowbytes"], lay["sample_bytes"], nc, prec, 0, 1, 0, 0, total, frame_max, out.ctypes.data, stride,
                                         lens, err, 512)
        return rc, [out[f * stride:f * stride + lens[f]].tobytes() for f in range(n)], err.value.decode()

    rc, got, err = write_files(total, frame_max)
    assert rc == 0, err
    assert got == want
    rc, got, err = write_files(100, 0)
    assert rc == -1 and "Error writing file" in err and "total_bytes" in err, err
    assert got == [b""] * len(frames)
