"""CPU: the reference model of the rate control's per-block arithmetic (tests/rate_model.py) against the code itself --
j2k_amd/csrc/rate_block.h compiled into a stand-alone host program (tests/native/rate_block_host.cpp) with the address and
undefined-behaviour sanitizers linked in, run as a child process with the test's own environment.  Every number must agree
bit for bit on every family of tests/rate_cases.py: cumulative distortions, slope ranges, reach, steepest, the scan's pass
counts, decisions, bytes and sums, the ahead walk, the header-bit formula.  This is also where the inputs are proven fit
before test_rate_stage.py hands them to the GPU: the properties asserted there on the device's numbers are asserted here on
the host's, against the plain makelayer of rate_model.py:

  * the shortcut never changes a pass count;
  * reach is a bound: when the plain scan adds bytes at threshold t, t does not exceed reach[last pass taken];
  * the ahead walk is a bound on the plain scan's body bytes, per component;
  * the sums are the sums of the per-block results.

The two bound properties are claimed for monotone tables (rate_control.cpp), and asserted on those.
"""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import rate_cases as rc
import rate_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "rate_block_host.cpp")
HAND_HEADERS = [(1, 1, 5), (2, 100, 13), (3, 5, 9), (6, 4096, 31), (37, 70000, 43)]  # (passes, bytes, bits), worked out below


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("rate_block_host") / "rate_block_host")
    subprocess.check_call([gxx, "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-Wall", "-I", os.path.join(ROOT, "j2k_amd", "csrc"), "-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def all_calls(oracle):
    return rc.calls(oracle)


def write_case(path, call, first, count, done, ahead, thresholds, headers=()):
    with open(path, "wb") as f:
        n = len(call["npasses"])
        f.write(b"RBH1" + struct.pack("<I", n))
        for i in range(n):
            k = int(call["npasses"][i])
            f.write(struct.pack("<dIII", float(call["weight"][i]), int(call["comp"][i]), int(call["numbps"][i]), k))
            f.write(call["pass_rate"][i, :k].astype("<u4").tobytes() + call["pass_dist"][i, :k].astype("<i4").tobytes())
        f.write(struct.pack("<III", first, count, 0 if done is None else 1))
        if done is not None:
            f.write(bytes(bytearray(int(v) for v in done)))
        f.write(struct.pack(f"<I{len(ahead)}d", len(ahead), *ahead))
        f.write(struct.pack(f"<I{len(thresholds)}d", len(thresholds), *thresholds))
        f.write(struct.pack("<I", len(headers)) + b"".join(struct.pack("<II", a, b) for a, b in headers))


def run_host(program, path):
    r = subprocess.run([program, path], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    out = dict(D={}, R={}, B={}, A={}, S={}, T={}, H=[])
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] in "DRB":
            out[w[0]][int(w[1])] = [int(v, 16) for v in w[2:]]
        elif w[0] in "AS":
            out[w[0]][int(w[1])] = [int(v, 16) for v in w[2:]]
        elif w[0] == "T":
            out["T"][(int(w[1]), int(w[2]))] = (int(w[3]), int(w[4], 16), int(w[5], 16), int(w[6]), int(w[7]))
        else:
            out["H"].append((int(w[1]), int(w[2]), int(w[3])))
    return out


def check_prepare(tb, got, n):
    for b in range(n):
        assert got["D"][b] == [rm.bits64(v) for v in tb.disto[b]], b
        assert got["R"][b] == [rm.bits32(v) for v in tb.reach[b]], b
        assert got["B"][b] == [rm.bits64(tb.bmin[b]), rm.bits64(tb.bmax[b]), rm.bits64(tb.steepest[b])], b


check_properties, variants, variant_thresholds = rc.check_properties, rc.variants, rc.variant_thresholds


@pytest.mark.parametrize("name", rc.CALL_NAMES)
def test_model_equals_host_and_properties_hold(program, all_calls, tmp_path, name):
    call = all_calls[name]
    n = len(call["npasses"])
    tb = rc.tables(call)
    if call["monotone"]:
        assert all(tb.monotone(b) for b in range(n))
    else:
        assert any(not tb.monotone(b) for b in range(n)) and all(tb.steepest[b] == rm.INF for b in range(n) if not tb.monotone(b))
    for v, (first, count, done, ahead_name) in enumerate(variants(call, tb)):
        ahead = rc.ahead_lists(tb, first, count)[ahead_name]
        assert ahead_name != "explicit128" or len(ahead) == 128
        thresholds = variant_thresholds(tb, first, count)
        path = str(tmp_path / f"{name}_{v}.case")
        write_case(path, call, first, count, done, ahead, thresholds)
        got = run_host(program, path)
        if v == 0:
            check_prepare(tb, got, n)
        assert [got["A"][c] for c in range(4)] == rm.ahead_range(tb, first, count, done, ahead), (name, v)
        scans = []
        for k, t in enumerate(thresholds):
            rows, sums = rm.scan_range(tb, first, count, done, t)
            host_rows = [got["T"][(k, i)] for i in range(count)]
            assert [r[:4] for r in host_rows] == rows, (name, v, t)
            assert [r[4] for r in host_rows] == [r[0] for r in rows], (name, v, t)  # the code's own scan without the shortcut
            assert got["S"][k] == sums, (name, v, t)
            scans.append((host_rows, got["S"][k]))
        check_properties(tb, call, first, count, done, thresholds, scans, ahead, [got["A"][c] for c in range(4)])


def test_the_shortcut_and_the_full_loop_are_both_taken(all_calls):
    """The thresholds reach both branches: above every steepest all monotone blocks take the shortcut, a spoiled block never."""
    for name in ("mono_255", "spoiled_65"):
        call = all_calls[name]
        tb = rc.tables(call)
        t = rc.thresholds(tb, 0, tb.n)[-1]
        short = [tb.steepest[b] + 1e-12 < t * 0.999999 for b in range(tb.n)]
        assert all(short[b] == tb.monotone(b) for b in range(tb.n))
    assert any(s for s in short) and not all(short)


def test_header_bits_by_hand(program, tmp_path):
    """T.800 B.10.6 / B.10.7 with Lblock = 3: bits = number-of-passes code + k increments and their closing zero + the length in
    3 + k + floor(log2 n) bits, k the least that holds the length.
      n = 1, 1 byte:       1 + (0 + 1) + 3            = 5
      n = 2, 100 bytes:    2 + (3 + 1) + (3 + 3 + 1)  = 13   (7 bits of length, 4 to start with)
      n = 3, 5 bytes:      4 + (0 + 1) + (3 + 0 + 1)  = 9
      n = 6, 4096 bytes:   9 + (8 + 1) + (3 + 8 + 2)  = 31   (13 bits of length, 5 to start with)
      n = 37, 70000 bytes: 16 + (9 + 1) + (3 + 9 + 5) = 43   (17 bits of length, 8 to start with)"""
    for n, nbytes, bits in HAND_HEADERS:
        assert rm.header_bits(n, nbytes) == bits
    assert rm.header_bits(0, 0) == 0
    call = rc.synthetic_call("one", 1, 3)
    path = str(tmp_path / "headers.case")
    write_case(path, call, 0, 1, None, [], [], [(a, b) for a, b, _ in HAND_HEADERS] + [(0, 0)])
    assert run_host(program, path)["H"] == HAND_HEADERS + [(0, 0, 0)]


def test_reach_of_a_three_pass_block_by_hand(program, tmp_path):
    """weight 64, two bit-planes, nmsedec 32 / 16 / 64: pass 0 lies in plane 1 (w = 128, 128 * 128 * 32 / 8192 = 64), passes 1
    and 2 in plane 0 (w = 64: 8 and 32); cumulative 64, 72, 104.  Rates 4, 4, 12: pass 1 has no bytes.  Pieces: pass 0 with
    the byte-less pass behind it, (64 + 8) / 4 = 18; pass 2 with the byte-less pass before it, (8 + 32) / 8 = 5.  The slack
    (1e-13 * 104, as slope under 3e-12) vanishes in single precision; times 1.0011: 18.0198 and 5.0055.  The byte-less pass
    takes the larger of its neighbours' bounds.  Single-pass slopes: 64 / 4 = 16 and 32 / 8 = 4."""
    call = rc._pack("hand", [(64.0, 0, 2, [4, 4, 12], [32, 16, 64])], True)
    tb = rc.tables(call)
    assert tb.disto[0] == [64.0, 72.0, 104.0]
    assert (tb.bmin[0], tb.bmax[0]) == (4.0, 16.0)
    assert [rm.bits32(v) for v in tb.reach[0]] == [rm.bits32(np.float32(18.0198)), rm.bits32(np.float32(18.0198)), rm.bits32(np.float32(5.0055))]
    assert tb.steepest[0] == float(np.float32(18.0198))
    path = str(tmp_path / "hand.case")
    write_case(path, call, 0, 1, None, [17.0, 6.0, 5.0], [18.1, 17.0, 16.0, 4.5, 4.0])
    got = run_host(program, path)
    check_prepare(tb, got, 1)
    assert [got["A"][0][k] for k in range(3)] == [4, 4, 12]  # pass 1 comes with pass 0; pass 2 once the threshold is within 5.0055
    assert [got["T"][(k, 0)][0] for k in range(5)] == [0, 2, 2, 2, 3]  # (at 17 the byte-less pass makes the run of passes 0 and 1 steep enough: 72 / 4)


def test_thresholds_below_the_absolute_term(program, tmp_path):
    """rate_block_choose takes a pass when thresh - slope < DBL_EPSILON: an absolute term, so below 2.2e-16 a threshold takes
    passes whose slope it exceeds.  Two blocks show it at t = 1e-16: one pass of slope about 1e-17, and a block whose second
    pass has bytes and no distortion (slope 0, 100000 bytes, behind a pass of distortion 32: its piece's bound is the slack alone, 1e-13 of
    the block's distortion over its bytes, 3.2e-17).  Real frames do not have slopes of 1e-17 -- block_weight is at least about 0.5,
    a non-zero single-pass slope at least weight^2 / 8192 / (bytes of a block) > 1e-10 -- but a pass with bytes and no
    distortion is ordinary (a significance pass that finds nothing), it makes the bisection's lower end 0, and 128 halvings
    of a bracket whose candidates all fit bring the threshold under 2.2e-16 after some 70 rounds.  So reach carries the
    absolute term too (rate_block.h: twice DBL_EPSILON on every piece's bound), and is a bound at these thresholds as well."""
    w = (8192e-17) ** 0.5
    call = rc._pack("tiny", [(w, 0, 1, [1], [1]), (256.0, 1, 2, [1000, 101000], [1, 0])], True)
    tb = rc.tables(call)
    t = 1e-16
    assert 0.9e-17 < tb.disto[0][0] < 1.1e-17 and tb.disto[1][1] == tb.disto[1][0]
    path = str(tmp_path / "tiny.case")
    write_case(path, call, 0, 2, None, [t], [t])
    got = run_host(program, path)
    check_prepare(tb, got, 2)
    assert [rm.makelayer_plain(tb.rate[b], tb.disto[b], 0, t) for b in range(2)] == [1, 2]
    assert [got["T"][(0, b)][0] for b in range(2)] == [1, 2]
    for b in range(2):
        assert all(float(v) >= t for v in tb.reach[b]), (b, tb.reach[b])
    assert (got["A"][0][0], got["A"][1][0]) == (1, 101000)
