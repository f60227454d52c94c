"""CPU: host Tier-2's plan (j2k_hip_debug_tier2_plan -> api.host_tier2_plan, api.assemble) held byte for byte and bit-field for
bit-field to two references that share no code with j2k_amd/csrc/tier2.cpp.

A. Every libopenjp2 file under tests/golden that the oracle's reader takes is planned again from its own block table (the
   reader's parse, in frame_blocks order) and must come out as the file, main header included.  70 candidates as committed
   (files whose COD has SOP / EPH or the vertically causal bit are none: the encoder writes neither -- that rule keeps out
   ext/s4, whose style 63 holds the bit); all 70 come out as the file, none is left out.
B. Synthetic block tables the images never produce (tier2_cases.CASES) are planned, assembled and parsed by the oracle's reader
   (oracle/j2k_oracle_dec.c, written from T.800 B.10): every block's numbps, its pieces per layer (bytes and passes) and its bytes
   must come back, and no other block.  A census over the input tables and the geometry asserts the corpus reaches the classes
   it was made for.

No device runs here.  Figures of the corpus as committed (test_census prints them before it asserts): 56 cases, 13249 blocks,
2050 packets; the most passes one packet gives a block is 70 -- the largest band the parameters allow is the 16-bit reversible
HH band at seven guard bits, Mb = 24, 3 Mb - 2 = 70 (Table B.4's last code reaches 164; a band of 32 bit-planes, 94 passes, is
refused by the parameters: 30 bit-planes at most).  181 packet headers hold a 0xFF before their last two bytes.  3 have
their last bit in the last bit of a 0xFF byte and carry the byte B.10.1 wants behind it, counted by the reader's own bit position: the three headers of the two
cases made for it (tier2_cases: ffend); the random tables reach none.  BitWriter::flush without that byte fails those cases."""
import numpy as np
import pytest

import tier2_cases as tc
from j2k_amd import api

J2K_HIP_ERR_OVERFLOW = 4

# Candidates of part A that are not planned again, each with the reason the encoder's parameters cannot express the file.
# At most 8 may stand here.
LEFT_OUT = {}


# ----------------------------------------------------------------------------------------------------- the reader first
def test_reader_pieces_are_the_blocks_totals():
    """Oracle.file_blocks(layers=True) is the reader's own parse written down: for every fixture the reader takes, a block's
    pieces sum to its passes and bytes (so they concatenate to its bytes), its layers never go back, the plain call finds the
    same blocks, and under bypass / termall the pieces cut the codeword segments and nothing else."""
    read = 0
    for rel in tc.fixture_files():
        cs, parsed = tc.read_fixture(rel)
        if parsed is None:
            continue
        read += 1
        f = tc.header_fields(cs)
        plain = tc.oracle().file_blocks(cs)
        assert len(plain["blocks"]) == len(parsed["blocks"]), rel
        for b, b0 in zip(parsed["blocks"], plain["blocks"]):
            assert {k: v for k, v in b.items() if k != "pieces"} == b0, rel
            pc = b["pieces"]
            assert sum(p[1] for p in pc) == len(b["data"]) and sum(p[2] for p in pc) == b["npasses"], rel
            assert all(p[2] >= 1 and p[0] < f["layers"] for p in pc) and [p[0] for p in pc] == sorted(p[0] for p in pc), rel
            if f["style"] & 5:
                ends = set(zip(np.cumsum([p[1] for p in pc]).tolist(), np.cumsum([p[2] for p in pc]).tolist()))
                seg_ends = list(zip(np.cumsum([s[0] for s in b["segs"]]).tolist(), np.cumsum([s[1] for s in b["segs"]]).tolist()))
                assert set(seg_ends) <= ends and seg_ends[-1] == (len(b["data"]), b["npasses"]), rel
                done = 0
                for lay in sorted({p[0] for p in pc}):  # a layer's pieces are its passes cut where B.10.7.2 cuts them
                    runs = [p[2] for p in pc if p[0] == lay]
                    assert runs == tc.layer_segments(f["style"], done, sum(runs)), rel
                    done += sum(runs)
            else:
                assert len({p[0] for p in pc}) == len(pc), rel  # one length per layer
    assert read >= 80


# -------------------------------------------------------------------------------------------------------------- part A
def test_every_libopenjp2_fixture_planned_again_is_the_file():
    candidates, same, failed = [], [], []
    for rel in tc.fixture_files():
        cs, parsed = tc.read_fixture(rel)
        if not tc.is_candidate(cs, parsed):
            continue
        candidates.append(rel)
        if rel in LEFT_OUT:
            continue
        try:
            params = tc.params_for(api, rel, cs)
            f = tc.header_fields(cs)
            numbps, pieces, data = tc.table_from_reader(api, params, cs, parsed)
            # one layer: no allocation, the blocks go to cblk_dst as a frame without rate control has them
            plan = tc.plan_table(api, params, f["style"], f["layers"], numbps, pieces, with_alloc=f["layers"] > 1)
            out = api.assemble(plan, data)
        except (ValueError, api.J2kHipError, AssertionError, KeyError) as e:
            failed.append((rel, repr(e)))
            continue
        if out == cs:
            same.append(rel)
        else:
            at = next((i for i, (a, b) in enumerate(zip(out, cs)) if a != b), min(len(out), len(cs)))
            failed.append((rel, "first difference at byte %d of %d (file: %d)" % (at, len(out), len(cs))))
    print("part A: %d candidates, %d planned again to the file's bytes, %d left out" % (len(candidates), len(same), len(LEFT_OUT)))
    assert not failed, failed
    assert len(LEFT_OUT) <= 8 and set(LEFT_OUT) <= set(candidates)
    assert len(same) + len(LEFT_OUT) == len(candidates) and len(same) >= 63
    # the spread the candidates were chosen for
    fields = [tc.header_fields(tc.read_fixture(rel)[0]) for rel in same]
    assert {f["prog"] for f in fields} == {0, 1, 2, 3, 4}
    assert sum(1 for f in fields if f["tile"][0] < f["width"] or f["tile"][1] < f["height"]) >= 6
    assert {2, 3, 7, 12} <= {f["layers"] for f in fields}
    assert any(f["pp"] and f["pp"][-1] == (3, 3) and f["cblk"] == (4, 4) for f in fields)  # precincts of 8 x 8 at the top, blocks of 4 x 4
    assert {1, 2, 4, 16, 32} <= {f["style"] for f in fields} and any(f["style"] & 5 and f["layers"] > 1 for f in fields)


# -------------------------------------------------------------------------------------------------------------- part B
_results = {}


def run_case(name):
    """Table, plan and assembled codestream of a case, made once; `stats`: set once the oracle has read the table back -- its packet
    figures (tier2_cases.readback)."""
    if name not in _results:
        case = tc.case_named(name)
        t = tc.synth_table(api, case)
        plan = tc.plan_table(api, t["params"], case["style"], case["layers"], t["numbps"], t["pieces"], with_alloc=case["layers"] > 1)
        _results[name] = dict(table=t, plan=plan, cs=api.assemble(plan, t["data"]), stats=None)
    return _results[name]


@pytest.mark.parametrize("name", [c["name"] for c in tc.CASES])
def test_synthetic_table_reads_back(name):
    r = run_case(name)
    stats = tc.assert_reads_back(api, r["table"], r["cs"])
    f, case = tc.header_fields(r["cs"]), r["table"]["case"]
    assert (f["layers"], f["style"], f["prog"]) == (case["layers"], case["style"], case["mk"].get("progression", 0))
    r["stats"] = stats


@pytest.mark.parametrize("name", [c["name"] for c in tc.WORKER_CASES])
def test_tile_of_4096_blocks_planned_by_workers(name):
    """One tile of 4096 blocks: four workers write the packets of the (resolution, component) pairs side by side; the plan is
    the serial one, array for array, and reads back."""
    r = run_case(name)
    t, case = r["table"], r["table"]["case"]
    assert len(t["pieces"]) >= 4096 and len(set(t["fb"][:, 0].tolist())) == 1
    par = tc.plan_table(api, t["params"], case["style"], case["layers"], t["numbps"], t["pieces"], with_alloc=case["layers"] > 1, workers=4)
    ser = r["plan"]
    assert par["total_len"] == ser["total_len"] and np.array_equal(par["blob"], ser["blob"])
    assert all(np.array_equal(a, b) for a, b in zip(par["headers"], ser["headers"]))
    if case["layers"] > 1:
        assert all(np.array_equal(a, b) for a, b in zip(par["bodies"], ser["bodies"]))
    else:
        assert np.array_equal(par["cblk_dst"], ser["cblk_dst"])
    assert api.assemble(par, t["data"]) == r["cs"]
    r["stats"] = tc.assert_reads_back(api, t, r["cs"])


def test_guard_auto_plans_again_with_the_count_the_table_needs():
    """A table beyond the floor's bit-planes: a strict count refuses it, GUARD_AUTO plans it again at three guard bits -- QCD
    says three, and the reader, who takes Mb from QCD, finds the same table."""
    r = run_case(tc.GUARD_CASE["name"])
    t = r["table"]
    floor = api.frame_blocks(tc.make_params(api, t["case"], guard_bits=0))
    assert any(nb > mb for nb, mb in zip(t["numbps"], floor[:, 9].tolist()))
    assert r["plan"]["guard_bits"] == 3 and tc.header_fields(r["cs"])["guard"] == 3
    r["stats"] = tc.assert_reads_back(api, t, r["cs"])
    inp = tc.table_inputs(0, t["case"]["layers"], t["numbps"], t["pieces"], True)
    with pytest.raises(api.J2kHipError) as ei:
        api.host_tier2_plan(tc.make_params(api, t["case"], guard_bits=0), inp["numbps"], inp["npasses"], inp["length"], alloc=inp["alloc"])
    assert ei.value.code == J2K_HIP_ERR_OVERFLOW
    # at three, strictly: the same bytes
    fixed = api.host_tier2_plan(tc.make_params(api, t["case"], guard_bits=3), inp["numbps"], inp["npasses"], inp["length"], alloc=inp["alloc"])
    assert api.assemble(fixed, t["data"]) == r["cs"]


def test_plan_hook_refusals_and_the_length_hook():
    """The hook's own contract: per-pass byte counts are required under a style and refused without one; an allocation is
    np, len and off of the parameters' layers; the planned length is j2k_hip_debug_tier2's."""
    t = run_case("l1_17x9_grey8")["table"]
    inp = tc.table_inputs(0, 1, t["numbps"], t["pieces"], False)
    assert api.host_tier2_plan(t["params"], inp["numbps"], inp["npasses"], inp["length"])["total_len"] == \
        api.host_tier2(t["params"], inp["numbps"], inp["npasses"], inp["length"])
    rates = np.zeros((len(t["numbps"]), tc.MAX_PASSES), np.uint32)
    with pytest.raises(api.J2kHipError):
        api.host_tier2_plan(t["params"], inp["numbps"], inp["npasses"], inp["length"], rates=rates)
    with pytest.raises(api.J2kHipError):
        api.host_tier2_plan(tc.make_params(api, t["case"], cblk_style=4), inp["numbps"], inp["npasses"], inp["length"])
    two = tuple(np.zeros((len(t["numbps"]), 2), np.uint32) for _ in range(3))
    with pytest.raises(api.J2kHipError):
        api.host_tier2_plan(t["params"], inp["numbps"], inp["npasses"], inp["length"], alloc=two)
    with pytest.raises(api.J2kHipError):
        api.host_tier2_plan(t["params"], inp["numbps"][:-1], inp["npasses"][:-1], inp["length"][:-1])
    # a piece list given in part is a parameter error, a capacity too small an overflow
    L, out, one = api.load_library(), api.Tier2Plan(), np.zeros(64, np.uint64)
    args = (t["params"], inp["numbps"].ctypes.data, inp["npasses"].ctypes.data, inp["length"].ctypes.data, inp["numbps"].size, None, None, None, None, 0, 0)
    out.hdr_dst, out.hdr_cap = one.ctypes.data, one.size
    assert L.j2k_hip_debug_tier2_plan(api.C.byref(args[0]), *args[1:], api.C.byref(out)) == 1
    out = api.Tier2Plan()
    out.cblk_dst, out.cblk_cap = one.ctypes.data, 1
    assert L.j2k_hip_debug_tier2_plan(api.C.byref(args[0]), *args[1:], api.C.byref(out)) == J2K_HIP_ERR_OVERFLOW


def test_census():
    """The corpus reaches every class it was made for -- counted on the input tables and the geometry, not on what the planner
    wrote; the 0xFF classes on the packet headers of plans the oracle has confirmed."""
    names = [c["name"] for c in tc.CASES + tc.WORKER_CASES + [tc.GUARD_CASE]]
    for n in names:
        r = run_case(n)
        if r["stats"] is None:
            r["stats"] = tc.assert_reads_back(api, r["table"], r["cs"])
    c = tc.census([_results[n]["table"] for n in names])
    headers = [h for n in names for h in tc.packet_headers(_results[n]["plan"])]
    assert sum(_results[n]["stats"][0] for n in names) == len(headers)  # a header piece per packet the reader read
    ff_inside = sum(1 for h in headers if b"\xff" in h[:-2])   # a 0xFF with a stuffed bit and more of the header behind it
    # The header's last bit is the last bit of a 0xFF byte, so that one more byte must follow: by the reader's own bit position
    # (the bytes alone cannot tell: FF 00 at a header's end is also a 0xFF and up to seven zero bits of the header).  Without that
    # byte the reader takes the body's first byte for it and nothing reads back: BitWriter::flush cut down to one byteout()
    # fails the cases counted here.
    ff_at_end = sum(_results[n]["stats"][1] for n in names)
    assert all(_results[n]["stats"][1] == _results[n]["table"]["case"]["layers"] for n in names if n.startswith("ffend_"))  # made for it
    assert all(h[-2:] == b"\xff\x00" for n in names if n.startswith("ffend_") for h in tc.packet_headers(_results[n]["plan"]))
    print("census: %d cases, %d blocks, %d packets, most passes in one packet %d, %d headers with 0xFF inside, %d ending on it"
          % (len(names), c["blocks"], len(headers), c["max_passes"], ff_inside, ff_at_end))
    print({k: (sorted(v, key=str) if isinstance(v, set) else v) for k, v in c.items() if k != "lengths"})
    # Table B.4: each of the five codes at a first inclusion and in a later layer
    assert c["b4_first"] == {0, 1, 2, 3, 4} and c["b4_later"] == {0, 1, 2, 3, 4} and c["max_passes"] == 70 == 3 * c["max_Mb"] - 2
    # length fields
    kmax = tc.flog2(c["max_cap"])
    assert c["zero_len"] > 0 and kmax >= 14 and {1} | {(1 << k) - d for k in range(1, kmax + 1) for d in (0, 1)} <= c["lengths"]
    assert c["lblock_packet"] and c["three_rises"] > 0
    # tag trees: every grid with every layer-0 pattern (one leaf: all or none)
    grids = ("1x1", "1xn", "nx1", "2x2", "3x5", "16+")
    assert {(g, p) for g in grids for p in tc.PATTERNS if g != "1x1" or p in ("all", "none")} <= c["grids"]
    assert c["zbp_full"] > 0 and c["zbp_Mb"] == c["max_Mb"] == 24
    # layers
    assert c["layer_counts"] == set(range(1, 8)) and c["first_layers_of_7"] == set(range(7))
    assert c["skip_middle"] > 0 and c["never"] > 0 and c["empty_frames"] > 0
    # styles (under termall no segment spans a layer boundary: every pass ends one)
    assert c["seg_termall"] > 0 and c["seg_bypass_1"] > 0 and c["seg_bypass_2"] > 0 and c["seg_both"] > 0 and c["boundary_in_segment"] > 0
    assert c["late_rise"] == {1, 4, 5}
    assert c["progressions"] == {0, 1, 2, 3, 4}
    assert ff_inside > 0 and ff_at_end >= 3


# -------------------------------------------------------------------------------------------------------------- part C
@pytest.mark.parametrize("name", [c["name"] for c in tc.CASES])
def test_libopenjp2_takes_the_assembled_file(opj, name):
    """Not the reference, a further reader: libopenjp2 decodes the assembled file without failing (the block bytes are random,
    the samples mean nothing).  Skips where the library is absent."""
    opj.decode_comps(run_case(name)["cs"])
