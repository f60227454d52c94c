"""The Tier-1 encode slots at their capacity edge, on the GPU (run with -m gpu): j2k_hip_stage_t1_slots runs the modeller, the
coder and the rate fix-up of a frame on slots whose capacities the test chooses, between guard stripes, and hands back the
kernels' error word and both arenas whole.  The six checked stores -- the modeller's 1 KiB flush and final drain (error word
2), the 16-byte unit flush and the 4-byte final drain of the two-wave coder in both instantiations and of the styled coder
(error word 3) -- are the only thing between a block that does not fit and its neighbour's codeword.

The blocks, capacities and launches are t1_capacity_cases.py's; test_t1_capacity_refs.py asserts on the CPU that they reach
the edges and that the guard stripes hold whatever a kernel without any check would write.  Per launch:

  fits        (both capacities at or above round_up(need, 16)): bit-planes, passes, the decisions byte for byte, length,
              codeword bytes -- and the pass rates when read -- are the oracle's, whatever the lanes beside the block did.  This pins the
              contract "a slot of round_up(decisions, 16) / round_up(length, 16) bytes suffices".
  short of decisions: error word 2, the block reported empty (no passes, no decisions, length 0), its codeword slot untouched.
  short of codeword: error word 3; the modeller's results are the oracle's, the slot holds the codeword's first out_cap
              bytes, the length reported is the whole codeword's.  With both kinds in a launch: 2 or 3.
  error word 0 only in the all-fitting launch, where every block is exact.
  always      every guard byte of both arenas still holds the fill; behind a fitting block's codeword (rounded up to the 4-byte
              word of the final drain: the one to three bytes behind the codeword in that word are the coder's stage, which the
              plain coder does not define) and behind its decisions (rounded up to 16) the slot holds the fill -- in the
              all-fitting launch and in the overflow launches alike, so no slot but a short block's own differs between them
              from there on.

The all-fitting launches of every setting run first (test order), then the overflow launches."""
import numpy as np
import pytest

import t1_capacity_cases as cc
from conftest import golden_case

pytestmark = pytest.mark.gpu

KNOBS = ("mq_window", "t1_sparse")


def _settings():
    out = []
    for rev, style in cc.COMBOS:
        for tables in (False, True):
            # (the pass-rate instantiation of the plain coder and the styled coder do not read mq_window)
            for window in ((0, -1, 2) if style == 0 and not tables else (0,)):
                for sparse in (-1, 0, 1):
                    out.append((rev, style, tables, window, sparse))
    return out


SETTINGS = _settings()


def _sid(s):
    rev, style, tables, window, sparse = s
    return f"{'rev' if rev else 'irr'}-style{style}-{'tables' if tables else 'plain'}-window{window}-sparse{sparse}"


@pytest.fixture(scope="module")
def api():
    from j2k_amd import api
    return api


@pytest.fixture(scope="module")
def enc(api):
    e = api.Encoder(0)
    before = {k: api.get_tune(k) for k in KNOBS}
    yield e
    for k, v in before.items():
        api.tune(k, v)
    e.close()


_launches = {}


def _launch_of(api, oracle, combo, kind):
    """(references, lanes, guard, plane, rectangles, orientations, steps) of a launch: built once, left unchanged."""
    key = (combo, kind)
    if key not in _launches:
        rs = cc.refs(oracle, combo)
        lanes = cc.launches(api, rs, combo[1])[kind]
        plane, rects, orients, steps = cc.launch_plane(lanes, combo[0])
        plane.setflags(write=False)
        _launches[key] = (rs, lanes, cc.guard_of(rs, lanes), plane, rects, orients, steps)
    return _launches[key]


def _run(api, enc, oracle, setting, kind):
    rev, style, tables, window, sparse = setting
    rs, lanes, guard, plane, rects, orients, steps = _launch_of(api, oracle, (rev, style), kind)
    before = {k: api.get_tune(k) for k in KNOBS}
    api.tune("mq_window", window)
    api.tune("t1_sparse", sparse)
    try:
        res = enc.stage_t1_slots(plane.copy(), rects, orients, steps, rev, style, [l["sym_cap"] for l in lanes],
                                 [l["out_cap"] for l in lanes], guard, want_passes=tables)
    finally:
        for k, v in before.items():
            api.tune(k, v)
    return rs, lanes, guard, res


def _check_rates(got, r, style, at):
    np_ = r["npasses"]
    got = [int(v) for v in got[:np_]]
    if not style:
        assert got == r["rates"], at
        return
    for p in range(np_):  # (as t1_styled_families.compare: exact where a segment ends and at the last pass)
        if r["seg_ends"][p] or p == np_ - 1:
            assert got[p] == r["rates"][p], at + (p,)
        assert got[p] <= r["len"] and (p == 0 or got[p - 1] <= got[p]), at + (p,)


def _check(rs, lanes, guard, res, style, kind):
    fill = res["fill"]
    kinds = {l["kind"] for l in lanes}
    want_err = {"fit": {0}, "short_sym": {2}, "short_out": {3}, "mixed": {2, 3}}[kind]
    assert res["err"] in want_err, (kind, res["err"])
    # every guard byte of both arenas
    for arena, offs, cap in ((res["sym"], res["sym_off"], "sym_cap"), (res["out"], res["out_off"], "out_cap")):
        end = 0
        for i, l in enumerate(lanes):
            o = int(offs[i])
            assert o - end == guard and np.all(arena[end:o] == fill), (kind, cap, "guard in front of lane", i)
            end = o + l[cap]
        assert arena.size - end == guard and np.all(arena[end:] == fill), (kind, cap, "last guard")
    exact = 0
    for i, l in enumerate(lanes):
        r = rs[l["block"]]
        at = (kind, i // 64, i % 64, l["kind"], r["name"], l["sym_cap"], l["out_cap"])
        so, oo = int(res["sym_off"][i]), int(res["out_off"][i])
        sym, out = res["sym"][so:so + l["sym_cap"]], res["out"][oo:oo + l["out_cap"]]
        got = tuple(int(res[k][i]) for k in ("numbps", "npasses", "nsym", "length"))
        data = np.frombuffer(r["data"], dtype=np.uint8)
        if l["kind"] == "short_sym":
            assert got == (r["numbps"], 0, 0, 0), at  # reported empty
            assert np.all(out == fill), at  # ... and the coder left its codeword slot alone
            continue
        assert got == (r["numbps"], r["npasses"], r["nsym"], r["len"]), at
        assert np.array_equal(sym[:r["nsym"]], r["symbols"]), at  # the decisions, up against the slot's end
        assert np.all(sym[r["need_sym"]:] == fill), at
        if l["kind"] == "short_out":
            assert np.array_equal(out, data[:l["out_cap"]]), at  # the units and words that fit, nothing else
            continue
        assert np.array_equal(out[:r["len"]], data), at
        assert np.all(out[cc.round_up(r["len"], 4):] == fill), at
        if "rates" in res:
            _check_rates(res["rates"][i], r, style, at)
        exact += 1
    assert exact == sum(l["kind"] == "fit" for l in lanes) > 0
    assert kinds == {"fit": {"fit"}, "short_sym": {"fit", "short_sym"}, "short_out": {"fit", "short_out"},
                     "mixed": {"fit", "short_sym", "short_out"}}[kind]


@pytest.mark.parametrize("setting", SETTINGS, ids=_sid)
def test_all_fitting_launch(api, enc, oracle, setting):
    """Error word 0, every block exact: slots of exactly round_up(need, 16) bytes, of 16 more, and the rule's own."""
    rs, lanes, guard, res = _run(api, enc, oracle, setting, "fit")
    assert guard == 1024
    _check(rs, lanes, guard, res, setting[1], "fit")


@pytest.mark.parametrize("setting", SETTINGS, ids=_sid)
def test_overflow_launches(api, enc, oracle, setting):
    """Decision shortages (error word 2), codeword shortages (3), both (2 or 3): the short blocks are reported, the fitting
    blocks beside them in every workgroup are exact, and nothing is written outside a slot."""
    for kind in cc.LAUNCH_KINDS[1:]:
        rs, lanes, guard, res = _run(api, enc, oracle, setting, kind)
        _check(rs, lanes, guard, res, setting[1], kind)


@pytest.mark.parametrize("combo", cc.COMBOS, ids=lambda c: f"{'rev' if c[0] else 'irr'}-style{c[1]}")
def test_handle_is_sound_after_an_overflow(api, enc, oracle, golden, combo):
    """After an overflow launch the same handle encodes a golden frame to its bytes, and stage_t1 of the same blocks at the
    default capacities gives the oracle's results."""
    from j2k_amd import synth
    rev, style = combo
    rs, lanes, guard, res = _run(api, enc, oracle, (rev, style, False, 0, api.get_tune("t1_sparse")), "mixed")
    assert res["err"] in (2, 3)
    g, pl, _, cs = golden_case(golden, "g1_64x64_grey_5lvl")
    frame, lay = synth.ae_frame(pl, g["prec"], row_pad_bytes=8)
    kw = g["params"]
    p = api.make_params(g["width"], g["height"], g["ncomp"], g["prec"], reversible=kw.get("reversible", True), ycc=kw.get("mct", False),
                        layers=kw.get("layers", 1), tile_size=kw.get("tile", 0), num_resolutions=kw.get("numres", 6),
                        cblk=tuple(kw.get("cblk", (64, 64))), comment="")
    assert enc.encode_host(frame, lay, p) == cs
    fits = list({l["block"]: l for l in lanes if l["kind"] == "fit"}.values())  # every block once
    assert sorted(l["block"] for l in fits) == list(range(len(rs)))
    plane, rects, orients, steps = cc.launch_plane(fits, rev)
    got = enc.stage_t1(plane.copy(), rects, orients, steps, rev, style=style)
    assert len(got) == len(rs)
    for l, o in zip(fits, got):
        r = rs[l["block"]]
        assert (o["numbps"], o["npasses"], o["data"]) == (r["numbps"], r["npasses"], r["data"]), r["name"]
        _check_rates(o["rates"], r, style, (r["name"],))


def test_hook_refuses_what_it_cannot_lay_out(api, enc, oracle):
    """Capacities that are no multiple of 16, under 16 or above the rule's value at Mb = 30, and a guard that is no multiple of
    16: J2K_HIP_ERR_PARAM, before any launch."""
    rs = cc.refs(oracle, (True, 0))
    lane = dict(block=4, sym_cap=rs[4]["need_sym"], out_cap=rs[4]["need_out"], kind="fit")
    plane, rects, orients, steps = cc.launch_plane([lane], True)
    top = api.cblk_capacities(rs[4]["area"], 30, 0)
    ok = (lane["sym_cap"], lane["out_cap"], 1024)
    for sc, oc, g in ((ok[0] + 8, ok[1], ok[2]), (ok[0], ok[1] - 4, ok[2]), (0, ok[1], ok[2]), (ok[0], 0, ok[2]),
                      (top[0] + 16, ok[1], ok[2]), (ok[0], top[1] + 16, ok[2]), (ok[0], ok[1], 1032)):
        with pytest.raises(api.J2kHipError) as ei:
            enc.stage_t1_slots(plane.copy(), rects, orients, steps, True, 0, [sc], [oc], g)
        assert ei.value.code == 1, (sc, oc, g)
    res = enc.stage_t1_slots(plane.copy(), rects, orients, steps, True, 0, [top[0]], [top[1]], 0)  # the largest slots, no guard
    assert res["err"] == 0 and int(res["length"][0]) == rs[4]["len"]
    assert res["out"][:rs[4]["len"]].tobytes() == rs[4]["data"]
