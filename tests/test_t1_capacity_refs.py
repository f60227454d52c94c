"""CPU: the cases of the Tier-1 slot tests (tests/t1_capacity_cases.py) meet their conditions on the oracle alone, and the slot
rule (cblk_capacities) holds the oracle's decisions and codewords of blocks with Mb and with Mb + 1 bit-planes.

No device runs here.  What test_t1_capacity.py compares on the GPU means something only if the blocks come close to a flush
unit of their slots' ends, if every coder workgroup of an overflow launch mixes fitting and short lanes, and if the guard
stripes are wide enough that a kernel with no capacity check at all would still write inside the arena: all asserted here.
The rule's half: the families of rule_families for Mb = 1 .. 12, the argument's bound on the decisions (decisions_bound),
a literal copy of the rule before its fix (old_capacities) for the capacities that must not move, and a seeded search over
1- and 2-bit frames for a block that outgrows its old slot."""
import pytest

import t1_capacity_cases as cc


@pytest.fixture(scope="module")
def api():
    from j2k_amd import api
    return api


def _ids(c):
    return f"{'rev' if c[0] else 'irr'}-style{c[1]}"


def test_edge_seeds_are_what_the_search_finds(oracle):
    assert cc.search_edge_seeds(oracle) == (list(cc.EDGE_SEEDS), cc.EDGE_TRIED)
    assert (cc.search_exact_seed(oracle, True), cc.search_exact_seed(oracle, False)) == cc.EXACT_SEEDS


@pytest.mark.parametrize("combo", cc.COMBOS, ids=_ids)
def test_blocks_reach_the_edges(oracle, combo):
    rs = cc.refs(oracle, combo)
    assert [r["name"] for r in rs[:9]] == ["noise64", "sparse64", "one64", "noise32", "noise16", "lap37x13", "noise4x4", "noise1x64", "noise64x1"]
    assert [r["area"] for r in rs[:9]] == [4096, 4096, 4096, 1024, 256, 37 * 13, 16, 64, 64]
    met = set().union(*(cc.edge_conditions_of(r) for r in rs))
    assert met == set(cc.EDGE_CONDITIONS), met  # decisions within 16 of a multiple of 1024 from below and above; length 0, 1, 15 mod 16
    # ... and one exactly at it: the modeller's last flush ends where a slot of need_sym bytes ends
    assert any(r["nsym"] > cc.KFLUSH and r["nsym"] % cc.KFLUSH == 0 for r in rs)
    nsym, ln = [r["nsym"] for r in rs], [r["len"] for r in rs]
    assert max(nsym) > 2 * cc.KFLUSH and min(nsym) < cc.KFLUSH
    assert max(ln) > 6 * 1024 and min(ln) < 16 and min(ln) > 0
    assert all(3 * r["numbps"] - 2 <= 96 for r in rs)  # (the per-pass tables: error word 1 is out of reach)
    by = {r["name"]: r for r in rs}
    assert by["noise64"]["nsym"] > 60 * cc.KFLUSH and by["noise64"]["len"] > 400 * 16  # many flushes, hundreds of units
    assert by["one64"]["numbps"] == 1 and by["one64"]["len"] < 16 and cc.KFLUSH < by["one64"]["nsym"] <= cc.KFLUSH + 16


@pytest.mark.parametrize("combo", cc.COMBOS, ids=_ids)
def test_lanes_launches_and_guards(oracle, api, combo):
    rs = cc.refs(oracle, combo)
    style = combo[1]
    lanes = cc.lanes_of(api, rs, style)
    for i, r in enumerate(rs):
        mine = [l for l in lanes if l["block"] == i]
        ns, no = r["need_sym"], r["need_out"]
        rule = cc.rule_caps(api, r, style)
        assert rule[0] >= ns and rule[1] >= no, r["name"]  # the rule's own slot holds the block
        sc = {l["sym_cap"] for l in mine if l["out_cap"] == no}
        oc = {l["out_cap"] for l in mine if l["sym_cap"] == ns}
        long = r["nsym"] > cc.KFLUSH
        want_s = {c for c in (ns - 1024, ns - 16) if c >= 16} | {ns, ns + 16} | ({16, 1008} if long else set())
        want_o = {c for c in (no - 16,) if c >= 16} | {no, no + 16} | ({16} if long else set())
        assert sc == want_s and oc == want_o, r["name"]
        assert any((l["sym_cap"], l["out_cap"]) == rule for l in mine)
    top = {a: api.cblk_capacities(a, 30, style) for a in {r["area"] for r in rs}}
    for l in lanes:
        r = rs[l["block"]]
        short = cc.shortage(rs, l)
        assert (short[0] > 0) + (short[1] > 0) == (0 if l["kind"] == "fit" else 1)  # one kind of shortage per lane
        assert (l["kind"] == "short_sym") == (short[0] > 0) and (l["kind"] == "short_out") == (short[1] > 0)
        for cap, lim in zip((l["sym_cap"], l["out_cap"]), top[r["area"]]):
            assert cap % 16 == 0 and 16 <= cap <= lim  # what the hook accepts
    ls = cc.launches(api, rs, style)
    assert list(ls) == list(cc.LAUNCH_KINDS)
    assert {l["kind"] for l in ls["fit"]} == {"fit"}
    # every lane of every kind runs somewhere
    key = lambda l: (l["block"], l["sym_cap"], l["out_cap"], l["kind"])
    assert {key(l) for v in ls.values() for l in v} == {key(l) for l in lanes}
    assert {l["kind"] for l in ls["short_sym"]} == {"fit", "short_sym"} and {l["kind"] for l in ls["short_out"]} == {"fit", "short_out"}
    assert {l["kind"] for l in ls["mixed"]} == {"fit", "short_sym", "short_out"}
    for kind, v in ls.items():
        assert 64 < len(v) <= 512
        g = cc.guard_of(rs, v)
        assert g % 16 == 0
        for l in v:  # the safety condition: a store with no check at all stays inside the arena
            assert all(g >= s + 1024 for s in cc.shortage(rs, l))
        if kind == "fit":
            continue
        for w in range(0, len(v), 64):  # lane mix: every coder workgroup holds fitting and short lanes
            kinds = {l["kind"] for l in v[w:w + 64]}
            assert "fit" in kinds and len(kinds) >= 2, (kind, w)


# ---------------------------------------------------------------------------------------------------- the rule against the oracle
def test_rule_is_the_old_one_from_three_bit_planes_on(api):
    """Byte for byte, every area, every style class: the arenas of every frame with Mb >= 3 in all its bands -- every frame of
    more than two bits -- are what they were.  Mb = 1 and 2 grew, and only the decision term's difference explains it."""
    for style in (0, 5):
        for Mb in range(0, 38):
            for area in list(range(1, 130)) + list(range(130, 4097, 7)) + [64 * 63, 4096]:
                new, old = api.cblk_capacities(area, Mb, style), cc.old_capacities(area, Mb, style)
                if Mb >= 3:
                    assert new == old, (area, Mb, style)
                else:
                    want = cc.round_up(max(area * 3 * Mb // 2 + area + 64, (Mb + 2) * area + area // 4 + 16), 1024)
                    assert new[0] == want >= old[0] and new[1] == cc.round_up(want // 4 + 64 + (24 * Mb if style else 0), 16), (area, Mb, style)
    assert cc.old_capacities(4096, 1, 0) == (11264, 2880) and api.cblk_capacities(4096, 1, 0)[0] == 14336
    assert cc.old_capacities(64 * 63, 2, 0)[0] == 16384 and api.cblk_capacities(64 * 63, 2, 0)[0] == 17408


_worst = {}


def _family_results(oracle, Mb):
    """Per (shape, planes) the oracle's (family, decisions, codeword bytes per style) -- each block coded once per style."""
    if Mb not in _worst:
        import numpy as np
        out = []
        for w, h in cc.RULE_SHAPES:
            for p in (Mb, Mb + 1):
                for name, mag in cc.rule_families(w, h, p, 100 * Mb + p):
                    rng = np.random.default_rng(7)
                    data = ((mag * cc.signs(rng, mag.shape)) << 6).astype(np.int32)
                    lens = {}
                    for style in cc.STYLES:
                        r = oracle.t1_block(data, (w + p) % 4, style=style, want_symbols=True)
                        assert r["numbps"] == p, (name, w, h, p)
                        lens[style] = len(r["data"])
                    out.append(dict(w=w, h=h, p=p, name=name, nsym=len(r["symbols"]), lens=lens))
        _worst[Mb] = out
    return _worst[Mb]


# Measured on the oracle, per Mb: the most decisions per sample and plane over the blocks of Mb planes and of Mb + 1 planes
# (the argument's (p + 1.25) / p, met by run_breaks), and the most codeword bytes per decision (the rule counts a quarter
# byte; among blocks of at least 256 decisions).  DESIGN section 8 quotes this table.
WORST = {
    1: (2.125, 1.75, 0.134), 2: (1.75, 1.5, 0.167), 3: (1.5, 1.375, 0.167), 4: (1.375, 1.3, 0.163),
    5: (1.3, 1.25, 0.165), 6: (1.25, 1.214, 0.168), 7: (1.214, 1.188, 0.165), 8: (1.188, 1.167, 0.166),
    9: (1.167, 1.15, 0.166), 10: (1.15, 1.136, 0.163), 11: (1.136, 1.125, 0.167), 12: (1.125, 1.115, 0.162),
}


@pytest.mark.parametrize("Mb", list(cc.RULE_MBS))
def test_rule_holds_blocks_of_Mb_and_one_more_bit_plane(oracle, api, Mb):
    res = _family_results(oracle, Mb)
    per_plane = {Mb: 0.0, Mb + 1: 0.0}
    per_dec = 0.0
    for b in res:
        area = b["w"] * b["h"]
        assert b["nsym"] <= cc.decisions_bound(b["w"], b["h"], b["p"]), b  # the argument's bound
        per_plane[b["p"]] = max(per_plane[b["p"]], b["nsym"] / (area * b["p"]))
        for style in cc.STYLES:
            sym_cap, out_cap = api.cblk_capacities(area, Mb, style)
            assert b["nsym"] <= sym_cap, (b, style, sym_cap)
            assert b["lens"][style] <= out_cap, (b, style, out_cap)
            if b["nsym"] >= 256:
                per_dec = max(per_dec, b["lens"][style] / b["nsym"])
    # run_breaks meets the bound in 64 x 64 blocks (from two planes on: with one, the other samples never turn significant)
    hit = [b for b in res if b["name"] == "run_breaks" and (b["w"], b["h"]) == (64, 64) and b["p"] >= 2]
    assert [b["nsym"] for b in hit] == [cc.decisions_bound(64, 64, b["p"]) for b in hit] == [(4 * b["p"] + 5) * 1024 for b in hit]
    got = (round(per_plane[Mb], 3), round(per_plane[Mb + 1], 3), round(per_dec, 3))
    print("Mb", Mb, "decisions per sample-plane (Mb, Mb + 1 planes), bytes per decision:", got)
    assert got == WORST[Mb]


def test_old_rule_lost_the_over_blocks_of_one_and_two_bit_planes(oracle):
    """The finding: under the rule as it stood a block of Mb + 1 planes outgrew the decision slot of Mb = 1, and of Mb = 2 where
    the rounding to 1 KiB left no room (64 x 63); Mb + 1 planes fit from Mb = 3 on, Mb planes always."""
    lost = set()
    for Mb in cc.RULE_MBS:
        for b in _family_results(oracle, Mb):
            if b["nsym"] > cc.old_capacities(b["w"] * b["h"], Mb, 0)[0]:
                assert b["p"] == Mb + 1
                lost.add((Mb, b["w"], b["h"]))
    assert {m for m, _, _ in lost} == {1, 2}
    assert (1, 64, 64) in lost and (2, 64, 63) in lost and (2, 64, 64) not in lost


def test_no_small_frame_of_the_search_outgrows_its_old_slot(oracle):
    """1- and 2-bit frames at guard_bits = 1 (search_small_frames): whether the old rule's overflow was reachable from a
    frame.  None of the frames tried holds such a block -- the worst block takes 0.80 of its old slot -- so DESIGN says "not
    reached in 2000 frames"; the rule is fixed either way."""
    tried, seen, found, worst = cc.search_small_frames(oracle)
    assert (tried, seen, found) == (2000, 22000, [])
    assert round(worst, 2) == 0.80
