"""Border following at its edge topologies, without a GPU (tests/border_ref.py): the plain reading of cv::findContours equals the oracle's on every
case, the walker formulation equals the size-filtered scan on every case, the cases reach the device's thresholds (asserted from the traces), and they
tell every misreading of the scan and of the formulation from the right reading."""
import numpy as np
import pytest

from tests import border_ref as B


def same(a, b):
    return len(a) == len(b) and all(x["hole"] == y["hole"] and tuple(x["trig"]) == tuple(y["trig"]) and np.array_equal(x["pts"], y["pts"])
                                    for x, y in zip(a, b))


@pytest.fixture(scope="module")
def cases():
    """per case: family, index, format, image, the scan's borders, the kept ones, the formulation's survivors and candidate traces, border traces"""
    res = []
    for fam, i, fmt, img in B.all_cases():
        W, H = B.FORMATS[fmt][:2]
        lo, hi = B.limits(fmt)
        borders = B.scan_borders(img)
        kept = B.size_filter(borders, lo, hi)
        cand = []
        surv = B.walk_survivors(img, lo, hi, traces=cand)
        res.append({"fam": fam, "i": i, "fmt": fmt, "img": img, "borders": borders, "kept": kept, "surv": surv, "cand": cand,
                    "traces": [B.border_trace(c, W, H) for c in borders], "kept_traces": [B.border_trace(c, W, H) for c in kept]})
    return res


def test_size_limits_of_the_formats():
    assert B.limits("sheet") == (10, 1024) and B.limits("strip") == (40, 4096) and B.limits("odd") == (10, 1012) and B.limits("reach") == (10, 256)


def test_scan_equals_the_oracle(cases):
    from oracle import orc
    for c in cases:
        assert same(c["borders"], orc.find_contours(c["img"])), (c["fam"], c["i"])


def test_formulation_equals_the_filtered_scan(cases):
    for c in cases:
        assert same(c["surv"], c["kept"]), (c["fam"], c["i"])


def test_the_probe_length_does_not_change_the_survivors(cases):
    """a backward proof is a proof at any distance: the survivors with no probe and with one of 64 steps are the same"""
    for c in cases:
        if c["fam"] == "noise" and c["fmt"] != "odd":
            continue      # one noise image is bulk enough for this
        lo, hi = B.limits(c["fmt"])
        for probe in (0, 64):
            assert same(B.walk_survivors(c["img"], lo, hi, probe=probe), c["kept"]), (c["fam"], c["i"], probe)


def test_every_listed_length_as_outer_and_as_hole(cases):
    for fmt, lengths in (("sheet", B.SHEET_LENGTHS), ("strip", B.STRIP_LENGTHS)):
        lo, hi = B.limits(fmt)
        have = {(t["hole"], t["n"]) for c in cases if c["fam"] == "lengths" and c["fmt"] == fmt for t in c["traces"]}
        kept = {(t["hole"], t["n"]) for c in cases if c["fam"] == "lengths" and c["fmt"] == fmt for t in c["kept_traces"]}
        for n in lengths:
            for hole in (0, 1):
                assert (hole, n) in have, (fmt, hole, n)
                assert ((hole, n) in kept) == (lo < n < hi), (fmt, hole, n)
        assert {lo, lo + 1, hi - 1, hi} <= set(lengths)


def test_straight_lines_at_the_early_exit(cases):
    """n == 2 * reach at max_contour - 2 (kept) and at max_contour (the early exit's own boundary), both polarities"""
    lo, hi = B.limits("reach")
    ts = [t for c in cases if c["fam"] == "reach" for t in c["traces"]]
    for hole in (0, 1):
        assert any(t["hole"] == hole and t["n"] == hi - 2 for t in ts) and any(t["hole"] == hole and t["n"] == hi for t in ts)
    assert sum(t["n"] == 2 * t["reach"] == hi - 2 for t in ts) >= 4 and sum(t["n"] == 2 * t["reach"] == hi for t in ts) >= 4
    longs = [t for c in cases if c["fam"] == "reach" for t in c["cand"] if t["verdict"] == "long"]
    assert any(t["n"] == hi // 2 for t in longs)          # ended by the reach, not by the step count


def test_start_pixel_passes_and_pixel_visits(cases):
    ts = [t for c in cases for t in c["kept_traces"]]
    for hole in (0, 1):
        assert any(t["hole"] == hole and t["start_passes"] == 2 for t in ts)
    # three passes cannot be built (border_ref's docstring gives the argument): no border of any case, noise included, has them
    assert max(t["start_passes"] for c in cases for t in c["traces"]) == 2
    for k in (2, 3, 4):
        assert any(t["visits"][k] > 0 for t in ts), k
    for hole in (0, 1):
        assert any(t["hole"] == hole and t["max_visits"] == 4 for t in ts)


def test_false_starts_die_in_every_stage(cases):
    designed = [t for c in cases if c["fam"] != "noise" for t in c["cand"]]
    backs = {(t["hole"], t["back"]) for t in designed if t["back"] is not None}
    for hole in (0, 1):
        assert (hole, 9) in backs and (hole, 10) in backs and (hole, 11) in backs
        assert any(t["hole"] == hole and t["verdict"] == "probe" and t["back"] == 10 for t in designed)
        assert any(t["hole"] == hole and t["verdict"] != "probe" and t["back"] == 11 for t in designed)
        stages = {t["stage"] for t in designed if t["hole"] == hole and t["verdict"] == "bad"}
        assert {"first", 1, 2, 3} <= stages and any(isinstance(s, int) and s >= 4 for s in stages), (hole, stages)
        # around the hand-overs themselves: a proof found in the last step of a stage and in the first of the next
        fw = {t["fwd"] for t in designed if t["hole"] == hole and t["verdict"] == "bad"}
        print("forward proofs, hole %d: %s" % (hole, sorted(fw)))
        assert {64, 65, 192, 193, 448, 449, 960, 961} <= fw, hole


def test_each_hole_clause_fires_alone(cases):
    proofs = {t["clauses"] for c in cases for t in c["cand"] if t["hole"] and t["verdict"] in ("bad", "probe")}
    designed = {t["clauses"] for c in cases if c["fam"] != "noise" for t in c["cand"] if t["hole"] and t["verdict"] in ("bad", "probe")}
    for name in ("W", "E", "N"):
        assert (name,) in designed, (name, designed)
    assert not any("S" in p for p in proofs), proofs          # never first (border_ref: CLAUSE_MUTATIONS)


@pytest.mark.parametrize("mut", B.CLAUSE_MUTATIONS)
def test_a_left_out_hole_clause_only_delays_the_proof(cases, mut):
    """the survivors stay (no image can tell these misreadings by its result); for W, E and N some false start's proof moves"""
    moved = 0
    for c in cases:
        if c["fam"] not in ("hole_combs", "thin", "repass"):
            continue
        lo, hi = B.limits(c["fmt"])
        tr = []
        assert same(B.walk_survivors(c["img"], lo, hi, (mut,), traces=tr), c["kept"]), (c["fam"], c["i"])
        moved += sum((a["back"], a["fwd"]) != (b["back"], b["fwd"]) for a, b in zip(tr, c["cand"]))
    assert (moved > 0) == (mut != "hole_no_S"), (mut, moved)


def test_lengths_modulo_16_and_the_grid(cases):
    kept = [t for c in cases if c["fam"] != "noise" for t in c["kept_traces"]]
    for hole in (0, 1):
        assert {0, 1, 15} <= {t["mod16"] for t in kept if t["hole"] == hole}
    grid = [t for c in cases if c["fam"] == "grid" for t in c["kept_traces"]]
    for g in (8, 16, 32):
        assert any(t["grid"][g] == (False, False) for t in grid), g          # a border that carries only its start waypoint
        assert any(t["grid"][g] == (True, True) for t in grid), g
    assert any(t["grid"][8] == (False, False) and not t["hole"] for t in grid) and any(t["grid"][8] == (False, False) and t["hole"] for t in grid)


def test_borders_at_every_image_side(cases):
    for fmt in ("sheet", "odd", "strip"):
        ts = [t for c in cases if c["fam"] == "frame" and c["fmt"] == fmt for t in c["kept_traces"]]
        for side in range(4):
            for hole in (0, 1):
                assert any(t["frame"][side] == 0 and t["hole"] == hole for t in ts), (fmt, side, hole)
        # the scan clears the frame: the images hold set pixels on it
        for c in cases:
            if c["fam"] == "frame" and c["fmt"] == fmt and c["i"] % 4 == 0:
                assert c["img"][0].any() and c["img"][-1].any() and c["img"][:, 0].any() and c["img"][:, -1].any()


def test_hole_start_rule_pixel_in_the_last_column(cases):
    """column W - 2 holds a hole start-rule pixel that is no hole (see border_ref); W - 3 holds a true trigger"""
    for c in cases:
        if c["fam"] == "frame" and c["i"] % 4 == 0:
            W = B.FORMATS[c["fmt"]][0]
            b = c["img"] != 0
            assert (~b[2:-2, W - 2] & b[2:-2, W - 3] & b[1:-3, W - 2]).any()
            assert not any(t["hole"] and t["trig"][0] == W - 2 for t in c["borders"])
            assert any(t["hole"] and t["trig"][0] == W - 3 for t in c["kept"])


@pytest.fixture(scope="module")
def catches(cases):
    """mutation -> the designed families that tell it from the right reading (a family is asked case by case until one of its cases differs)"""
    res = {m: set() for m in B.MUTATIONS}
    for mut in B.MUTATIONS:
        for c in sorted(cases, key=lambda c: len(c["cand"])):
            if c["fam"] == "noise" or c["fam"] in res[mut]:
                continue
            lo, hi = B.limits(c["fmt"])
            if mut in B.SCAN_MUTATIONS:
                got = B.size_filter(B.scan_borders(c["img"], (mut,)), lo, hi, (mut,))
            else:
                got = B.walk_survivors(c["img"], lo, hi, (mut,))
            if not same(got, c["kept"]):
                res[mut].add(c["fam"])
    return res


@pytest.mark.parametrize("mut", B.MUTATIONS)
def test_mutation_is_caught(catches, mut):
    print(mut, "caught by", sorted(catches[mut]))
    assert catches[mut], mut


def test_every_family_is_needed(catches):
    """every designed family catches a mutation; the noise family is bulk beside them: it is there for candidates_sparse_kernel's dealt windows,
    full walker waves and generation lists with hundreds of entries"""
    for fam in B.FAMILIES:
        if fam != "noise":
            assert any(fam in v for v in catches.values()), fam
    # the families that are some mutation's only witness
    sole = {m: next(iter(v)) for m, v in catches.items() if len(v) == 1}
    print("sole witnesses:", sole)
    assert sole.get("keep_frame") == "frame" and sole.get("reach_gt") == "reach" and sole.get("outer_le") == "repass"
    assert catches["close_on_start"] <= {"repass", "thin"}
