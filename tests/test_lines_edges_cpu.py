"""The reference side of the LINES edge tests, pinned before the device is compared with it: the CPU restatement of refineCandidateLines
(oracle/orc_detect.cpp: refine_lines, centred double normal equations) against tests/lines_ref.py (uncentred float64 least squares by SVD,
Python integers for the walk's size_t arithmetic) on every non-hostile case, the measurement behind lines_ref.FINE_BOUND_SPACINGS, and the
proof that the families tell five deliberately wrong readings of the reference from the right one. The hostile cases are never handed
to the oracle: with an empty side its fit_line reads p[0] of an empty vector."""
import numpy as np
import pytest

from tests import lines_ref as ref

FAMILIES = ("raster", "start", "length", "inverse", "short", "duplicate", "tie", "far", "lens")
_worst = {}


def oracle_side(family):
    """(worst spacings from f32lines, its case, worst relative deviation from exact) of the oracle over one family, once per process."""
    from oracle import orc

    if family not in _worst:
        ws, wn, wr = 0.0, None, 0.0
        for c in ref.families()[family]:
            r = ref.reference(c)
            got = orc.refine_lines(c["contour"], c["corners"], K=None if c["K"] is None else c["K"].reshape(-1), dist=c["dist"])
            assert np.all(np.isfinite(got)), c["name"]
            s = float(ref.spacings(got, r["f32lines"]).max())
            if s > ws or wn is None:
                ws, wn = max(s, ws), c["name"] if s >= ws else wn
            wr = max(wr, ref.rel_dev(got, r["exact"]))
        _worst[family] = (ws, wn, wr)
    return _worst[family]


def test_families_hold_what_they_promise():
    fam = ref.families()
    assert set(fam) == set(FAMILIES) | {"hostile"}
    total = sum(len(fam[f]) for f in FAMILIES)
    print("%d non-hostile cases: %s" % (total, ", ".join("%s %d" % (f, len(fam[f])) for f in FAMILIES)))
    assert 500 <= total <= 900
    assert all(len(fam[f]) >= 4 for f in FAMILIES)
    assert {len(c["contour"]) for c in fam["length"]} >= {63, 64, 65, 127, 128, 129, 513}
    assert len(fam["start"]) == 16 * len(fam["raster"])
    assert not any(ref.reference(c)["inverse"] for c in fam["raster"]) and all(ref.reference(c)["inverse"] for c in fam["inverse"])
    # every raster angle, plain and in perspective, is walked backwards too, and so is every tie shape; each again under every lens
    rev = [c for c in fam["inverse"] if c["name"].startswith("rev_")]
    assert len(rev) == len(fam["raster"]) == 2 * len(ref.ANGLES)
    assert {c["name"].split("_")[1] for c in rev} == {"a%d" % a for a in ref.ANGLES}
    assert sum(ref.reference(c)["inverse"] for c in fam["tie"]) == sum(not ref.reference(c)["inverse"] for c in fam["tie"]) == 4
    assert sum(c["name"].startswith("inverse_rev_") for c in fam["lens"]) == 3 * len(rev)
    # forward sides that pass through contour index 0, and sides below, at and above one wave of 64 points
    assert any(any(s[-1] < s[0] for s in ref.reference(c)["sides"]) for c in fam["start"])
    lens = {len(s) for f in ("length", "raster", "start") for c in fam[f] for s in ref.reference(c)["sides"]}
    assert {63, 64, 65} <= lens and min(lens) < 16 and max(lens) > 256
    assert {len(c["dist"]) for c in fam["lens"]} == {5} and any(not np.any(c["dist"]) for c in fam["lens"])
    assert max(int(c["contour"].max()) for c in fam["far"]) > 16300 and len(fam["hostile"]) >= 6


@pytest.mark.parametrize("family", FAMILIES)
def test_oracle_equals_the_reference(family):
    ws, wn, wr = oracle_side(family)
    print("%-9s oracle: worst %.3f float32 spacings from f32lines (%s), worst %.3g relative from exact" % (family, ws, wn, wr))
    assert wr <= ref.REL_TOL
    assert ws <= ref.FINE_BOUND_SPACINGS


def test_fine_bound_is_the_measured_one():
    """The bound in lines_ref.py is four times the recorded worst of the oracle over every non-hostile family, at least 4, and this
    measurement stays inside it (the recorded worst is this measurement as committed; another LAPACK may round one coefficient otherwise)."""
    worst = max(oracle_side(f)[0] for f in FAMILIES)
    for f in FAMILIES:
        print("%-9s oracle worst %.3f spacings" % (f, oracle_side(f)[0]))
    print("measured worst %.3f spacings, bound %.1f" % (worst, max(4.0 * worst, 4.0)))
    assert ref.FINE_BOUND_SPACINGS == max(4.0 * ref.ORACLE_WORST_SPACINGS, 4.0)
    assert 4.0 * worst <= ref.FINE_BOUND_SPACINGS


def _leaves_the_bound(cases, wrong):
    """(cases whose wrong reading is a finite result outside the fine bound, cases it turns hostile or non-finite)."""
    out, undefined = [], []
    for c in cases:
        r = ref.reference(c)
        w = ref.refine(c["contour"], c["corners"], c["K"], c["dist"], wrong=wrong)
        if w["hostile"] is not None or not np.all(np.isfinite(w["f32lines"])):
            undefined.append(c["name"])
        elif ref.spacings(w["f32lines"], r["f32lines"]).max() > ref.FINE_BOUND_SPACINGS:
            out.append(c["name"])
    return out, undefined


@pytest.mark.parametrize("wrong,family", [("first", "duplicate"), ("wrap", "inverse"), ("nonext", "short"), ("ge", "tie"), ("dropend", "raster"),
                                          ("dropend", "far")])
def test_families_tell_a_wrong_reading_from_the_right_one(wrong, family):
    """First match instead of last; a wrap to n - 1 instead of the size_t modulo; no added next corner; >= in the span test; one end
    point dropped from one side (which 1e-4 relative cannot see at x = 16300: 1.6 px). Each leaves the fine bound in its own family."""
    cases = ref.families()[family]
    if wrong == "wrap":
        cases = [c for c in cases if len(c["contour"]) & (len(c["contour"]) - 1)]
        assert cases
    caught, undefined = _leaves_the_bound(cases, wrong)
    print("%s: %d of %d %s cases give a finite result outside the fine bound, %d no defined result" % (wrong, len(caught), len(cases), family, len(undefined)))
    assert caught
    if wrong == "dropend":
        # and the project's relative tolerance alone would have let the far ones through
        seen = [c for c in cases if ref.rel_dev(ref.refine(c["contour"], c["corners"], c["K"], c["dist"], wrong=wrong)["f32lines"],
                                                ref.reference(c)["exact"]) <= ref.REL_TOL]
        print("dropend: %d of %d %s cases pass 1e-4 relative" % (len(seen), len(cases), family))
        assert family != "far" or seen


def test_hostile_cases_are_recognised_without_running_them():
    for c in ref.families()["hostile"]:
        r = ref.refine(c["contour"], c["corners"])
        print("%-24s %s" % (c["name"], r["hostile"]))
        assert r["hostile"] is not None
        assert r["terminates"] == (not c["name"].startswith("endless"))
        assert len(c["contour"]) <= 2000
