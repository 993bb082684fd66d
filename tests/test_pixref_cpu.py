"""The reference side of the pixel-refinement edge tests, pinned before the device is compared with it: the CPU restatements of cv::cornerSubPix,
SubPixelCorner::RefineCorner and findCornerMaxima (oracle/orc_detect.cpp, oracle/orc_extra.cpp) against tests/pixref.py on every family, the
measurement behind pixref.ORACLE_WORST_PX, the cap on the fragile share of every family, and the proof that the families hold the branches and
shapes they are named for. Nothing here runs on the device."""
import collections

import numpy as np
import pytest

from tests import pixref as ref


def oracle_call(frame, width, pts, method, win, wsize):
    from oracle import orc

    p = pts
    if wsize:
        p = orc.find_corner_maxima(frame, p, wsize, width=width)
    if method == ref.SUBPIX:
        p = orc.corner_subpix(frame, p, win=win, width=width)
    elif method == ref.HARRIS:
        p = orc.corner_harris(frame, p, width=width)
    return p


_oracle = {}


def oracle_side(family):
    """The oracle's results of one family, once per process."""
    if family not in _oracle:
        _oracle[family] = ref.run(ref.families()[family], oracle_call)
    return _oracle[family]


def records(family, part="refine"):
    return [ref.reference(c)["record"][part] for c in ref.families()[family]]


def test_families_hold_what_they_promise():
    fam = ref.families()
    assert set(fam) == set(ref.FAMILIES)
    print(", ".join("%s %d" % (f, len(fam[f])) for f in ref.FAMILIES))
    sub = lambda f: [c for c in fam[f] if c["method"] == "subpix"]
    assert {c["win"] for c in sub("interior")} == {c["win"] for c in sub("border")} == set(ref.WINS) == {1, 2, 3, 7, 9, 15}
    assert any(c["pt"][0] % 1 == 0.5 for c in fam["interior"]) and any(c["pt"][0] % 0.125 == 0 and c["pt"][0] % 0.5 for c in fam["interior"])
    # border: starts on the first and last row and column, in every image corner, and a frame smaller than the 33 x 33 patch
    for W, H in ((64, 48), (48, 64)):
        pts = {c["pt"] for c in sub("border") if c["image"][1:3] == (W, H)}
        assert {(0.0, 0.0), (W - 1.0, 0.0), (0.0, H - 1.0), (W - 1.0, H - 1.0)} <= pts
        assert {p[0] for p in pts} >= {0.0, W - 1.0} and {p[1] for p in pts} >= {0.0, H - 1.0}
    assert any(c["image"][1:3] == (16, 12) and c["win"] == 15 for c in sub("border"))
    assert {c["stride"] - c["image"][1] for c in fam["stride"]} == {3, 13} and len(fam["stride"]) == 2 * (len(fam["interior"]) + len(fam["locked_interior"]))
    assert {c["method"] for c in fam["stride"]} == {"subpix", "harris", "locked"}
    assert all(r["exit"] == "det" and r["iters"][0]["det"] == 0 for r in records("degenerate"))
    esc = records("escape")
    n_reset = sum(r["reset"] and r["exit"] != "left" for r in esc)
    n_left_reset, n_left = sum(r["exit"] == "left" and r["reset"] for r in esc), sum(r["exit"] == "left" and not r["reset"] for r in esc)
    print("escape: %d resets after a walk inside the image, %d breaks with a reset, %d breaks without" % (n_reset, n_left_reset, n_left))
    assert min(n_reset, n_left_reset, n_left) >= 4
    # and four corners that move by exactly `win` and are kept: the reset asks for more than win
    rim = [(c, ref.reference(c)) for c in fam["escape"] if c["image"][0] == "rim"]
    assert len(rim) == 8 and all(not r["record"]["refine"]["reset"] and not r["fragile"] for _, r in rim)
    assert {tuple(r["exact"] - np.array(c["pt"])) for c, r in rim} == {(1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (0.0, -1.0)}
    assert all(np.array_equal(r["exact"], r["f32path"]) for _, r in rim)
    print("starts left out because `exact` magnifies a displacement of 1e-6 px more than %g times: %s" % (ref.MAX_AMPLIFICATION, ref.dropped))
    assert len(ref.dropped) <= 4
    full = sum(r["exit"] == "maxiter" for r in records("maxiter"))
    print("maxiter: %d of %d cases run all 8 iterations" % (full, len(fam["maxiter"])))
    assert all(c["win"] == 1 for c in fam["maxiter"]) and 3 * full >= len(fam["maxiter"])
    # the SUBPIX exits over all families
    exits = collections.Counter(r["exit"] for f in ("interior", "border", "escape", "maxiter") for c, r in zip(fam[f], records(f)) if c["method"] == "subpix")
    assert set(exits) == {"eps", "maxiter", "left"} and min(exits.values()) >= 8
    # HARRIS quirks on the tall frame: y in (W, H] is skipped, y == W is not, x < 0 and y < 0 are
    tall = [(c, r) for c, r in zip(fam["quirk"], records("quirk")) if c["image"][1:3] == (48, 64)]
    assert all((r["exit"] == "skipped") == (c["pt"][0] < 0 or c["pt"][1] < 0 or c["pt"][1] > 48) for c, r in tall)
    assert sum(48 < c["pt"][1] <= 64 for c, _ in tall) >= 4 and sum(c["pt"][1] == 48 for c, _ in tall) >= 2 and sum(c["pt"][0] < 0 for c, _ in tall) >= 2
    assert any(c["pt"][1] == 48 and r["exit"] == "step" for c, r in tall)
    assert any(c["pt"][0] % 1 for c in fam["interior"] if c["method"] == "harris")      # fractional 16.16 weights
    # locked corners: the window shapes
    shapes = lambda f: {r["window"][2:] for r in records(f, "locked")}
    assert {(2 * w, 2 * w) for w in (5, 7, 15, 31)} <= shapes("locked_interior")
    clipped = shapes("clipped")
    assert any(rw != rh for rw, rh in clipped) and (1, 1) in clipped and any(rw == 1 and rh > 1 for rw, rh in clipped) and any(rh == 1 and rw > 1 for rw, rh in clipped)
    assert any(rw > rh for rw, rh in clipped) and any(rw < rh for rw, rh in clipped) and all(rw >= 1 and rh >= 1 for rw, rh in clipped)
    assert all(min(s) < 9 for s in shapes("thin")) and {(2, 2), (6, 6), (8, 8)} <= shapes("thin")
    assert all(r["exit"] == "nopeak" for r in records("nopeak", "locked"))
    assert any(tuple(ref.reference(c)["exact"]) == (-1.0, -1.0) for c in fam["nopeak"]) and any(ref.reference(c)["exact"][0] > 0 for c in fam["nopeak"])
    # twin: an exact tie, the first in raster order taken, on the lower and on the higher lane of the two
    order = collections.Counter()
    for c, r in zip(fam["twin"], records("twin", "locked")):
        (b, bi), (s, si) = r["best"], r["second"]
        assert b == s > 0 and bi < si and r["window"][2:] == (62, 62), c["name"]
        rw = 62
        assert abs(bi % rw - si % rw) >= 10 and abs(bi // rw - si // rw) >= 10
        assert all(6 <= i % rw < rw - 6 and 6 <= i // rw < rw - 6 for i in (bi, si))
        assert abs(bi % rw - 31) + abs(bi // rw - 31) == abs(si % rw - 31) + abs(si // rw - 31)
        order[bi % 64 < si % 64] += 1
    print("twin: the winner on the lower lane %d times, on the higher lane %d times" % (order[True], order[False]))
    assert min(order[True], order[False]) >= 4
    # chain: the refiners are handed (-1, -1)
    assert sum(tuple(r["pt"]) == (-1.0, -1.0) for r in records("chain", "locked")) >= 3
    assert {c["method"] for c in fam["chain"]} == {"locked+subpix", "locked+harris"}
    assert len(ref.many_points(7)) == 7


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_fragile_share_is_capped(family):
    """No family may have more than 5 % of its cases fragile; which cases are is decided by `exact` alone."""
    cs = ref.families()[family]
    kinds = collections.Counter(k for c in cs for k in ref.reference(c)["fragile"])
    n = sum(bool(ref.reference(c)["fragile"]) for c in cs)
    print("%-16s %4d cases, %d fragile (%.1f %%): %s" % (family, len(cs), n, 100.0 * n / len(cs), dict(kinds)))
    assert n <= ref.FRAGILE_CAP * len(cs)


def _worst(family):
    """{method: (worst deviation of the oracle from `exact` in px over the non-fragile cases that are not exact by definition, its case)}."""
    w = {}
    for c, got in zip(ref.families()[family], oracle_side(family)):
        r = ref.reference(c)
        if r["fragile"] or c["method"] == "locked" or ref.returns_start(c):
            continue
        d, m = float(np.max(np.abs(got.astype(np.float64) - r["exact"]))), ref.bound_key(c["method"])
        if d >= w.get(m, (-1.0, None))[0]:
            w[m] = (d, c["name"])
    return w


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_oracle_equals_the_reference(family):
    """Integer results and returned starts bit for bit; the rest within 1e-4 relative of `exact` (a fragile case: of its neighbouring result),
    and `f32path`, which rounds where the published code rounds, within the fine bound of the oracle."""
    bad, worst_rel, worst_f32 = [], 0.0, 0.0
    for c, got in zip(ref.families()[family], oracle_side(family)):
        r = ref.reference(c)
        if "fragile_det" in r["fragile"]:
            continue
        wants = [r["exact"]] + list(r["accept"])
        if c["method"] == "locked" or ref.returns_start(c):
            ok = any(np.array_equal(got.astype(np.float64), w) for w in wants)
            if c["method"] == "locked" and not r["fragile"]:
                ok = ok and np.array_equal(r["f32path"], r["exact"])
        else:
            rel = min(ref.rel_dev(got, w) for w in wants)
            worst_rel = max(worst_rel, rel)
            ok = bool(np.all(np.isfinite(got))) and rel <= ref.REL_TOL
            if not r["fragile"]:
                worst_f32 = max(worst_f32, float(np.max(np.abs(got.astype(np.float64) - r["f32path"]))))
        if not ok:
            bad.append((c["name"], got.tolist(), r["exact"].tolist()))
    print("%-16s oracle: worst %.3g relative from exact, %.3g px from f32path; %s" % (family, worst_rel, worst_f32, {m: "%.3g px" % d for m, (d, _) in _worst(family).items()}))
    assert not bad, bad[:6]


def test_fine_bound_is_the_measured_one():   # -k measured
    """pixref.ORACLE_WORST_PX is this measurement, as committed: per method the oracle's worst deviation from `exact` over every non-fragile
    case of every family (run with -k measured -s for the figures per family)."""
    worst = {}
    for f in ref.FAMILIES:
        w = _worst(f)
        print("%-16s %s" % (f, ", ".join("%s %.3g px (%s)" % (m, d, n) for m, (d, n) in sorted(w.items()))))
        for m, (d, _) in w.items():
            worst[m] = max(worst.get(m, 0.0), d)
    print("measured worst: %s" % {m: float("%.3g" % d) for m, d in worst.items()})
    assert set(worst) == set(ref.ORACLE_WORST_PX) == {"subpix", "harris"}
    for m, d in worst.items():
        assert ref.ORACLE_WORST_PX[m] == float("%.3g" % d), (m, d)
        assert ref.FINE_BOUND_PX[m] == 4.0 * ref.ORACLE_WORST_PX[m]


def _wrong_result(c, wrong):
    img = ref.image(c["image"])
    if c["method"] == "subpix":
        return ref.subpix(img, c["pt"], c["win"], wrong=wrong)["pt"]
    if c["method"] == "harris":
        return ref.harris(img, c["pt"], wrong=wrong)["pt"]
    return ref.locked(img, c["pt"], c["wsize"], wrong=wrong)["pt"]


@pytest.mark.parametrize("wrong,method,family", [("clamp", "subpix", "border"), ("iter7", "subpix", "maxiter"), ("ge", "subpix", "escape"), ("noround", "harris", "interior"),
                                                 ("fixedy", "harris", "interior"), ("fixedy", "harris", "quirk"), ("lasttie", "locked", "twin"),
                                                 ("rim", "locked", "clipped"), ("rim", "locked", "locked_interior"), ("den", "locked", "clipped"),
                                                 ("den", "locked", "locked_interior")])
def test_families_tell_a_wrong_reading_from_the_right_one(wrong, method, family):
    """A right clamp at W - 2; 7 iterations; a reset at exactly `win`; no rounding of the 8-bit patch; the y update in its "fixed" form; the last
    of equal maxima; one more row of block sums; weights over rw + rh. Each is judged wrong by the rule the device is judged by, in its family."""
    cases = [c for c in ref.families()[family] if c["method"] == method and not ref.reference(c)["fragile"]]
    caught = [c["name"] for c in cases if not ref.judge(c, _wrong_result(c, wrong))[0]]
    print("%s: %d of %d %s cases fail" % (wrong, len(caught), len(cases), family))
    assert len(caught) >= 2
