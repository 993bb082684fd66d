"""tests/tail_ref.py, the plain restatement of MarkerDetector::detect's tail (src/markerdetector.cpp:371-382, 417-447), pinned on the CPU:
hand-computed chain cases, the near-tie pairs and their teeth, the border rectangle against handle code compiled with the host compiler,
and the border filter against the compiled oracle on frames whose marker touches the rectangle. test_gpu_tail_edges.py holds
finalize_kernel to the same reference on the same cases."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import tail_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chain_cases_by_hand():
    """Every rule of the same-id dedupe (:421-430) and its order before the border filter (:433-447), each run worked out by hand in
    tail_ref.CHAINS: > is strict, a removed neighbour still takes part in the next comparison's guard, a winner outside the rectangle
    leaves nothing."""
    ids, corners, members = ref.chain_frame()
    assert (ids == -1).sum() >= 8                      # undecoded candidates sit between the runs
    kept = ref.finalize(ids, corners, ref.border_rect(ref.W, ref.H))
    assert [int(ids[i]) for i in kept] == sorted(int(ids[i]) for i in kept)
    for name, (per, want) in ref.CHAINS.items():
        run = members[name]
        assert [float(ref.perimeter(corners[i])) for i in run] == [float(abs(p)) for p in per], name
        assert [ref.inside(corners[i], ref.border_rect(ref.W, ref.H)) for i in run] == [p > 0 for p in per], name
        assert [run.index(i) for i in kept if i in run] == want, name
    # the three rules most easily lost in a rewrite
    assert ref.CHAINS["triple_10_5_7"][1] == [0, 2] and ref.CHAINS["pair_tie"][1] == [1] and ref.CHAINS["winner_outside"][1] == []
    assert len(ref.CHAINS["four_5_10_7_8"][0]) == 4


def test_runs_of_four_in_every_order():
    """A run of four equal ids in every order of its perimeters against a direct reading of the loop: candidate i + 1 goes when it is
    smaller than i, else i goes, and the pair is skipped when i + 1 is already gone (which the forward loop never finds: it is the guard
    that keeps a removed i in play)."""
    rect = ref.border_rect(ref.W, ref.H)
    seen = set()
    for per, corners in ref.permutation_chains():
        rem = [False] * 4
        for i in range(3):
            if per[i] > per[i + 1]:
                rem[i + 1] = True
            else:
                rem[i] = True
        want = [i for i in range(4) if not rem[i]]
        assert ref.finalize([7] * 4, corners, rect) == want, per
        seen.add(len(want))
    assert seen == {1, 2}                              # one survivor, or two of the same id


def test_sort_is_stable_and_skips_undecoded():
    rect = ref.border_rect(ref.W, ref.H)
    for n in (1, 63, 64, 65, 130, 512):
        ids, corners = ref.order_frame(n, 100 + n, distinct=True)
        kept = ref.finalize(ids, corners, rect)
        assert kept == [i for i in np.argsort(ids, kind="stable") if ids[i] != -1]      # distinct ids inside the rectangle: all are kept
        ids, corners = ref.order_frame(n, 200 + n)
        kept = ref.finalize(ids, corners, rect)
        assert all((ids[a], a) < (ids[b], b) for a, b in zip(kept, kept[1:]))
        assert n < 4 or {0, 1, 1023, 2 ** 31 - 1} <= set(int(i) for i in ids)


def test_near_tie_pairs_have_teeth():
    """The perimeter is a float32 running sum of double norms (utils.h:39-46). On at least a quarter of the near-tie pairs a sum kept in
    double decides differently, so a kernel that accumulates in the wrong type fails on them; the pairs are chosen for it in tail_ref."""
    ids, corners, disagree = ref.near_tie_pairs()
    rect = ref.border_rect(ref.W, ref.H)
    npairs = len(ids) // 2
    differs = 0
    for k in range(npairs):
        a, b = corners[2 * k], corners[2 * k + 1]
        assert ref.inside(a, rect) and ref.inside(b, rect)
        p32, p64 = (ref.perimeter(a), ref.perimeter(b)), (ref.perimeter64(a), ref.perimeter64(b))
        assert abs(float(p32[0]) - float(p32[1])) <= 4 * float(np.spacing(p32[0]))       # a near tie
        assert ((p32[0] > p32[1]) != (p64[0] > p64[1])) == (k in disagree)
        differs += k in disagree
    assert 4 * differs >= npairs
    k32, k64 = ref.finalize(ids, corners, rect), ref.finalize(ids, corners, rect, perimeter=ref.perimeter64)
    assert len(k32) == len(k64) == npairs and sum(a != b for a, b in zip(k32, k64)) == differs


def test_border_values_round_half_to_even():
    rect = ref.border_rect(100, 60)
    assert rect == (2, 2, 98, 58)
    sq = lambda v: ref.border_probe(rect, (0, 0), np.float32(v))
    # 1.5 -> 2: inside; an ulp below -> 1: outside
    assert ref.inside(sq(1.5), rect) and not ref.inside(sq(np.nextafter(np.float32(1.5), np.float32(0))), rect)
    assert ref.inside(sq(97.5), rect) is False          # 97.5 -> 98: the bound is open
    assert ref.inside(sq(np.nextafter(np.float32(97.5), np.float32(0))), rect)
    assert ref.inside(sq(2.5), rect) and not ref.inside(sq(-0.5), rect) and not ref.inside(sq(-0.49), rect)
    zero = ref.border_rect(100, 60, 0.0)
    assert zero == (0, 0, 100, 60)
    assert ref.inside(ref.border_probe(zero, (0, 0), np.float32(-0.5)), zero) and not ref.inside(ref.border_probe(zero, (0, 0), np.float32(-0.51)), zero)
    assert ref.inside(ref.border_probe(zero, (0, 0), np.float32(99.49)), zero) and not ref.inside(ref.border_probe(zero, (0, 0), np.float32(99.5)), zero)


def test_border_rect_of_the_handle_equals_the_plain_rectangle(tmp_path):
    """aruco_amd/csrc/border_rect.h, which make_detect_params hands to finalize_kernel, compiled with the host compiler alone
    (tests/cpp/border_rect_check.cpp) against recover_ref.border_rect for the table of sizes and border distances: the half-way products
    (100 x 60 -> [2, 98) x [2, 58), 180 x 100 -> [4, 176) x [2, 98), 300 x 140 -> [8, 292) x [4, 136)), t = 0, the empty rectangle of
    t = 0.5, the swapped one of t = 0.6, and a 1 x 1 frame."""
    exe = str(tmp_path / "border_rect_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "border_rect_check.cpp"), "-o", exe], check=True)
    table = [(w, h, t) for (w, h) in ref.RECT_TABLE_SIZES for t in ref.RECT_TABLE_T]
    args = [str(v) for row in table for v in (row[0], row[1], repr(float(np.float32(row[2]))))]
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(table)
    for (w, h, t), line in zip(table, lines):
        got = line.split()
        assert (int(got[0]), int(got[1])) == (w, h) and np.float32(got[2]) == np.float32(t), line
        assert tuple(int(v) for v in got[3:]) == ref.border_rect(w, h, t), (w, h, t, line)
    assert ref.border_rect(100, 60) == (2, 2, 98, 58) and ref.border_rect(180, 100) == (4, 2, 176, 98) and ref.border_rect(300, 140) == (8, 4, 292, 136)
    assert ref.border_rect(640, 480, 0.5) == (320, 240, 320, 240) and ref.border_rect(100, 60, 0.6) == (40, 24, 60, 36)
    assert ref.border_rect(1, 1) == (0, 0, 1, 1)


def test_tail_capacity_status_and_given_up_frames():
    """tail(): what the project puts around the reference's tail, on a frame that keeps five markers"""
    rng = np.random.RandomState(3)
    fr = (np.arange(5, dtype=np.int32), ref.random_quads(rng, 5))
    empty = (np.zeros(0, np.int32), np.zeros((0, 8), np.float32))
    t = ref.tail([fr], ref.W, ref.H, cap_markers=4, out_cap=3)
    assert t["n"] == [5] and t["status"] == ref.ST_MARKER_OVERFLOW and t["rows"] == [[0, 1, 2, 3]] and t["out_rows"] == [[0, 1, 2]]
    assert t["list"] == {0, 1, 2, 3} and t["hdr"] == (5, 32)
    t = ref.tail([fr], ref.W, ref.H, cap_markers=5, out_cap=9)
    assert t["n"] == [5] and t["status"] == 0 and t["out_rows"] == [[0, 1, 2, 3, 4]] and t["hdr"] == (5, 0)
    t = ref.tail([fr, fr, empty], ref.W, ref.H, cap_markers=8, plane_status=[[0, 0, 0], [0, 0, 4], [0, 0, 0]])
    assert t["n"] == [5, -1, 0] and t["status"] == 4 and t["rows"][1] is None and t["hdr"] is None
    assert t["list"] == {0, 1, 2, 3, 4}
    t = ref.tail([fr], ref.W, ref.H, cap_markers=8, border_dist=0.5)
    assert t["n"] == [0] and t["list"] == set()


# ---- the oracle leg ---------------------------------------------------------------------------------------------------------------------
ORACLE_SIZES = ref.HALFWAY_SIZES


def oracle_corners(o_free, frame):
    ms = o_free.detect(frame)
    if [m["id"] for m in ms] != [ref.ORACLE_ID]:
        return None
    c = ms[0]["corners"]
    assert np.array_equal(c, np.rint(c))                # corner method NONE: contour points
    return c


@functools.lru_cache(maxsize=None)
def oracle_leg_cases(width, height):
    """[(name, frame, the marker's corners without a border filter, the oracle's ids with it)] of one size, or None where the oracle does
    not find the centred marker. Shared with test_gpu_tail_edges.py."""
    from oracle import orc

    o_free, o = orc.Oracle(corner_method=0, border_dist=0.0), orc.Oracle(corner_method=0)
    leg = ref.oracle_leg(width, height, functools.partial(oracle_corners, o_free))
    if leg is None:
        return None
    return [(name, frame, oracle_corners(o_free, frame), [m["id"] for m in o.detect(frame)]) for name, frame in leg]


@pytest.mark.parametrize("size", ORACLE_SIZES, ids=lambda s: "%dx%d" % s)
def test_border_filter_equals_the_oracle_on_a_marker_at_the_rectangle(size):
    """One synthetic marker, corner method NONE, moved so that its extreme corner lies on b0 - 1, b0, b1 - 1 and b1 of the border rectangle
    in x and in y: the compiled oracle keeps or drops it as tail_ref says of the corners the oracle itself reports without a border
    filter. The oracle finds the centred 35-px marker at all three half-way sizes (100 x 60, 180 x 100, 300 x 140)."""
    cases = oracle_leg_cases(*size)
    assert cases is not None, "the oracle does not find the centred marker at %d x %d" % size
    rect = ref.border_rect(*size)
    assert len(cases) == 9 and cases[0][3] == [ref.ORACLE_ID]
    verdicts = []
    for name, frame, corners, ids in cases:
        assert corners is not None, name                                  # found without the filter at every placement
        axis = "xy".index(name[0]) if name != "centre" else None
        if axis is not None:                                              # the placement is what its name says
            target = int(name.split()[-1])
            assert int(corners[:, axis].min() if " lo " in name else corners[:, axis].max()) == target, name
        want = ref.finalize([ref.ORACLE_ID], corners.reshape(1, 8), rect)
        assert ids == [ref.ORACLE_ID] * len(want), name
        verdicts.append(len(want))
    assert verdicts == [1, 0, 1, 1, 0, 0, 1, 1, 0]                        # b0 - 1 out, b0 in, b1 - 1 in, b1 out
