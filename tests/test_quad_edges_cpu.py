"""The contour-to-candidate stage's edge cases on the CPU: every family of tests/quad_ref.py meets its precondition on every case (by the instrumented
reference), the oracle's pieces equal the reference on every case, and the cases tell deliberate misreadings of the reference from the right one.
"""
import math

import numpy as np
import pytest

from tests import quad_ref as Q


@pytest.fixture(scope="module")
def orc():
    from oracle import orc
    return orc


def traced(tile_, lo=25):
    """(border, Trace, quad) of every border of a tile that passes the sheets' size filter"""
    res = []
    for b in Q.borders_of(tile_ * 255):
        if len(b) > lo:
            tr = Q.Trace()
            res.append((b, tr, Q.border_quad(b, tr)))
    return res


def pattern(tr):
    return ["".join("NOFD"[k] if c[k] else "." for k in range(4)) for c in tr.clean]


def test_length_family_counts():
    lo, hi = Q.size_limits(Q.SHEET_W, Q.SHEET_H, Q.MIN_SIZE, Q.MAX_SIZE)
    counts = [len(Q.outer_border(t)) for _, t in Q.family("length")[0]]
    assert sorted(set(counts)) == sorted({511, 512, 513, 961, 1023, 1024, 1025, lo + 1, hi - 1})
    assert any("deg0" not in n for n, _ in Q.family("length")[0])
    for _, t in Q.family("length")[0]:
        assert lo < len(Q.outer_border(t)) < hi


def test_stride_family_remainders():
    counts = [len(Q.outer_border(t)) for _, t in Q.family("stride")[0]]
    for below in (True, False):
        assert sorted((c - 1) % 64 for c in counts if (c <= 512) == below) == [0, 1, 31, 32, 33, 63]
    # the half-wave scans: count - 1 = 0, 1 or 31 (mod 32) for some border too
    assert {0, 1, 31} <= {(c - 1) % 32 for c in counts}


def test_pairing_family_parity():
    lo, hi = Q.size_limits(Q.SHEET_W, Q.SHEET_H, Q.MIN_SIZE, Q.MAX_SIZE)
    for fam, parity in (("pairing_even", 0), ("pairing_odd", 1)):
        cases, sheets = Q.family(fam)
        assert len(sheets) == 1
        kept = [len(b) for b in Q.borders_of(sheets[0][0]) if lo < len(b) < hi]
        assert len(kept) % 2 == parity and len(kept) == len(cases)
        assert kept.count(40) >= 2 and 512 in kept and all(k <= 512 for k in kept)
        order = [len(Q.outer_border(t)) for _, t in cases]
        assert order[0] == 40 and order[1] == 512                       # the 40-point border beside the 512-point one
        assert all((a < 60) != (b < 60) for a, b in zip(order[3:], order[4:]))   # short and long in turns


def test_tie_family_has_ties_and_first_maximum_matters():
    changed = {}
    for name, t in Q.family("tie")[0]:
        (b, tr, q), = traced(t)
        assert tr.ties > 0 and q is not None, name
        sub = name.split("_")[0] + ("_" + name.split("_")[1] if name.startswith(("diamond", "kite")) else "")
        if sub.startswith("kite_lane"):
            # the tie of the first scan spans a multiple of 64 positions, and a lane keeping its last maximum changes the quad
            assert int(sub[9:]) in tr.tie_gaps and int(sub[9:]) % 64 == 0 and Q.border_quad(b, None, ("lane_last",)) != q, name
            continue
        changed[sub] = changed.get(sub, False) or Q.border_quad(b, None, ("last_max",)) != q
    assert set(changed) == {"diamond_tip2", "diamond_tip3", "kite_tip2", "kite_tip3", "hexagon"}
    assert all(changed.values()), changed


def test_eps_family_reaches_equality():
    """every case states what it reaches: a bump or notch of depth d on a border of 20 d points holds the split test with equality and is absorbed,
    one pixel less is absorbed without equality, one more splits the side"""
    seen = set()
    for name, t in Q.family("eps")[0]:
        res = traced(t)
        b, tr, q = max(res, key=lambda r: len(r[0]))
        parts = name.split("_")
        if len(parts) == 4 and parts[1] == "of":
            depth, d = int(parts[0].lstrip("bumpnotch")), int(parts[2])
            assert tr.n == 20 * d, name
            if depth == d:
                assert tr.eq_split > 0 and tr.raw == 4, name         # depth 0.05 n exactly: `<=` holds with equality
                seen.add((parts[0].rstrip("0123456789"), parts[3]))
            elif depth < d:
                assert tr.eq_split == 0 and tr.raw == 4, name
            else:
                assert tr.eq_split == 0 and tr.raw > 4, name
        elif name.startswith("turned15_of_15"):
            assert tr.n == 300 and tr.eq_split > 0 and tr.raw == 4 and q is not None, name   # equality against an oblique chord of length 5 t
            assert all(dx != 0 and dy != 0 for (dx, dy) in [(q[j][0] - q[j - 1][0], q[j][1] - q[j - 1][1]) for j in range(4)]), name
            seen.add(("turned", "top"))
        elif name.startswith("bump") and "deg" in name:
            assert tr.eq_split == 0 and tr.eq_clean == 0 and len(res) == 1, name      # a depth that is no whole number: either side of eps, never on it
        elif name == "clean_equal":
            assert tr.n == 160 and tr.eq_clean > 0 and q is not None and tr.raw == 7, name
            assert Q.border_quad(b, None, ("clean_lt",)) is None                         # the vertex that equality removes
        elif name == "axis_only":
            assert "N.F." in pattern(tr)       # near its neighbours' chord and in front of both: kept only because the chord is axis-aligned
        elif name == "sip_only":
            assert "NO.." in pattern(tr)       # near an oblique chord: kept only by the inner product
        else:
            raise AssertionError("a case without a precondition: " + name)
    assert seen == {(k, s) for k in ("bump", "notch") for s in ("top", "left")} | {("turned", "top")}


def test_vertex_family_depths():
    raws, depths, kept_at = {}, [], set()
    for name, t in Q.family("vertices")[0]:
        for b, tr, q in traced(t):
            assert tr.depth == tr.raw      # the bookkeeping's depth is the vertex count: contour_quad's early reject sees exactly tr.raw
            depths.append(tr.depth)
            raws.setdefault(tr.raw, set()).add(q is not None)
            if q is not None:
                kept_at.add(tr.depth)
            if name.startswith("raw"):
                assert tr.raw == int(name[3]) and q is not None, name
    assert 8 in depths and max(depths) >= 9
    for raw in (4, 5, 6, 7, 8):
        assert True in raws[raw], raw          # ends as an accepted quad
    assert 8 in kept_at and 7 in kept_at       # a quad at the deepest bookkeeping the device lets through, and one below it
    assert False in raws[8]                    # and a refused shape at 8
    assert all(not any(v) for k, v in raws.items() if k > 8)   # the reference refuses them as well


def corner_gaps(q0, q1):
    a, b = Q.thin_out([q0])[0], Q.thin_out([q1])[0]
    return sorted(math.hypot(a[c][0] - b[c][0], a[c][1] - b[c][1]) for c in range(4))


def survivors(t):
    return Q.detect_rectangles([Q.borders_of(t * 255)], Q.SHEET_W, Q.SHEET_H, Q.MIN_SIZE, Q.MAX_SIZE)


def test_integer_family_edges():
    quads, tiles = {}, dict(Q.family("integer")[0])
    for name, t in tiles.items():
        quads[name] = [(tr, q) for _, tr, q in traced(t)]
    for name, v, ok in (("side_10_0", 100, False), ("side_6_8", 100, False), ("side_8_6", 100, False), ("side_10_1", 101, True), ("side_10_2", 104, True),
                        ("side_11_0", 121, True)):
        for u in ("_u0", "_u-9"):
            (tr, q), = quads[name + u]
            assert len(tr.poly) == 4 and Q.is_convex(tr.poly)
            assert min((tr.poly[j][0] - tr.poly[j - 1][0]) ** 2 + (tr.poly[j][1] - tr.poly[j - 1][1]) ** 2 for j in range(4)) == v, name
            assert (q is not None) == ok
    for name in ("collinear_house", "collinear_bump"):
        (tr, q), = quads[name]
        assert q is None and len(tr.poly) == 5
    (tr, q), = quads["triangle_flat"]
    assert q is None and len(tr.poly) == 3
    # four vertices, one turn with a zero cross product, every side longer than 10: only the convexity test refuses it
    (tr, q), = quads["zero_cross_spur"]
    p = tr.poly
    turns = [(p[i][1] - p[i - 1][1]) * (p[i - 1][0] - p[i - 2][0]) - (p[i][0] - p[i - 1][0]) * (p[i - 1][1] - p[i - 2][1]) for i in range(4)]
    assert len(p) == 4 and turns.count(0) == 1 and Q.min_side(p) > 10 and q is None
    # thin frames: the outer border's quad and the hole's, corner by corner
    for t_ in (1, 2, 3, 5, 6):
        (_, qa), (_, qb) = quads["frame_%d" % t_]
        gaps = corner_gaps(qa, qb)
        assert gaps[0] == gaps[3] and (gaps[3] < 6) == (t_ <= 3), (t_, gaps)
        assert len(survivors(tiles["frame_%d" % t_])) == (1 if t_ <= 3 else 2)
        (_, qa), (_, qb) = quads["frame_%d_corner" % t_]
        moved = corner_gaps(qa, qb)
        assert moved[:3] == gaps[:3] and moved[3] > gaps[3], (t_, moved)          # exactly one corner moved
        assert len(survivors(tiles["frame_%d_corner" % t_])) == (1 if moved[3] < 6 else 2)
    for name, gap, kept in (("near_6", 6.0, 2), ("near_5", 5.0, 1)):
        (_, qa), (_, qb) = quads[name]
        gaps = corner_gaps(qa, qb)
        assert gaps[3] == gap and gaps[2] < gap, (name, gaps)                      # exactly one corner at 6 px (kept apart) / at 5 px (joined)
        assert len(survivors(tiles[name])) == kept, name
    assert len(quads["nested_frames"]) == 4 and len(quads["nested_frames_2px"]) == 5
    assert all(q is not None for _, q in quads["nested_frames"] + quads["nested_frames_2px"])
    assert len(survivors(tiles["nested_frames"])) == 1 and len(survivors(tiles["nested_frames_2px"])) == 1


def test_orientation_is_never_zero_on_a_frame():
    """o = (q1 - q0) x (q2 - q0) of a quad that passed the convexity test is a non-zero integer, and below 2^24 on every frame here (on the 16368 x 72
    one too: 16368 * 72 < 2^24), so its float32 products are exact and `o == 0` cannot come from a frame. The reading `o < 0` (a zero leaves the
    order) is pinned on a hand-made degenerate quad."""
    flat = [(0, 0), (20, 0), (40, 0), (20, 30)]
    assert Q.thin_out([flat]) == [flat]
    sheets = [s for _, _, s in Q.all_sheets()] + [Q.far_sheet()]
    n = 0
    for s in sheets:
        traces = []
        Q.detect_rectangles([Q.borders_of(s)], s.shape[1], s.shape[0], 0.001 if s.shape[1] > Q.SHEET_W else Q.MIN_SIZE, Q.MAX_SIZE, (), traces)
        for _, q in traces:
            if q is not None:
                o = (q[1][0] - q[0][0]) * (q[2][1] - q[0][1]) - (q[1][1] - q[0][1]) * (q[2][0] - q[0][0])
                assert 0 < abs(o) < 2 ** 24
                n += 1
    assert n > 150


def test_multi_plane_cases():
    """(15, 1): every plane gives the same two outer quads with equal perimeters (ties), the holes' quads differ between the planes.
    (9, 3): the holes' quads form a chain of near-duplicates whose ends are not near each other."""
    g = Q.multi_frame()
    for (p1, rng), nplanes in zip(Q.MULTI_PARAMS, (3, 7)):
        assert len(Q.plane_windows(p1, rng)) == nplanes
        per_plane = []
        for borders in Q.multi_planes(g, p1, rng):
            traces = []
            Q.detect_rectangles([borders], Q.SHEET_W, Q.SHEET_H, Q.MULTI_MIN, Q.MULTI_MAX, (), traces)
            qs = [q for _, q in traces]
            assert len(qs) == 4 and all(q is not None for q in qs)       # hole, outer, hole, outer
            per_plane.append(qs)
        for k in (1, 3):       # the outer quads: identical on every plane, so their perimeters tie
            assert all(pl[k] == per_plane[0][k] for pl in per_plane)
        for k in (0, 2):       # the holes' quads: the first and the last plane's differ, and each is near the next plane's
            assert per_plane[0][k] != per_plane[-1][k]
            assert all(corner_gaps(a[k], b[k])[3] < 6 for a, b in zip(per_plane, per_plane[1:]))
            assert Q.perimeter(per_plane[0][k]) > Q.perimeter(per_plane[-1][k])
        if rng == 3:
            assert corner_gaps(per_plane[0][0], per_plane[-1][0])[3] >= 6          # a chain, not a cluster
        assert len(Q.multi_candidates(g, p1, rng)) == Q.MULTI_COUNT[(p1, rng)]


def test_revisit_family_walks_pixels_twice():
    for name, t in Q.family("revisit")[0]:
        b = Q.outer_border(t)
        assert len(set(b)) < len(b), name


def test_oracle_pieces_equal_the_reference(orc):
    n = 0
    for fam in Q.FAMILIES:
        for name, t in Q.family(fam)[0]:
            for b in Q.borders_of(t * 255):
                if len(b) < 8:
                    continue
                for rule, mut in ((1, ()), (0, ("no_sip",))):
                    got = orc.approx_poly(np.array(b), len(b) * 0.05, rule)
                    assert [tuple(p) for p in got.tolist()] == [tuple(p) for p in Q.approx_poly(b, len(b) * 0.05, None, mut)], (fam, name)
                poly = Q.approx_poly(b, len(b) * 0.05)
                if len(poly) >= 3:
                    assert orc.is_contour_convex(poly) == Q.is_convex(poly), (fam, name)
                n += 1
    assert n > 200


def oracle_candidates(orc, sheet, min_size=Q.MIN_SIZE, max_size=Q.MAX_SIZE):
    o = orc.Oracle(thres_method=0, thres_p1=100.0, min_size=min_size, max_size=max_size)
    o.detect_raw(255 - sheet)
    return np.array([c["quad0"] for c in o.candidates()], np.float32).reshape(-1, 4, 2)


def test_oracle_detect_equals_the_reference_on_every_sheet(orc):
    for fam, i, sheet in Q.all_sheets():
        assert np.array_equal(oracle_candidates(orc, sheet), Q.sheet_candidates(sheet)), (fam, i)
    far = Q.far_sheet()
    ref = Q.sheet_candidates(far, 0.001, 0.5)
    assert len(ref) == 3 and ref[..., 0].max() > 16350
    assert np.array_equal(oracle_candidates(orc, far, 0.001, 0.5), ref)


def test_oracle_detect_equals_the_reference_on_several_planes(orc):
    g = Q.multi_frame()
    for p1, rng in Q.MULTI_PARAMS:
        o = orc.Oracle(thres_method=1, thres_p1=float(p1), thres_p2=7.0, thres_range=rng, min_size=Q.MULTI_MIN, max_size=Q.MULTI_MAX)
        o.detect_raw(g)
        got = np.array([c["quad0"] for c in o.candidates()], np.float32).reshape(-1, 4, 2)
        assert np.array_equal(got, Q.multi_candidates(g, p1, rng)), (p1, rng)


def test_early_reject_search_reaches_deep_borders():
    """the search behind contour_quad's limit of 8 vertices is only worth its answer where it produces borders of more than 8: a short seeded run does,
    and none of them ends as a quad"""
    tried, deep, found = Q.search_early_reject(2, float("inf"), shapes=150)
    assert tried == 150 and deep > 0 and found == []


# the family (or the several-plane case) whose cases tell each misreading from the right reading
MUTATION_FAMILY = {"last_max": "tie", "lane_last": "tie", "split_lt": "eps", "clean_lt": "eps", "no_axis": "eps", "no_sip": "eps", "reject7": "vertices", "side_ge": "integer",
                   "near_le": "integer", "tie_j": (15, 1), "removed_stop": (9, 3)}


def test_mutation_table_is_complete():
    assert sorted(MUTATION_FAMILY) == sorted(Q.MUTATIONS)


@pytest.mark.parametrize("mut", sorted(MUTATION_FAMILY))
def test_cases_tell_a_misreading_from_the_reference(mut):
    fam = MUTATION_FAMILY[mut]
    if isinstance(fam, tuple):
        g = Q.multi_frame()
        assert not np.array_equal(Q.multi_candidates(g, *fam, mut=(mut,)), Q.multi_candidates(g, *fam)), mut
        return
    differs = [i for i, (s, _) in enumerate(Q.family(fam)[1]) if not np.array_equal(Q.sheet_candidates(s, mut=(mut,)), Q.sheet_candidates(s))]
    assert differs, mut
