"""Plain float64 reference for the LINES corner refinement at its edges (numpy): MarkerDetector::refineCandidateLines restated from the
reference's text (src/markerdetector.cpp:83-153, 931-997), and the case families both edge test files run. The line fit goes through
np.linalg.lstsq on the uncentred [u 1] system (SVD based, minimum norm, like cv::solve(DECOMP_SVD)): deliberately another route than
the centred normal equations the device and the oracle share. The size_t arithmetic of the walk (:967) is modelled with Python integers.
Used by test_lines_edges_cpu.py, which pins the oracle on the families and measures the fine bound, and by test_gpu_lines_edges.py,
which holds the device to the same cases. The lens model is planar_ref's (undistort with five iterations, brown_project)."""
import numpy as np

from tests.planar_ref import brown_project, undistort

REL_TOL = 1e-4            # the project's corner tolerance, relative to the largest coordinate of the case

# The fine bound, in float32 spacings of each corner coordinate (np.spacing(np.float32(abs(v)))) around the f32lines result.
# Measured with   pytest -s -m "not gpu" tests/test_lines_edges_cpu.py -k measured   which prints the oracle's worst deviation per
# family: the worst over all 854 non-hostile cases is ORACLE_WORST_SPACINGS = 0.0 (the oracle equals f32lines bit for bit in every family), and the bound is four times that, never below 4: the
# margin is for the device summing 64 lanes as a tree where the oracle sums in order, which changes the last bits of the double sums
# and can only surface through a float32 rounding boundary of a line coefficient, about one spacing per line, amplified by at
# most 1 / sin 30 degrees = 2. Measured against the oracle and this reference only, never against the device.
ORACLE_WORST_SPACINGS = 0.0
FINE_BOUND_SPACINGS = max(4.0 * ORACLE_WORST_SPACINGS, 4.0)

K_MAIN = np.array([[1400.0, 0.0, 960.0], [0.0, 1400.0, 540.0], [0.0, 0.0, 1.0]])   # the matrix suite's camera (tests/test_gpu_matrix.py)
DIST_MAIN = (-0.10, 0.02, 1e-3, -5e-4, 0.0)
DIST_STRONG = (-0.30, 0.12, 2e-3, -1e-3, -0.02)
DIST_ZERO = (0.0, 0.0, 0.0, 0.0, 0.0)
WRAP = 2 ** 64


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------------
def _fit(pts, ge=False):
    """interpolate2Dline :83-130: (a, b, c) of a x + b y + c = 0 through the points, float64."""
    sx, sy = np.ptp(pts[:, 0]), np.ptp(pts[:, 1])
    yx = sx >= sy if ge else sx > sy
    u, v = (pts[:, 0], pts[:, 1]) if yx else (pts[:, 1], pts[:, 0])
    sol = np.linalg.lstsq(np.stack([u, np.ones(len(u))], axis=1), v, rcond=None)[0]
    return np.array([sol[0], -1.0, sol[1]]) if yx else np.array([-1.0, sol[0], sol[1]])


def _cross(l1, l2):
    """getCrossPoint :132-139."""
    return np.linalg.lstsq(np.array([l1[:2], l2[:2]]), -np.array([l1[2], l2[2]]), rcond=None)[0]


def _min_angle(lines):
    best = 90.0
    for i in range(4):
        a, b = lines[i][:2], lines[(i + 3) % 4][:2]
        c = abs(a @ b) / (np.linalg.norm(a) * np.linalg.norm(b))
        best = min(best, float(np.degrees(np.arccos(min(c, 1.0)))))
    return best


def corner_indices(contour, corners, first=False):
    """:934-941: the contour index of each corner's pixel (cvRound, ties to even), the last match; None for an absent corner (the reference
    reads an uninitialised index there)."""
    q = np.rint(np.asarray(corners, np.float32).reshape(4, 2)).astype(np.int64)
    out = []
    for k in range(4):
        hit = np.nonzero((contour[:, 0] == q[k, 0]) & (contour[:, 1] == q[k, 1]))[0]
        out.append(None if len(hit) == 0 else int(hit[0] if first else hit[-1]))
    return out


def is_inverse(ci):
    """:944-951 as written."""
    if (ci[1] > ci[0]) and (ci[2] > ci[1] or ci[2] < ci[0]):
        return False
    if ci[2] > ci[1] and ci[2] < ci[0]:
        return False
    return True


def walk_sides(ci, n, inverse, wrong=None):
    """:961-977: the contour indices of each side, or None where the walk does not reach its end corner within 2 n steps (the reference
    itself would not terminate). wrong: "wrap" steps to n - 1 below 0 instead of the size_t modulo, "nonext" adds no next corner."""
    inc = -1 if inverse else 1
    sides = []
    for l in range(4):
        j, end, idx = ci[l], ci[(l + 1) % 4], []
        while j != end:
            if len(idx) > 2 * n:
                return None
            idx.append(j)
            j = (j + inc) % n if wrong == "wrap" else ((j + inc) % WRAP) % n
        if len(idx) == 1 and wrong != "nonext":
            idx.append(end)
        sides.append(idx)
    return sides


def refine(contour, corners, K=None, dist=None, wrong=None):
    """refineCandidateLines on an n x 2 integer contour and 4 x 2 corners. Returns a dict:
    hostile    None, or why the reference has no defined result (absent corner, empty side, endless walk, singular crossing)
    terminates False where the inverse walk never reaches its end corner
    exact      [4,2] everything in float64
    f32lines   [4,2] the storage formats of the reference around float64 arithmetic: the undistorted contour rounded to float32 (Point2f;
               integer points are exact), each line's three coefficients rounded to float32 (Point3f), the crossing solved in float64 and
               rounded to float32 (Point2f); with a lens the normalisation of distortPoints in float32 as written (:149-150), the
               projection in float64, the result rounded to float32
    angle      the smallest angle between adjacent fitted lines, degrees (exact lines)
    inverse, sides (the contour indices of each side)
    wrong: one of the deliberately wrong variants "first", "wrap", "nonext", "ge", "dropend" (the discrimination checks)."""
    contour = np.asarray(contour, np.int64).reshape(-1, 2)
    n = len(contour)
    res = {"hostile": None, "terminates": True}
    ci = corner_indices(contour, corners, first=(wrong == "first"))
    if any(c is None for c in ci):
        res["hostile"] = "corner absent from the contour"
        return res
    inverse = is_inverse(ci)
    sides = walk_sides(ci, n, inverse, wrong)
    res["inverse"], res["cidx"] = inverse, ci
    if sides is None:
        res["hostile"], res["terminates"] = "the walk does not terminate", False
        return res
    if any(len(s) == 0 for s in sides):
        res["hostile"] = "a side without points (two corners on one contour point)"
        return res
    if wrong == "dropend" and len(sides[0]) > 2:
        sides[0] = sides[0][:-1]
    res["sides"] = sides
    lens = K is not None and dist is not None and len(dist) > 0
    pts = contour.astype(np.float64)
    if lens:
        K = np.asarray(K, np.float32).astype(np.float64).reshape(3, 3)      # camMatrix and distCoeff are float matrices
        dist = np.asarray(dist, np.float32).astype(np.float64)
        un = undistort(pts, K, dist)                                        # :959, P = camMatrix
        h = np.concatenate([un, np.ones((n, 1))], axis=1) @ K.T
        pts = h[:, :2] / h[:, 2:3]
    lines = [_fit(pts[s], ge=(wrong == "ge")) for s in sides]
    if _min_angle(lines) < 1e-6:
        res["hostile"] = "adjacent sides on one line: the crossing is singular"
        return res
    # f32lines fits what the reference's containers hold: the undistorted contour is a vector<Point2f> (:957-959), each line a Point3f
    pts32 = pts.astype(np.float32).astype(np.float64)
    lines32 = [_fit(pts32[s], ge=(wrong == "ge")).astype(np.float32).astype(np.float64) for s in sides]
    exact = np.array([_cross(lines[i], lines[(i + 3) % 4]) for i in range(4)])
    f32 = np.array([_cross(lines32[i], lines32[(i + 3) % 4]) for i in range(4)]).astype(np.float32)
    if lens:
        eye, zero = np.eye(3), np.zeros(3)
        nrm = np.stack([(exact[:, 0] - K[0, 2]) / K[0, 0], (exact[:, 1] - K[1, 2]) / K[1, 1], np.ones(4)], axis=1)
        exact = brown_project(nrm, eye, zero, K, dist)
        K32 = K.astype(np.float32)
        nrm32 = np.stack([(f32[:, 0] - K32[0, 2]) / K32[0, 0], (f32[:, 1] - K32[1, 2]) / K32[1, 1], np.ones(4, np.float32)], axis=1)
        assert nrm32.dtype == np.float32
        f32 = brown_project(nrm32.astype(np.float64), eye, zero, K, dist).astype(np.float32)
    res["exact"], res["f32lines"], res["angle"] = exact, f32.astype(np.float64), _min_angle(lines)
    return res


def spacings(got, f32lines):
    """Deviation of each corner coordinate from f32lines in float32 spacings of that coordinate, [4,2]."""
    f = np.asarray(f32lines, np.float64)
    return np.abs(np.asarray(got, np.float64) - f) / np.spacing(np.abs(f).astype(np.float32)).astype(np.float64)


def rel_dev(got, exact):
    return float(np.max(np.abs(np.asarray(got, np.float64) - exact)) / np.max(np.abs(exact)))


# ---------------------------------------------------------------------------------------------------------------------------------
# contours
# ---------------------------------------------------------------------------------------------------------------------------------
def digital_quad(vertices):
    """A closed point list through four integer vertices, max(|dx|, |dy|) points per side (the end vertex belongs to the next side),
    and the four vertices as corners."""
    v = np.asarray(vertices, np.int64)
    pts = []
    for i in range(4):
        a, b = v[i], v[(i + 1) % 4]
        L = int(np.max(np.abs(b - a)))
        for t in range(L):
            pts.append(a + np.rint((b - a) * (t / L)).astype(np.int64))
    return np.array(pts), v.astype(np.float32)


def rectangle(w, h, x0=40, y0=30):
    """Border of an axis-aligned w x h pixel rectangle, 2 (w + h) - 4 points, clockwise in image coordinates from the top left corner."""
    return digital_quad([(x0, y0), (x0 + w - 1, y0), (x0 + w - 1, y0 + h - 1), (x0, y0 + h - 1)])


def rectangle_of(n):
    """A rectangle border of exactly n points. An odd n has no rectangle: the border of n + 1 points without one point from the middle
    of its third side (the stage takes any point list)."""
    m = n + (n & 1)
    s = (m + 4) // 2
    w = (s * 7) // 13
    c, q = rectangle(w, s - w)
    assert len(c) == m
    if n & 1:
        c = np.delete(c, (w - 1) + (s - w - 1) + (w - 1) // 2, axis=0)
    return c, q


def slanted_quad(n, x0=60, y0=40):
    """A convex quad of exactly n points with no side parallel to an axis (every side's points are jagged, so leaving points out of a
    side moves its line)."""
    e3 = 2 if n & 1 else 3
    s = (n + 9 + e3) // 2          # a + b
    a = (s * 4) // 7
    b = s - a
    c, q = digital_quad([(x0, y0), (x0 + a, y0 + 3), (x0 + a - 4, y0 + b), (x0 + e3, y0 + b - 2)])
    assert len(c) == n, (len(c), n)
    return c, q


def raster_quad(vertices):
    """A filled convex quad drawn into a small binary image; the outer border in the order orc.find_contours walks it, the corners are the
    contour points nearest the true vertices."""
    from oracle import orc

    v = np.asarray(vertices, np.float64)
    w, h = int(np.ceil(v[:, 0].max())) + 4, int(np.ceil(v[:, 1].max())) + 4
    ys, xs = np.mgrid[0:h, 0:w]
    m = np.ones((h, w), bool)
    ctr = v.mean(axis=0)
    for i in range(4):
        a, b = v[i], v[(i + 1) % 4]
        cr = (b[0] - a[0]) * (ys - a[1]) - (b[1] - a[1]) * (xs - a[0])
        m &= (cr >= 0) if (b[0] - a[0]) * (ctr[1] - a[1]) - (b[1] - a[1]) * (ctr[0] - a[0]) > 0 else (cr <= 0)
    cs = [c for c in orc.find_contours(m.astype(np.uint8) * 255) if not c["hole"]]
    c = max(cs, key=lambda c: len(c["pts"]))["pts"].astype(np.int64)
    idx = [int(np.argmin(np.sum((c - p) ** 2, axis=1))) for p in v]
    return c, c[idx].astype(np.float32)


ANGLES = [base + d for base in (0, 45, 90, 135) for d in (-1, 0, 1)]
SIZES = [10, 400, 14, 64, 150, 23, 260, 33, 97, 12, 200, 40]     # side lengths in pixels, by angle; the diagonals get no side under 8 points
PERSPECTIVE = np.array([[0.03, -0.02], [-0.04, 0.03], [0.02, 0.05], [-0.03, -0.04]])


def _raster_vertices(angle, size, perspective):
    base = np.array([[-0.5, -0.5], [0.5, -0.5], [0.5, 0.5], [-0.5, 0.5]])
    if perspective:
        base = base + PERSPECTIVE
    a = np.radians(angle)
    R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    if angle % 45 == 0:   # exact rotations: no rounding of cos / sin
        r2 = np.sqrt(0.5)
        R = {0: [[1, 0], [0, 1]], 45: [[r2, -r2], [r2, r2]], 90: [[0, -1], [1, 0]], 135: [[-r2, -r2], [r2, -r2]]}[angle]
        R = np.array(R, np.float64)
    v = (base * size) @ R.T
    return v - v.min(axis=0) + 6.0


def _nudge(corners):
    """Corners a fraction off their pixel, so the search has to round: half a pixel (a tie, to even) off an even coordinate, a quarter
    off an odd one, alternating in sign."""
    c = np.asarray(corners, np.float64).copy().reshape(-1)
    for i in range(len(c)):
        sg = 1.0 if i % 2 == 0 else -1.0
        c[i] += sg * (0.5 if int(c[i]) % 2 == 0 else 0.25)
    return c.reshape(4, 2).astype(np.float32)


def case(family, name, contour, corners, K=None, dist=None):
    return {"family": family, "name": name, "contour": np.ascontiguousarray(contour, np.int32), "corners": np.ascontiguousarray(corners, np.float32),
            "K": K, "dist": dist}


def _side_bounds(r):
    return min(len(s) for s in r["sides"]), r["angle"]


def _check_formed(c, r, min_pts=8, min_angle=30.0):
    assert r["hostile"] is None, (c["name"], r["hostile"])
    pts, ang = _side_bounds(r)
    assert pts >= min_pts and ang >= min_angle, (c["name"], pts, ang)


_cache = {}


def _raster_size(i, persp):
    size = SIZES[(i + 5 * persp) % 12]
    return 64 if ANGLES[i] % 90 in (44, 45, 46) and size < 14 else size      # a diagonal side of 10 px has 7 points


def _rasters():
    if "raster" not in _cache:
        out = []
        for i, ang in enumerate(ANGLES):
            for persp in (False, True):
                size = _raster_size(i, persp)
                c, q = raster_quad(_raster_vertices(ang, size, persp))
                if is_inverse(corner_indices(c, q)):            # corners in the border's own direction: the forward walk
                    q = q[[0, 3, 2, 1]]
                out.append(case("raster", "a%d_s%d_p%d" % (ang, size, persp), c, _nudge(q)))
        _cache["raster"] = out
    return _cache["raster"]


def _rolled(c, shift):
    return np.roll(c, -shift, axis=0)


def skipped_by_wrap(n):
    """The points a backward walk through index 0 leaves out: it steps to (2^64 - 1) % n, not to n - 1."""
    return n - 1 - (WRAP - 1) % n


def _inverse_roll(contour, corners):
    """The reversed contour, rolled so that the backward walk terminates where it can. The walk steps from index 0 to (2^64 - 1) % n, so
    the side that passes through index 0 ends only if its end corner, the largest corner index, lies at or below that: the `skip` points
    above it have to fit between two corners. The roll puts them in the middle of the longest side. None where that side would keep
    fewer than 8 points."""
    c = contour[::-1].copy()
    n = len(c)
    skip = skipped_by_wrap(n)
    order = sorted(corner_indices(c, corners))
    gaps = [(order[(k + 1) % 4] - order[k]) % n for k in range(4)]      # the points of the side walked (backwards) from order[k + 1] to order[k]
    k = int(np.argmax(gaps))
    if gaps[k] - skip < 8:
        return None
    top = order[k]                       # that side's end corner becomes the largest index: skip + half of what is left of the side below n - 1
    return _rolled(c, (top - (n - 1 - skip - (gaps[k] - skip) // 2)) % n)


def _reversible_raster(angle, size, perspective):
    """The raster quad of this angle whose side is `size` px or the least above it, in steps of a quarter pixel, at which the reversed
    border can be walked backwards: a power of two of points, or the wrap's skipped points inside one side. (For any other length the
    reference's walk never ends; those are `hostile`.) Returns (contour, corners, size)."""
    for step in range(400):
        s = size + 0.25 * step
        c, q = raster_quad(_raster_vertices(angle, s, perspective))
        q = _nudge(q[[0, 3, 2, 1]] if is_inverse(corner_indices(c, q)) else q)
        rc = _inverse_roll(c, q)
        if rc is not None:
            return rc, q, s
    raise AssertionError("no reversible raster at %d degrees from %g px" % (angle, size))


def families():
    """Every case, generated once per process: {family: [case, ...]}; `hostile` holds the inputs the reference has no defined result for."""
    if "all" in _cache:
        return _cache["all"]
    fam = {k: [] for k in ("raster", "start", "length", "inverse", "short", "duplicate", "tie", "far", "lens", "hostile")}
    rasters = _rasters()
    fam["raster"] = list(rasters)

    # start: index 0 on each corner, one after and one before it, and in the middle of each side
    for c in rasters:
        r = refine(c["contour"], c["corners"])
        n = len(c["contour"])
        ci = r["cidx"]
        order = sorted(ci)
        shifts = []
        for k in range(4):
            nxt = order[(k + 1) % 4]
            shifts += [order[k], (order[k] + 1) % n, (order[k] - 1) % n, (order[k] + ((nxt - order[k]) % n) // 2) % n]
        for s in shifts:
            fam["start"].append(case("start", "%s_r%d" % (c["name"], s), _rolled(c["contour"], s), c["corners"]))

    # length: contours of exactly 63 .. 513 points, and sides of 63 / 64 / 65 / 130 points in each position
    for n in (63, 64, 65, 127, 128, 129, 513):
        c, q = rectangle_of(n)
        assert len(c) == n
        fam["length"].append(case("length", "rect_n%d" % n, c, q))
    qv = np.array([(10, 10), (140, 10), (120, 74), (55, 73)])
    for k in range(4):
        c, q = digital_quad(np.roll(qv, -k, axis=0))
        r = refine(c, q)
        assert sorted(len(s) for s in r["sides"]) == [63, 64, 65, 130]
        fam["length"].append(case("length", "sides_63_64_65_130_from%d" % k, c, q))

    # inverse: reversed contours. A power of two wraps to n - 1; any other length wraps to (2^64 - 1) % n and skips the points above
    pow2 = other = skipping = 0
    for n in (64, 128, 256, 512):
        for base, nm in ((rectangle_of(n), "rect"), (slanted_quad(n), "slant")):
            c, q = base
            for s in (0, 1, n // 3):
                fam["inverse"].append(case("inverse", "%s_n%d_r%d" % (nm, n, s), _rolled(c[::-1], s), q))
                pow2 += 1
    cand_n = [n for n in range(90, 1400) if n & (n - 1) and 1 <= skipped_by_wrap(n) <= n // 24]
    for n in cand_n[:: max(1, len(cand_n) // 10)][:10]:
        c, q = slanted_quad(n)
        rc = _inverse_roll(c, q)
        assert rc is not None, n
        fam["inverse"].append(case("inverse", "slant_n%d_skip%d" % (n, skipped_by_wrap(n)), rc, q))
        other += 1
    # every raster angle, plain and in perspective, reversed: at the raster's own side length where that border can be walked backwards,
    # else at the least length above it that can (the reference's walk never ends on the others)
    for i, ang in enumerate(ANGLES):
        for persp in (False, True):
            rc, q, size = _reversible_raster(ang, _raster_size(i, persp), persp)
            fam["inverse"].append(case("inverse", "rev_a%d_s%g_p%d" % (ang, size, persp), rc, q))
            n = len(rc)
            pow2, other = pow2 + (n & (n - 1) == 0), other + (n & (n - 1) != 0)
    assert sum(c["name"].startswith("rev_") for c in fam["inverse"]) == 2 * len(ANGLES) == len(rasters)
    for c in fam["inverse"]:
        r = refine(c["contour"], c["corners"])
        assert r["hostile"] is None and r["inverse"], c["name"]
        n = len(c["contour"])
        walked = sum(len(s) for s in r["sides"])
        if n & (n - 1):
            assert walked == n - skipped_by_wrap(n), c["name"]
            skipping += walked < n
        else:
            assert walked == n, c["name"]
    assert pow2 >= 4 and other >= 4 and skipping >= 1

    # short: one side, then two opposite sides, of exactly one point; forwards and reversed (128 points: the backward walk terminates)
    shorts = {"one_flat": [(50, 10), (51, 10), (74, 50), (27, 50)], "one_diag": [(50, 10), (51, 11), (74, 50), (27, 51)],
              "two_flat": [(50, 10), (51, 10), (51, 73), (50, 73)], "two_slant": [(50, 10), (51, 11), (40, 74), (39, 73)]}
    for nm, v in shorts.items():
        c, q = digital_quad(v)
        assert len(c) == 128, (nm, len(c))
        for rev in (False, True):
            cc = c[::-1].copy() if rev else c
            for s in (0, 5):
                r = refine(_rolled(cc, s), q)
                assert r["hostile"] is None and r["inverse"] == rev and min(len(x) for x in r["sides"]) == 2
                if np.all(np.isfinite(r["exact"])) and r["angle"] > 1.0:
                    fam["short"].append(case("short", "%s_rev%d_r%d" % (nm, rev, s), _rolled(cc, s), q))
    assert len(fam["short"]) >= 8

    # duplicate: a corner's pixel a second time 3, 64 and n / 2 positions later (511 + 1 points: every walk terminates)
    kept = set()
    for base, nm in ((rectangle_of(511), "rect"), (slanted_quad(511), "slant")):
        c, q = base
        n = len(c)
        ci = corner_indices(c, q)
        for k in range(4):
            for off in (3, 64, n // 2):
                pos = (ci[k] + off) % n
                if pos <= ci[k]:
                    continue            # "later" in the contour's own order
                cc = np.insert(c, pos, c[ci[k]], axis=0)
                r, rf = refine(cc, q), refine(cc, q, wrong="first")
                if r["hostile"] or rf["hostile"] or not np.all(np.isfinite(r["exact"])):
                    continue
                # half a contour later the corner lies on the opposite side and two fitted sides run nearly parallel: no such case keeps
                # 30 degrees, so that offset is held to 0.25 degrees and 8 points (its crossings are ill conditioned by up to 1 / sin 0.25 = 230)
                if min(len(s) for s in r["sides"]) < 8 or r["angle"] < (0.25 if off == n // 2 else 30.0):
                    continue
                assert r["sides"] != rf["sides"]
                fam["duplicate"].append(case("duplicate", "%s_c%d_off%d" % (nm, k, off), cc, q))
                kept.add(off)
    assert kept == {3, 64, 511 // 2}, kept

    # tie: sides whose x span equals their y span exactly, or differs by one pixel either way; every third point a pixel off the diagonal, so
    # that regressing x on y and y on x give different lines
    diffs = set()
    shapes = {"tie": lambda L: [(10, 10 + L), (10 + L, 10), (10 + 2 * L, 10 + L), (10 + L, 10 + 2 * L)],
              "xwider": lambda L: [(10, 10 + L), (11 + L, 10), (11 + 2 * L, 10 + L), (10 + L, 11 + 2 * L)],
              "ywider": lambda L: [(10, 11 + L), (10 + L, 10), (10 + 2 * L, 11 + L), (10 + L, 11 + 2 * L)]}
    for nm, shape, L0 in (("tie", "tie", 32), ("xwider", "xwider", 40), ("ywider", "ywider", 40), ("tie_large", "tie", 128)):
        for L in range(L0, L0 + 200):       # the least half diagonal whose reversed contour can be walked backwards
            c, q = digital_quad(shapes[shape](L))
            for s in refine(c, q)["sides"]:
                for t in s[3:-3:3]:
                    c[t, 0] += 1 if (t // 3) % 2 else -1
            rc = _inverse_roll(c, q)
            if rc is not None:
                break
        assert rc is not None, nm
        for rev, cc in ((False, c), (True, rc)):
            r = refine(cc, q)
            assert r["hostile"] is None and r["inverse"] == rev, (nm, rev)
            for s in r["sides"]:
                p = cc[s]
                diffs.add(int(np.ptp(p[:, 0]) - np.ptp(p[:, 1])))
            fam["tie"].append(case("tie", "%s_L%d_rev%d" % (nm, L, rev), cc, q))
    assert len(fam["tie"]) == 8
    assert {0, 1, -1} <= diffs, diffs

    # far: raster quads near x, y = 3800, 8000 and 16300
    for off in (3800, 8000, 16300):
        for c in rasters[2::9]:
            fam["far"].append(case("far", "%s_at%d" % (c["name"], off), c["contour"] + off, c["corners"] + np.float32(off)))

    # lens: raster, start (one roll of each contour), inverse and far (up to 3800) under three camera settings
    pool = list(fam["raster"]) + fam["start"][5::16] + list(fam["inverse"]) + [c for c in fam["far"] if c["name"].endswith("at3800")]
    spots = [(8, 6), (1500, 8), (12, 880), (1480, 860)]      # near the corners of the camera's 1920 x 1080 image
    for i, c in enumerate(pool):
        ext = c["contour"].max(axis=0)
        for tag, d in (("main", DIST_MAIN), ("strong", DIST_STRONG), ("zero", DIST_ZERO)):
            cc, qq = c["contour"], c["corners"]
            if tag == "strong" and c["family"] == "far":
                continue                                   # the strong lens is for quads near the image corners: 3800 px is far outside its image
            if tag == "strong":
                sx, sy = spots[i % 4]
                sx, sy = min(sx, 1915 - int(ext[0])), min(sy, 1075 - int(ext[1]))
                sx, sy = sx - sx % 2, sy - sy % 2           # even: a corner half a pixel off an even coordinate stays a tie to even
                cc, qq = cc + np.array([sx, sy], np.int32), qq + np.array([sx, sy], np.float32)
            fam["lens"].append(case("lens", "%s_%s_%s" % (c["family"], c["name"], tag), cc, qq, K=K_MAIN, dist=d))

    # hostile: inputs for which the reference has no defined result
    c, q = rectangle_of(128)
    absent = q.copy()
    absent[2] += 2.0                                       # two pixels inside the rectangle: not a contour point
    fam["hostile"].append(case("hostile", "corner_absent", c, absent))
    same = q.copy()
    same[1] = same[0]
    fam["hostile"].append(case("hostile", "two_corners_one_point", c, same))
    for n in (1, 2, 3):
        fam["hostile"].append(case("hostile", "contour_of_%d" % n, c[:n], np.array([c[i % n] for i in range(4)], np.float32)))
    c, q = rectangle_of(100)                               # (2^64 - 1) % 100 = 15: the wrapped side never comes back to its end corner
    fam["hostile"].append(case("hostile", "endless_walk_n100", c[::-1].copy(), q))
    c, q = slanted_quad(1999)
    fam["hostile"].append(case("hostile", "endless_walk_n1999", c[::-1].copy(), q))
    for c in fam["hostile"]:
        r = refine(c["contour"], c["corners"])
        assert r["hostile"] is not None, c["name"]
        assert r["terminates"] == (not c["name"].startswith("endless")), c["name"]

    for name, cases in fam.items():
        if name in ("hostile", "short"):
            continue
        for c in cases:
            if name == "duplicate" and c["name"].endswith("off%d" % (511 // 2)):
                continue
            _check_formed(c, refine(c["contour"], c["corners"], c["K"], c["dist"]))
    _cache["all"] = fam
    return fam


def non_hostile():
    return [c for name, cases in families().items() if name != "hostile" for c in cases]


def reference(c):
    """refine() of a case, computed once per process and left unchanged."""
    key = ("ref", c["family"], c["name"])
    if key not in _cache:
        _cache[key] = refine(c["contour"], c["corners"], c["K"], c["dist"])
    return _cache[key]
