"""Plain reference of the contour-to-candidate stage and the generator of its edge cases (CPU only).

The reference restates what MarkerDetector::detectRectangles does with a frame's borders once cv::findContours has delivered them: the size
filter, cv::approxPolyDP(closed, eps = 0.05 n), the 4-vertex / convexity / minimum-side tests, the orientation swap and the near-duplicate
removal. It runs on Python integers and floats (a Python float is the C double), one point at a time in the scan order of the sequential algorithm,
so nothing vectorised can hide an order. It is a second reading, independent of oracle/orc_imgproc.cpp and of the device code, and it is
instrumented: a Trace per border says how many vertices the recursion left, how deep its bookkeeping went, which scans had their maximum more than once,
which `<=` held with equality and what every clause of the clean-up pass said about every vertex.

`mut` names deliberate misreadings (MUTATIONS); tests/test_quad_edges_cpu.py shows that the cases tell every one of them from the right reading.

The generator draws binary tiles with numpy (convex polygons by half-plane tests, unions, notches), each with its own quiet zone, and packs them into
sheets of 640 x 480. Borders come from the oracle's find_contours: border following is pinned by tests/border_ref.py
(tests/test_border_edges_cpu.py, tests/test_gpu_border_edges.py).
"""
import math
import struct

import numpy as np

MUTATIONS = ("last_max", "lane_last", "split_lt", "clean_lt", "no_axis", "no_sip", "reject7", "side_ge", "near_le", "tie_j", "removed_stop")

SHEET_W, SHEET_H = 640, 480
MIN_SIZE, MAX_SIZE = 0.01, 0.5   # of every 640 x 480 sheet: borders of 26 .. 1279 points pass


def f32(x):
    """a double rounded to float32 (and back)"""
    return struct.unpack("f", struct.pack("f", x))[0]


def size_limits(width, height, min_size, max_size):
    """minSize, maxSize of detectRectangles: float32 products truncated to int"""
    side = np.float32(max(width, height))
    return int(np.float32(min_size) * side * np.float32(4)), int(np.float32(max_size) * side * np.float32(4))


class Trace:
    def __init__(self):
        self.n = 0
        self.raw = 0          # vertices before the clean-up pass
        self.depth = 0        # deepest (vertices out) + (ranges waiting)
        self.ties = 0         # scans whose non-zero maximum was attained more than once
        self.tie_gaps = []    # per such scan: scan positions between the first and the last occurrence
        self.eq_far = 0       # `max distance <= eps^2` of the three farthest-point passes held with equality
        self.eq_split = 0     # `maxd^2 <= eps^2 |chord|^2` held with equality
        self.eq_clean = 0     # `dist^2 <= 0.5 eps^2 |chord|^2` held with equality
        self.zero_chord = 0   # ranges whose two ends are the same pixel
        self.clean = []       # per vertex looked at: (near, oblique, forward, removed)
        self.poly = []


def _first_max(values, last, tr, lanes=0):
    """values: (position, non-negative int) in scan order -> (maximum, position of its first occurrence or None if it is 0).
    lanes: the misreading of a scan dealt out to `lanes` lanes in turns, each of which keeps the last of its own equal maxima, the first lane's winning"""
    best, at, hits, tied = 0, None, 0, []
    for i, (k, v) in enumerate(values):
        if v > best:
            best, at, hits, tied = v, k, 1, [(i, k)]
        elif v == best and v > 0:
            hits += 1
            tied.append((i, k))
            if last:
                at = k
    if hits > 1:
        tr.ties += 1
        tr.tie_gaps.append(tied[-1][0] - tied[0][0])
        if lanes:
            kept = {}
            for i, k in tied:
                kept[i % lanes] = (i, k)
            at = min(kept.values())[1]
    return best, at


def approx_poly(pts, eps, tr=None, mut=()):
    """cv::approxPolyDP(pts, eps, closed=true) on a list of (x, y) integer pairs -> list of vertices"""
    tr = tr if tr is not None else Trace()
    n = tr.n = len(pts)
    if n == 0:
        return []
    last = "last_max" in mut
    lanes = 32 if "lane_last" in mut else 0
    e2 = float(eps) * float(eps)

    # three passes "farthest point from where I stand, go there": the last two places are the ends of the first two ranges
    here, hop, flat = 0, 0, False
    for _ in range(3):
        here = (here + hop) % n
        ax, ay = pts[here]
        far, at = _first_max(((j, (pts[(here + j) % n][0] - ax) ** 2 + (pts[(here + j) % n][1] - ay) ** 2) for j in range(1, n)), last, tr, lanes)
        if at is not None:
            hop = at
        flat = float(far) <= e2
        tr.eq_far += float(far) == e2

    out, todo = [], []
    if flat:
        out.append(pts[here])
    else:
        there = (here + hop) % n
        todo = [(there, here), (here, there)]   # the top of the stack is taken first
    while todo:
        tr.depth = max(tr.depth, len(out) + len(todo))
        if "reject7" in mut and len(out) + len(todo) > 7:
            return []
        s, e = todo.pop()
        (sx, sy), (ex, ey) = pts[s], pts[e]
        k = (s + 1) % n
        if k == e:
            out.append(pts[s])
            continue
        dx, dy = ex - sx, ey - sy
        tr.zero_chord += dx == 0 and dy == 0
        inner = []
        while k != e:
            inner.append((k, abs((pts[k][1] - sy) * dx - (pts[k][0] - sx) * dy)))
            k = (k + 1) % n
        far, at = _first_max(inner, last, tr, lanes)
        lhs, rhs = float(far) * float(far), e2 * (float(dx) * float(dx) + float(dy) * float(dy))
        tr.eq_split += lhs == rhs and far > 0
        if (lhs < rhs) if "split_lt" in mut else (lhs <= rhs):
            out.append(pts[s])
        else:
            if at is None:
                at = (s + 1) % n
            todo.append((at, e))
            todo.append((s, at))
    tr.raw = len(out)

    # clean-up: one walk round the polygon in place; a vertex near the chord of its neighbours goes, unless the chord is axis-aligned or the
    # vertex lies behind one of the chord's ends
    cnt = left = len(out)
    ring = list(out)
    rd = cnt - 1

    def take():
        nonlocal rd
        p = ring[rd]
        rd = rd + 1 if rd + 1 < cnt else 0
        return p

    a = take()
    wr = rd
    b = take()
    i = 0
    while i < cnt and left > 2:
        c = take()
        dx, dy = c[0] - a[0], c[1] - a[1]
        d = float(abs((b[0] - a[0]) * dy - (b[1] - a[1]) * dx))
        lhs, rhs = d * d, 0.5 * e2 * (float(dx) * float(dx) + float(dy) * float(dy))
        near = (lhs < rhs) if "clean_lt" in mut else (lhs <= rhs)
        oblique = dx != 0 and dy != 0
        forward = (b[0] - a[0]) * (c[0] - b[0]) + (b[1] - a[1]) * (c[1] - b[1]) >= 0
        drop = near and (oblique or "no_axis" in mut) and (forward or "no_sip" in mut)
        tr.eq_clean += lhs == rhs
        tr.clean.append((near, oblique, forward, drop))
        if drop:
            left -= 1
            ring[wr] = a = c
            wr = wr + 1 if wr + 1 < cnt else 0
            b = take()
            i += 2
        else:
            ring[wr] = a = b
            wr = wr + 1 if wr + 1 < cnt else 0
            b = c
            i += 1
    tr.poly = ring[:left]
    return tr.poly


def is_convex(poly):
    """cv::isContourConvex on integer vertices: every turn has the same strict sense"""
    n = len(poly)
    if n < 3:
        return False
    senses = set()
    for i in range(n):
        p, q, r = poly[i - 2], poly[i - 1], poly[i]
        turn = (r[1] - q[1]) * (q[0] - p[0]) - (r[0] - q[0]) * (q[1] - p[1])
        if turn == 0:
            return False
        senses.add(turn > 0)
        if len(senses) > 1:
            return False
    return True


def min_side(poly):
    """the float the call site compares with 10: the shortest side's length, a double norm stored in a float"""
    return min(f32(math.sqrt(float((poly[j][0] - poly[(j + 1) % 4][0]) ** 2 + (poly[j][1] - poly[(j + 1) % 4][1]) ** 2))) for j in range(4))


def perimeter(q):
    """utils.h perimeter(): double norms added into a float"""
    s = 0.0
    for i in range(4):
        j = (i + 1) % 4
        s = f32(s + math.sqrt(float(q[i][0] - q[j][0]) ** 2 + float(q[i][1] - q[j][1]) ** 2))
    return s


def border_quad(pts, tr=None, mut=()):
    """one kept border -> its quad (4 integer vertices in approxPolyDP's order) or None"""
    poly = approx_poly(pts, float(len(pts)) * 0.05, tr, mut)
    if len(poly) != 4 or not is_convex(poly):
        return None
    m = min_side(poly)
    if (m < 10) if "side_ge" in mut else (m <= 10):
        return None
    return [tuple(p) for p in poly]


def thin_out(quads, mut=()):
    """orientation swap and near-duplicate removal over the joined list -> candidates"""
    qs = []
    for q in quads:
        q = list(q)
        d1x, d1y, d2x, d2y = q[1][0] - q[0][0], q[1][1] - q[0][1], q[2][0] - q[0][0], q[2][1] - q[0][1]
        if f32(f32(float(d1x) * float(d2y)) - f32(float(d1y) * float(d2x))) < 0.0:
            q[1], q[3] = q[3], q[1]
        qs.append(q)
    gone = [False] * len(qs)
    for i in range(len(qs)):
        for j in range(i + 1, len(qs)):
            if "removed_stop" in mut and (gone[i] or gone[j]):
                continue
            ds = [f32(math.sqrt(float(qs[i][c][0] - qs[j][c][0]) ** 2 + float(qs[i][c][1] - qs[j][c][1]) ** 2)) for c in range(4)]
            if not all((d <= 6) if "near_le" in mut else (d < 6) for d in ds):
                continue
            pi, pj = perimeter(qs[i]), perimeter(qs[j])
            if (pi >= pj) if "tie_j" in mut else (pi > pj):
                gone[j] = True
            else:
                gone[i] = True
    return [q for q, g in zip(qs, gone) if not g]


def detect_rectangles(planes, width, height, min_size, max_size, mut=(), traces=None):
    """planes: per threshold plane, the borders (lists of (x, y)) in RETR_LIST order -> candidate list of 4 (x, y) integer pairs each"""
    lo, hi = size_limits(width, height, min_size, max_size)
    quads = []
    for borders in planes:
        for pts in borders:
            if not lo < len(pts) < hi:
                continue
            tr = Trace()
            q = border_quad(pts, tr, mut)
            if traces is not None:
                traces.append((tr, q))
            if q is not None:
                quads.append(q)
    return thin_out(quads, mut)


# ------------------------------------------------------------------------------------------------------------------------------------
# drawing
# ------------------------------------------------------------------------------------------------------------------------------------
def fill_convex(mask, poly, value=1):
    """pixels whose centre lies inside or on the edge of the convex polygon (either sense)"""
    h, w = mask.shape
    ys, xs = np.mgrid[0:h, 0:w]
    area = sum(poly[i - 1][0] * poly[i][1] - poly[i][0] * poly[i - 1][1] for i in range(len(poly)))
    sgn = 1.0 if area >= 0 else -1.0
    inside = np.ones((h, w), bool)
    for i in range(len(poly)):
        (x0, y0), (x1, y1) = poly[i - 1], poly[i]
        inside &= sgn * ((x1 - x0) * (ys - y0) - (y1 - y0) * (xs - x0)) >= -1e-9
    mask[inside] = value


def rot(poly, deg, about=(0.0, 0.0)):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return [(about[0] + c * (x - about[0]) - s * (y - about[1]), about[1] + s * (x - about[0]) + c * (y - about[1])) for x, y in poly]


def rect(x0, y0, w, h):
    """the pixels x0 .. x0 + w - 1, y0 .. y0 + h - 1"""
    return [(x0, y0), (x0 + w - 1, y0), (x0 + w - 1, y0 + h - 1), (x0, y0 + h - 1)]


QUIET = 3


def tile(add, sub=()):
    """union of the convex polygons `add` minus those of `sub`, cropped to its bounding box plus a quiet zone -> uint8 0/1"""
    xs = [x for p in add for x, _ in p]
    ys = [y for p in add for _, y in p]
    ox, oy = math.floor(min(xs)) - QUIET, math.floor(min(ys)) - QUIET
    w, h = math.ceil(max(xs)) - ox + 1 + QUIET, math.ceil(max(ys)) - oy + 1 + QUIET
    m = np.zeros((h, w), np.uint8)
    for p in add:
        fill_convex(m, [(x - ox, y - oy) for x, y in p], 1)
    for p in sub:
        fill_convex(m, [(x - ox, y - oy) for x, y in p], 0)
    m[:QUIET] = m[-QUIET:] = 0
    m[:, :QUIET] = m[:, -QUIET:] = 0
    return m


def pack(tiles, width=SHEET_W, height=SHEET_H):
    """shelf packing in the given order -> list of (sheet uint8 0/255, [(x, y) of every tile])"""
    sheets, places = [], []
    x = y = 1
    shelf = 0
    cur, where = np.zeros((height, width), np.uint8), []
    for t in tiles:
        th, tw = t.shape
        assert tw <= width - 2 and th <= height - 2, (tw, th)
        if x + tw > width - 1:
            x, y, shelf = 1, y + shelf, 0
        if y + th > height - 1:
            sheets.append(cur), places.append(where)
            cur, where = np.zeros((height, width), np.uint8), []
            x, y, shelf = 1, 1, 0
        cur[y:y + th, x:x + tw] = t * 255
        where.append((x, y))
        x, shelf = x + tw, max(shelf, th)
    sheets.append(cur), places.append(where)
    return list(zip(sheets, places))


def borders_of(binimg):
    """the oracle's border following -> list of lists of (x, y) Python ints, RETR_LIST order"""
    from oracle import orc
    return [[(int(x), int(y)) for x, y in c["pts"]] for c in orc.find_contours(binimg)]


def outer_border(t):
    """the longest border of a tile"""
    return max(borders_of(t * 255), key=len)


# ------------------------------------------------------------------------------------------------------------------------------------
# cases: (name, tile). Every family's precondition is asserted per case by tests/test_quad_edges_cpu.py with the Trace.
# ------------------------------------------------------------------------------------------------------------------------------------
def quad_of_count(n, deg=0.0):
    """a filled rectangle, turned by `deg`, whose outer border has exactly n points: sizes are searched, the count is asserted"""
    if n % 2 == 0 and deg == 0.0:
        h = max(3, min(100, (n + 4) // 8))
        t = tile([rect(0, 0, (n + 4) // 2 - h, h)])
        assert len(outer_border(t)) == n
        return t
    h = max(6.0, min(90.0, n / 8.0))
    w0 = n / 2.0 / max(math.cos(math.radians(deg)), 0.5) - h
    for dh in (0.0, 0.37, 0.71, 1.13, 1.6):
        for k in range(-160, 160):
            w = w0 + 0.25 * k
            if w < 4:
                continue
            t = tile([rot([(0, 0), (w, 0), (w, h + dh), (0, h + dh)], deg)])
            if len(outer_border(t)) == n:
                return t
    raise AssertionError("no turned rectangle with a border of %d points at %g degrees" % (n, deg))


def length_cases():
    lo, hi = size_limits(SHEET_W, SHEET_H, MIN_SIZE, MAX_SIZE)
    out = []
    for n, deg in ((511, 9.0), (512, 0.0), (512, 14.0), (513, 21.0), (961, 6.0), (1023, 4.0), (1024, 0.0), (1024, 8.0), (1025, 5.0),
                   (lo + 1, 0.0), (hi - 1, 7.0)):
        out.append(("n%d_deg%g" % (n, deg), quad_of_count(n, deg)))
    return out


def stride_cases():
    out = []
    for base in (448, 576):
        for r in (0, 1, 31, 32, 33, 63):
            n = base + r + 1 - (64 if r == 63 else 0)   # count - 1 = r (mod 64)
            out.append(("n%d" % n, quad_of_count(n, 0.0 if n % 2 == 0 else 11.0)))
    return out


def pairing_cases(odd):
    """short and long borders in turns; a 40-point border beside a 512-point one"""
    out = [("n40", quad_of_count(40)), ("n512", quad_of_count(512)), ("n40b", tile([rect(0, 0, 9, 13)]))]
    for i in range(37 + (1 if odd else 0)):
        if i % 2 == 0:
            out.append(("short%d" % i, tile([rot(rect(0, 0, 13 + i % 5, 12 + i % 3), 3.0 * (i % 7))])))
        else:
            out.append(("long%d" % i, tile([rot(rect(0, 0, 70 + 3 * (i % 9), 22 + i % 4), 5.0 * (i % 5))])))
    return out


def blunt(a, b_top, b_bot, tip):
    """a diamond (b_top == b_bot) or kite, taller than wide, with sharp top and bottom and side tips `tip` pixels high: the first ranges' chord is the
    vertical axis, and every pixel of a side tip is equally far from it"""
    return [(0, -b_top), (a, 0), (a, tip - 1), (0, b_bot + tip - 1), (-a, tip - 1), (-a, 0)]


def tie_cases():
    out = []
    for tip in (2, 3):
        for a, b in ((30, 41), (25, 40), (26, 37)):
            out.append(("diamond_tip%d_%dx%d" % (tip, a, b), tile([blunt(a, b, b, tip)])))
        for a, b1, b2 in ((30, 31, 45), (24, 30, 50), (35, 48, 40)):
            out.append(("kite_tip%d_%d_%d_%d" % (tip, a, b1, b2), tile([blunt(a, b1, b2, tip)])))
    # kites whose side tips are the farthest points from the start and lie 64, 128 and 256 scan positions apart: both fall to the same lane of a scan
    # dealt out 32 or 64 lanes wide, where a lane that kept its last maximum would hand on the second tip
    for a, b1, b2 in ((32, 40, 10), (64, 80, 20), (128, 160, 40)):
        out.append(("kite_lane%d" % (2 * a), tile([blunt(a, b1, b2, 1)])))
    for a, c, b in ((30, 5, 44), (26, 7, 40), (34, 9, 50), (30, 6, 38)):   # mirror-symmetric hexagons: vertical sides of c pixels
        out.append(("hexagon_%d_%d_%d" % (a, c, b), tile([[(0, -b), (a, 0), (a, c - 1), (0, b + c - 1), (-a, c - 1), (-a, 0)]])))
    return out


def bumped(w, h, at, bw, depth, deg=0.0, side="top"):
    """rectangle of w x h pixels with a bump (depth > 0) or notch (depth < 0) of bw pixels on its top or left side -> tile"""
    body = rect(0, 0, w, h)
    d = abs(depth)
    if side == "top":
        extra = rect(at, -d, bw, d + 1) if depth > 0 else rect(at, 0, bw, d)
    else:
        extra = rect(-d, at, d + 1, bw) if depth > 0 else rect(0, at, d, bw)
    if deg:
        body, extra = rot(body, deg), rot(extra, deg)
    return tile([body, extra]) if depth > 0 else tile([body], [extra])


# shapes found by search_early_reject's generator (seed 1; shapes 1422, 466, 443), kept as their polygons
MINED_AXIS = [[(0.0, 0.0), (63.61, 23.2), (40.75, 117.78), (-30.18, 116.05)], [(-30.18, 116.05), (-28.8, 44.12), (-19.36, 36.14), (-22.27, 14.29), (0.0, 0.0)],
              [(4.57, 125.09), (-30.18, 116.05), (-28.8, 44.12), (-19.36, 36.14), (-22.27, 14.29), (0.0, 0.0)],
              [(63.61, 23.2), (72.05, 50.62), (69.27, 51.46), (68.02, 77.86), (40.75, 117.78)],
              [(30.33, 15.16), (63.61, 23.2), (72.05, 50.62), (69.27, 51.46), (68.02, 77.86), (40.75, 117.78)],
              [(40.75, 117.78), (4.94, 126.83), (1.37, 128.38), (-11.72, 127.22), (-30.18, 116.05)],
              [(41.27, 96.37), (40.75, 117.78), (4.94, 126.83), (1.37, 128.38), (-11.72, 127.22), (-30.18, 116.05)]]
MINED_RAW6 = [[(29.29, 38.74), (19.65, 34.43), (11.55, 41.73), (-38.48, 31.86), (-52.89, 13.26), (-58.62, -11.69), (-38.24, -28.28), (-16.21, -38.88),
               (4.99, -42.85), (16.26, -36.34), (26.43, -35.1), (37.32, -26.34)]]
MINED_RAW5 = [[(0.0, 0.0), (5.72, 43.43), (-59.59, 63.64), (-78.0, 22.65)], [(0.0, 0.0), (17.47, 32.81), (5.72, 43.43)],
              [(-25.84, 3.41), (0.0, 0.0), (17.47, 32.81), (5.72, 43.43)], [(-59.59, 63.64), (-72.24, 64.2), (-78.0, 22.65)],
              [(-38.12, 53.99), (-59.59, 63.64), (-72.24, 64.2), (-78.0, 22.65)]]


def eps_cases():
    """border of n = 20 d points and a bump / notch of depth d - 1, d, d + 1 against the side it sits on"""
    def build(d, depth, w, bw, at, sign, side):
        # n = 2 (w + h) - 4 + 2 depth - 2: the border cuts the two concave corners diagonally. "left" is the same shape mirrored in the diagonal:
        # the border then starts at a corner of the rectangle, not on the bump
        t = bumped(w, (20 * d + 6 - 2 * depth) // 2 - w, at, bw, sign * depth)
        return t if side == "top" else np.ascontiguousarray(t.T)

    def reaches(t):
        tr = Trace()
        border_quad(outer_border(t), tr)
        return tr.eq_split > 0

    out = []
    for d in (6, 8, 10):
        for sign in (1, -1):
            for side in ("top", "left"):
                # the place and width of the bump at which the side it sits on is the chord of its range: searched, asserted
                w, bw, at = next(p for p in ((40, 3, 12), (50, 5, 30), (62, 4, 20), (46, 4, 15), (54, 3, 24), (58, 5, 18)) if reaches(build(d, d, *p, sign, side)))
                for depth in (d - 1, d, d + 1):
                    out.append(("%s%d_of_%d_%s" % ("bump" if sign > 0 else "notch", depth, d, side), build(d, depth, w, bw, at, sign, side)))
    # turned rectangles on the (4, 3) grid: sides (4 t, 3 t) and (-3 s, 4 s), a border of 300 points (eps = 15) and a bump whose apex is the pixel
    # (9, -12) off its side, 15 away: maxd^2 = (15 * 5 t)^2 = eps^2 |chord|^2
    for t_, s_, j, dl in ((18, 17, 6, 5), (22, 13, 11, 8), (27, 8, 13, 5)):
        u, v, p = (4 * t_, 3 * t_), (-3 * s_, 4 * s_), (4 * j, 3 * j)
        body = [(0, 0), u, (u[0] + v[0], u[1] + v[1]), v]
        bump = [(p[0] - 0.8 * dl, p[1] - 0.6 * dl), (p[0] + 9, p[1] - 12), (p[0] + 0.8 * dl, p[1] + 0.6 * dl)]
        out.append(("turned15_of_15_%d_%d" % (t_, s_), tile([body, bump])))
    for deg in (6.0, 17.0, 33.0):          # turned by other angles: the depth is no whole number of pixels, so these pass on either side of eps
        for depth in (5, 6, 7):
            out.append(("bump%d_deg%g" % (depth, deg), bumped(44, 24, 14, 4, depth, deg)))
    out.append(("clean_equal", tile([clean_equal()])))   # equality in the clean-up pass's bound
    out.append(("axis_only", tile(MINED_AXIS)))          # a vertex that only `dx != 0 && dy != 0` keeps
    out.append(("sip_only", bumped(40, 16, 12, 3, -6, 0.0, "left")))   # a vertex that only `sip >= 0` keeps
    return out


def chamfered(w, h, cuts):
    """rectangle with the corners cut by cuts[i] pixels (0: kept) -> up to 8 vertices"""
    c = cuts
    return [(c[0], 0), (w - c[1], 0), (w, c[1]), (w, h - c[2]), (w - c[2], h), (c[3], h), (0, h - c[3]), (0, c[0])]


def comb(teeth, tw, gap, th, base):
    add = [rect(0, 0, teeth * (tw + gap) - gap, base)]
    for i in range(teeth):
        add.append(rect(i * (tw + gap), -th, tw, th + 1))
    return add


def star(n, r_out, r_in):
    """n-pointed star as a union of triangles round a core"""
    core = [(r_in * math.cos(2 * math.pi * (i + 0.5) / n), r_in * math.sin(2 * math.pi * (i + 0.5) / n)) for i in range(n)]
    add = [core]
    for i in range(n):
        tipp = (r_out * math.cos(2 * math.pi * i / n), r_out * math.sin(2 * math.pi * i / n))
        add.append([core[i - 1], tipp, core[i]])
    return add


def bowed(length, width, apex, bow, bows=2, apexes=2):
    """convex many-gon: a rectangle whose long sides carry a shallow outward vertex `bow` high at their middle and whose short sides one `apex` high.
    The farthest-point passes start at the apexes, so the recursion meets a bow before the corners beside it and emits both; the clean-up pass then
    finds apexes and bows near their neighbours' chords and removes them: 4 + bows + apexes vertices before, the rectangle after"""
    pts = [(0, 0)]
    if bows >= 1:
        pts.append((length / 2, -bow))
    pts.append((length, 0))
    if apexes >= 1:
        pts.append((length + apex, width / 2))
    pts.append((length, width))
    if bows >= 2:
        pts.append((length / 2, width + bow))
    pts.append((0, width))
    if apexes >= 2:
        pts.append((-apex, width / 2))
    return pts


def clean_equal(k=8, w=16, m=54, h=3):
    """a bowed rectangle on the diagonal grid with a border of 20 k points (eps = k): the long side runs from (0, 0) to (m, m) and its bow sits
    k / sqrt(2) off it at a pixel, so the clean-up's dist^2 <= 0.5 eps^2 |chord|^2 reads (k m)^2 <= 0.5 k^2 (2 m^2): equality"""
    return [(0, 0), (m // 2 - k // 2, m // 2 + k // 2), (m, m), (m + w // 2 + h, m - w // 2 + h), (m + w, m - w), (w, -w), (w // 2 - h, -w // 2 - h)]


def vertex_cases():
    out = []
    # 7 and 8 vertices before the clean-up pass, a quad after it: the deepest bookkeeping the device's early reject lets through
    out.append(("raw7_to_4", tile([rot(bowed(120, 40, 5, 5, 1, 2), 20.0)])))
    out.append(("raw7_to_4_deg33", tile([rot(bowed(120, 40, 7, 7, 1, 2), 33.0)])))
    out.append(("raw8_to_4", tile([rot(bowed(100, 40, 7, 7, 2, 2), 20.0)])))
    out.append(("raw8_to_4_deg33", tile([rot(bowed(120, 40, 5, 5, 2, 2), 33.0)])))
    for name, cuts in (("c0", (0, 0, 0, 0)), ("c1", (9, 0, 0, 0)), ("c2", (9, 0, 10, 0)), ("c3", (9, 11, 10, 0)), ("c4", (9, 11, 10, 12)),
                       ("c4big", (14, 15, 16, 13)), ("c4deep", (22, 22, 22, 22))):
        out.append(("chamfer_" + name, tile([chamfered(80, 60, cuts)])))
        out.append(("chamfer_%s_deg13" % name, tile([rot(chamfered(80, 60, cuts), 13.0)])))
    out.append(("raw5_to_4", tile(MINED_RAW5)))
    out.append(("raw6_to_4", tile(MINED_RAW6)))
    out.append(("two_squares", tile([rect(0, 0, 40, 40), rect(50, 50, 40, 40), [(39, 39), (50, 50), (50, 50)]])))   # 8 vertices exactly
    out.append(("comb5", tile(comb(5, 8, 8, 30, 12))))
    out.append(("comb3", tile(comb(3, 10, 14, 26, 10))))
    out.append(("star5", tile(star(5, 40, 16))))
    out.append(("star7", tile(star(7, 44, 24))))
    for k in (9, 10, 12):
        out.append(("gon%d" % k, tile([[(40 * math.cos(2 * math.pi * i / k + 0.2), 40 * math.sin(2 * math.pi * i / k + 0.2)) for i in range(k)]])))
    return out


def frame_tile(w, h, t, corner_extra=0):
    """a frame t pixels thick; corner_extra thickens the top-left corner's two arms so the hole's corner moves"""
    outer = rect(0, 0, w, h)
    hole = rect(t, t, w - 2 * t, h - 2 * t)
    m_add, m_sub = [outer], [hole]
    tl = tile(m_add, m_sub)
    if corner_extra:
        tl[QUIET + t:QUIET + t + corner_extra, QUIET + t:QUIET + t + corner_extra] = 1
    return tl


def integer_cases():
    out = []
    # shortest side exactly 10 / just above: the corners of a parallelogram are pixels, so its quad has exactly these side vectors
    for name, v in (("side_10_0", (10, 0)), ("side_6_8", (6, 8)), ("side_8_6", (8, 6)), ("side_10_1", (10, 1)), ("side_10_2", (10, 2)), ("side_11_0", (11, 0))):
        for u in ((0, 40), (-9, 44)):
            if v[0] * u[1] - v[1] * u[0] == 0:
                continue
            p = [(0, 0), v, (v[0] + u[0], v[1] + u[1]), u]
            out.append(("%s_u%d" % (name, u[0]), tile([p])))
    # three collinear vertices: an axis-aligned side keeps its middle vertex through the clean-up pass
    out.append(("collinear_house", tile([[(0, 0), (30, -30), (60, 0), (60, 40), (0, 40)]])))
    out.append(("collinear_bump", tile([rect(0, 0, 60, 40), [(20, 0), (30, -16), (40, 0)]])))
    out.append(("triangle_flat", tile([[(0, 0), (80, 0), (40, 50)]])))
    # a 4-gon with a zero cross product: a 1-px spur prolongs the triangle's flat side, the border walks out and back, and the spur's foot stays a vertex
    # between the far corner and the tip (its neighbours' chord is axis-aligned and it lies behind the tip): every side is longer than 10
    out.append(("zero_cross_spur", tile([[(0, 0), (60, 0), (30, 50)], rect(60, 0, 40, 1)])))
    for t in (1, 2, 3, 5, 6):
        out.append(("frame_%d" % t, frame_tile(70, 56, t)))
        out.append(("frame_%d_corner" % t, frame_tile(70, 56, t, corner_extra=2)))
    # the hole's quad against the outer border's: three corners nearer than 6 px, the fourth at exactly 6 px (0, 6) / at 5 px
    for name, top in (("near_6", 9), ("near_5", 8)):
        fr = np.zeros((62, 76), np.uint8)
        fr[3:59, 3:73] = 1
        fr[top:58, 4:72] = 0
        out.append((name, fr))
    # three nested near-duplicates: two frames, one inside the other
    nest = np.zeros((72, 72), np.uint8)
    nest[3:69, 3:69] = 1
    nest[6:66, 6:66] = 0
    nest[9:63, 9:63] = 1
    nest[12:60, 12:60] = 0
    out.append(("nested_frames", nest))
    nest2 = np.zeros((72, 72), np.uint8)
    nest2[3:69, 3:69] = 1
    nest2[5:67, 5:67] = 0
    nest2[7:65, 7:65] = 1
    nest2[9:63, 9:63] = 0
    nest2[11:61, 11:61] = 1
    out.append(("nested_frames_2px", nest2))
    return out


def revisit_cases():
    out = []
    # 1-px spurs: the border walks out and back over the same pixels
    for L in (6, 15, 30):
        out.append(("spur_top_%d" % L, tile([rect(0, 0, 60, 44), rect(25, -L, 1, L + 1)])))
        out.append(("spur_corner_%d" % L, tile([rect(0, 0, 60, 44), [(59 + i, -i) for i in (0, L)] + [(59 + L, -L)]])))
        out.append(("spur_side_%d" % L, tile([rot(rect(0, 0, 60, 44), 12.0), rect(60, 20, L, 1)])))
    # 1-px bridges between two quads
    out.append(("bridge_h", tile([rect(0, 0, 40, 40), rect(60, 0, 40, 40), rect(39, 18, 22, 1)])))
    out.append(("bridge_diag", tile([rect(0, 0, 40, 40), rect(50, 50, 40, 40), [(39, 39), (50, 50), (50, 50)]])))
    out.append(("line_only", tile([rect(0, 0, 50, 1)])))
    out.append(("spur_pair", tile([rect(0, 0, 60, 44), rect(10, -12, 1, 13), rect(48, -12, 1, 13)])))
    return out


def couple_cases():
    """a plane whose only kept borders are one of 40 and one of 512 points: whatever the order of the descriptors, these two share a wave"""
    return [("n40", quad_of_count(40)), ("n512", quad_of_count(512))]


FAMILIES = {"length": length_cases, "stride": stride_cases, "pairing_even": lambda: pairing_cases(False), "pairing_odd": lambda: pairing_cases(True),
            "couple": couple_cases,
            "tie": tie_cases, "eps": eps_cases, "vertices": vertex_cases, "integer": integer_cases, "revisit": revisit_cases}

_cache = {}


def family(name):
    """-> (cases [(name, tile)], sheets [(sheet, places)]); built once"""
    if name not in _cache:
        cases = FAMILIES[name]()
        _cache[name] = (cases, pack([t for _, t in cases]))
    return _cache[name]


def all_sheets():
    """-> [(family, index, sheet uint8 0/255)] of every 640 x 480 sheet"""
    return [(fam, i, s) for fam in FAMILIES for i, (s, _) in enumerate(family(fam)[1])]


def sheet_candidates(sheet, min_size=MIN_SIZE, max_size=MAX_SIZE, mut=(), traces=None):
    """the reference's candidate list of one sheet (one plane) -> float32 [k][4][2], and the kept borders"""
    h, w = sheet.shape
    borders = borders_of(sheet)
    cands = detect_rectangles([borders], w, h, min_size, max_size, mut, traces)
    return np.array(cands, np.float32).reshape(-1, 4, 2)


# ------------------------------------------------------------------------------------------------------------------------------------
# several threshold planes: two flat dark rectangles on a flat ground under the adaptive threshold. A plane marks a ring inside each rectangle, as thick
# as half its window: the outer borders, and so their quads, are the same on every plane (equal perimeters: the tie removes the earlier one), the
# hole's quad shrinks as the window grows.
#   (15, 1): windows 15, 15, 17. The survivors of a tie are the last plane's under the right reading and the first plane's under `tie_j`; the holes'
#            survivors come from a middle plane, so the list's order tells the readings apart.
#   (9, 3):  windows 7, 9, 13, 15, 19, 21, 25. The holes' quads form a chain, each near the next but the first not near the last, and the outer quads remove the
#            first of them: quads already removed go on removing.
# ------------------------------------------------------------------------------------------------------------------------------------
MULTI_MIN, MULTI_MAX = 0.04, 0.5
MULTI_PARAMS = ((15, 1), (9, 3))
MULTI_COUNT = {(15, 1): 4, (9, 3): 2}   # candidates left: both outer quads and both holes' / the outer quads alone, the whole chain gone


def multi_frame():
    g = np.full((SHEET_H, SHEET_W), 200, np.uint8)
    g[40:140, 60:180] = 30
    g[200:330, 300:420] = 30
    return g


def plane_windows(p1, rng):
    """the adaptive threshold's window of every plane of MarkerDetector::detect: p1 - rng + rng i, made odd and at least 3"""
    out = []
    for i in range(2 * rng + 1):
        p = p1 - rng + rng * i
        out.append(3 if p < 3 else p + 1 if p % 2 != 1 else p)
    return out


def multi_planes(gray, p1, rng, p2=7.0):
    """-> per plane the borders of the oracle's adaptive threshold (thresholding is pinned elsewhere)"""
    from oracle import orc
    return [borders_of(orc.adaptive_threshold(gray, w, p2)) for w in plane_windows(p1, rng)]


def multi_candidates(gray, p1, rng, mut=(), traces=None):
    h, w = gray.shape
    cands = detect_rectangles(multi_planes(gray, p1, rng), w, h, MULTI_MIN, MULTI_MAX, mut, traces)
    return np.array(cands, np.float32).reshape(-1, 4, 2)


FAR_W, FAR_H = 16368, 72


def far_sheet():
    """a turned quad and a chamfered one at the far right of a 16368 x 72 frame: coordinates near 2^14"""
    s = np.zeros((FAR_H, FAR_W), np.uint8)
    for t, x in ((tile([rot(rect(0, 0, 52, 40), 9.0)]), FAR_W - 1), (tile([chamfered(50, 44, (6, 0, 7, 0))]), FAR_W - 72), (tile([blunt(20, 28, 28, 2)]), FAR_W - 140)):
        th, tw = t.shape
        assert th <= FAR_H - 2
        s[1:1 + th, x - tw:x] = t * 255
    return s


# ------------------------------------------------------------------------------------------------------------------------------------
# the search behind contour_quad's early reject: is there a border with more than 8 vertices before the clean-up pass that ends as a quad?
# ------------------------------------------------------------------------------------------------------------------------------------
def random_shape(rng):
    """-> (polygons to fill, polygons to cut out): a quad with bumps and notches round eps deep, a rectangle with bulging sides, an irregular 9- to 12-gon or a
    rounded rectangle"""
    kind = rng.randint(0, 16)
    if kind >= 10:
        # a rectangle every side of which bulges as a shallow convex arc of 1 to 3 vertices, about eps high: the farthest-point passes start on the short
        # sides' arcs, the recursion emits arc vertices before the corners, and the clean-up pass has near-collinear triples to work on. These are
        # the shapes that reach 9 and more vertices before the clean-up pass
        length = rng.uniform(80, 170)
        width = length * rng.uniform(0.3, 0.7)
        eps = 0.1 * (length + width)
        sides = [((0, 0), (length, 0)), ((length, 0), (length, width)), ((length, width), (0, width)), ((0, width), (0, 0))]
        pts = []
        for i, ((x0, y0), (x1, y1)) in enumerate(sides):
            pts.append((x0, y0))
            side = math.hypot(x1 - x0, y1 - y0)
            nx, ny = (y1 - y0) / side, -(x1 - x0) / side
            high = eps * rng.uniform(0.3, 1.3)
            for t in sorted(rng.uniform(0.1, 0.9, rng.randint(0 if i % 2 else 1, 4))):
                d = high * (1.0 - (2.0 * t - 1.0) ** 2)
                pts.append((x0 + t * (x1 - x0) + d * nx, y0 + t * (y1 - y0) + d * ny))
        return [rot(pts, rng.uniform(0, 90))], ()
    if kind < 7:
        # a quad with up to four triangular bumps or notches per side, their depths round 0.05 n and 0.035 n (eps and eps / sqrt 2): every bump near eps is
        # a vertex the recursion may emit and the clean-up pass may take back
        w, h = rng.uniform(40, 130), rng.uniform(40, 130)
        q = rot([(0, 0), (w + rng.uniform(-12, 12), rng.uniform(-12, 12)), (w, h), (rng.uniform(-12, 12), h + rng.uniform(-12, 12))], rng.uniform(0, 90))
        n = 2.0 * (w + h)
        add, sub = [q], []
        for i in range(4):
            (x0, y0), (x1, y1) = q[i - 1], q[i]
            L = math.hypot(x1 - x0, y1 - y0)
            ux, uy = (x1 - x0) / L, (y1 - y0) / L
            nx, ny = uy, -ux                               # outward: the quad runs clockwise on the screen
            for t in rng.uniform(0.1, 0.9, rng.randint(0, 6)):
                d = rng.choice((0.05, 0.035)) * n * rng.uniform(0.6, 2.0)
                half = rng.uniform(2.0, max(3.0, 0.12 * L))
                bx, by = x0 + t * (x1 - x0), y0 + t * (y1 - y0)
                if rng.randint(0, 3):
                    add.append([(bx - half * ux - nx, by - half * uy - ny), (bx + d * nx, by + d * ny), (bx + half * ux - nx, by + half * uy - ny)])
                else:
                    sub.append([(bx - half * ux + nx, by - half * uy + ny), (bx - d * nx, by - d * ny), (bx + half * ux + nx, by + half * uy + ny)])
        return add, sub
    if kind < 9:
        k = rng.randint(9, 13)
        ang = np.sort(rng.uniform(0, 2 * math.pi, k))
        r = rng.uniform(30, 70)
        return [[(r * rng.uniform(0.85, 1.0) * math.cos(a) * rng.uniform(1.0, 1.6), r * rng.uniform(0.85, 1.0) * math.sin(a)) for a in ang]], ()
    w, h = rng.uniform(50, 140), rng.uniform(50, 140)
    r = rng.uniform(4, 0.5 * min(w, h))
    arc = [(r - r * math.cos(a), r - r * math.sin(a)) for a in np.linspace(0, math.pi / 2, 6)]
    pts = arc + [(w - x, y) for x, y in arc[::-1]] + [(w - x, h - y) for x, y in arc] + [(x, h - y) for x, y in arc[::-1]]
    return [rot(pts, rng.uniform(0, 90))], ()


def search_early_reject(seed, seconds, on_shape=None, shapes=None):
    """seeded; stops after `seconds` or `shapes` shapes -> (shapes tried, borders of more than 8 raw vertices, those among them that end as an accepted quad
    [(seed, index)])"""
    import time
    rng = np.random.RandomState(seed)
    t0, tried, deep, found = time.time(), 0, 0, []
    while time.time() - t0 < seconds and (shapes is None or tried < shapes):
        t = tile(*random_shape(rng))
        tried += 1
        for b in borders_of(t * 255):
            if len(b) < 60:
                continue
            tr = Trace()
            q = border_quad(b, tr)
            deep += tr.raw > 8
            if tr.raw > 8 and q is not None:
                found.append((seed, tried - 1))
            if on_shape:
                on_shape(tried - 1, t, b, tr, q)
    return tried, deep, found
