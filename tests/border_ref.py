"""Border following (aruco_amd/csrc/k_contours.hip: candidates_sparse_kernel + walker_kernel + walker_long_kernel + late_quad_kernel's walkers;
k_segments.hip) at its edge topologies: an exact reference, a restatement of the walker formulation, deliberate misreadings of both, and the generator of
the hand-made sheets. CPU only, plain Python ints, one pixel at a time.

scan_borders()    cv::findContours(RETR_LIST, CHAIN_APPROX_NONE) as OpenCV 3.0 codes it (cvStartFindContours / cvFindNextContour / icvFetchContour),
                  written from the algorithm: a second reading beside oracle/orc_imgproc.cpp, which tests/test_border_edges_cpu.py holds it against.
walk_survivors()  the device's formulation, not its code: the start candidates of tests/cand_ref.py, one walk per candidate with the same step rule, dropped
                  by the rules the header of k_contours.hip states (outer: a visited pixel precedes the start in raster order; hole: an examined
                  background 4-neighbour precedes the trigger), after a backward walk in the x-mirrored image (the reverse probe), then the size filter.
                  Order: the device keeps a plane's borders in no order of its own (slots come from atomics); debug_contours sorts them by ContourDesc::key
                  (the trigger's raster index) descending, which is the scan's reverse discovery order. walk_survivors returns that order.
MUTATIONS         misreadings of either; the CPU test shows that the cases below tell every one of them from the right reading.

Formats (size_limits with the float32 arithmetic of quad_ref.size_limits):
  sheet  256 x 192, min_size 0.01, max_size 1.0   borders of 11 .. 1023 points pass: the leash (64) and the generations that end at 192, 448 and 960
  odd    253 x 189, the same sizes                borders of 11 .. 1011 points pass: no multiple of 8 either way
  strip 1024 x  96, the same sizes                borders of 41 .. 4095 points pass: the generations that end at 1984, 3008 and 4032
  reach  256 x 192, max_size 0.25                 borders of 11 .. 255 points pass. With max_size 1.0 the early exit `2 * reach >= max_contour` can never
                                                  be the first thing to end a walk (max_contour = 4 * max(W, H), reach <= max(W, H) - 3), so the straight
                                                  lines with n == 2 * reach == max_contour - 2 and == max_contour live on a format of their own.

What could not be built, and why:
  * a true start pixel that its own border passes three times. An outer start has W, NW, N and NE clear; the border passes it once per run of clear
    neighbours that holds a 4-neighbour, and E, SE, S, SW leave room for one such run (S, between SW and SE / E) beside the one that holds W and N: two
    passes at most. A hole's first pixel p has the trigger E of it and a set NE; a clear W, NW or N of p precedes the trigger, so it belongs to another
    background region and another border: again only E and S remain. The CPU test asserts two passes in both polarities and that no border of any case,
    noise included, passes its start a third time (so the argument is checked, not only stated). Pixels other than the start are passed up to 4 times.
  * a hole border whose trigger lies in column W - 2. The clear pixel there is 4-connected to the cleared frame column, so it belongs to the outer
    background and the set pixel W of it got the negative mark from an outer border. The frame family holds the start-rule pixel (a false hole start in
    column W - 2, which the run rule drops and is_waypoint's `x + 1 <= width - 2` must not take for a hole start) and a true hole trigger at W - 3.
"""
import numpy as np

from tests import cand_ref
from tests.quad_ref import size_limits

DX = (1, 1, 0, -1, -1, -1, 0, 1)      # E NE N NW W SW S SE
DY = (0, -1, -1, -1, 0, 1, 1, 1)

SCAN_MUTATIONS = ("close_on_start", "first_ccw", "hole_from_4", "no_neg_mark", "hole_any_prev", "no_reread", "four_conn", "keep_frame", "size_le_min",
                  "size_le_max", "discovery_order")
WALK_MUTATIONS = ("outer_le", "hole_E_le", "hole_W_le", "reach_gt")
MUTATIONS = SCAN_MUTATIONS + WALK_MUTATIONS
# size_le of the issue is two misreadings, one per bound.
# Dropped from the issue's list, because no image can tell them from the right reading by its survivors: hole_no_W, hole_no_E, hole_no_N (CLAUSE_MUTATIONS,
# with hole_no_S). A false hole start follows the border of a hole whose first pixel t' precedes its own trigger. Unless it is dropped earlier, the walk
# passes the set pixel W of t' and examines t' as that pixel's E neighbour, and it passes the set pixel N of t' and examines t' as its S neighbour: with
# one clause left out another one still fires, at the latest there. Leaving a clause out only lets false starts live longer - a loss of speed, which the
# traces show (the candidate's forward proof moves) and which the CPU test asserts instead: for each of W, E and N some candidate's proof is that clause
# alone, and the misreading moves it. The S clause never fires first in any case, noise included: a clear pixel that precedes the trigger is examined
# from the border pixel beside it before the walk gets above it.
CLAUSE_MUTATIONS = ("hole_no_W", "hole_no_E", "hole_no_N", "hole_no_S")

FORMATS = {"sheet": (256, 192, 0.01, 1.0), "odd": (253, 189, 0.01, 1.0), "strip": (1024, 96, 0.01, 1.0), "reach": (256, 192, 0.01, 0.25)}
PROBE, LEASH = 10, 64
GEN_ENDS = (192, 448, 960, 1984, 3008, 4032)     # then + 1024 each


def limits(fmt):
    w, h, lo, hi = FORMATS[fmt]
    return size_limits(w, h, lo, hi)


# ---------------------------------------------------------------------------------------------------------------------------------------
# a. the sequential scan
# ---------------------------------------------------------------------------------------------------------------------------------------

def _trace(img, x0, y0, hole, mut, cap):
    """icvFetchContour on img[y][x] (ints; 0 clear, 1 set, 2 / -2 marked), relabels as it goes -> points"""
    step = 2 if "four_conn" in mut else 1
    s_end = s = 4 if ("hole_from_4" in mut or not hole) else 0
    while True:                                   # 4. first search, clockwise
        s = (s + step) & 7 if "first_ccw" in mut else (s - step) & 7
        if img[y0 + DY[s]][x0 + DX[s]] != 0 or s == s_end:
            break
    if s == s_end:                                # isolated pixel
        img[y0][x0] = -2
        return [(x0, y0)]
    x1, y1 = x0 + DX[s], y0 + DY[s]               # the first neighbour
    x3, y3 = x0, y0
    pts = []
    while True:                                   # 5. the step loop, counter-clockwise from the previous pixel
        s_end = s
        while True:
            s += step
            x4, y4 = x3 + DX[s & 7], y3 + DY[s & 7]
            if img[y4][x4] != 0:
                break
        s &= 7
        if ((s - 1) & 0xFFFFFFFF) < s_end and "no_neg_mark" not in mut:      # 6. the east neighbour was examined and is clear
            img[y3][x3] = -2
        elif img[y3][x3] == 1:
            img[y3][x3] = 2
        pts.append((x3, y3))
        if x4 == x0 and y4 == y0 and ((x3 == x1 and y3 == y1) or "close_on_start" in mut):      # 7. closure
            break
        if len(pts) >= cap:                       # only a misreading gets here
            break
        x3, y3 = x4, y4
        s = (s + 4) & 7
    return pts


def scan_borders(binimg, mut=()):
    """-> [{"hole", "trig": (x, y), "pts": int32 [n][2]}] in cv::findContours' order (RETR_LIST: last found first)"""
    b = np.asarray(binimg) != 0
    H, W = b.shape
    # one spare clear ring, so that keep_frame's walks along the frame read defined pixels; coordinates below are shifted by one
    img = [[0] * (W + 2)] + [[0] + [1 if v else 0 for v in row] + [0] for row in b.tolist()] + [[0] * (W + 2)]
    if "keep_frame" not in mut:                   # 1. the 1-px frame
        img[1] = [0] * (W + 2)
        img[H] = [0] * (W + 2)
        for y in range(1, H + 1):
            img[y][1] = img[y][W] = 0
    found = []
    cap = 32768                                   # more points than any border of the cases has: ends the walks of a misreading that never closes
    for y in range(2, H):                         # 2. raster scan over the rows and columns 1 .. size - 2
        row = img[y]
        prev = 0
        for x in range(2, W):
            p = row[x]
            if p == prev:
                continue
            hole = 0
            if not (prev == 0 and p == 1):        # 3. outer or hole
                if p != 0 or (prev < 1 and "hole_any_prev" not in mut):
                    prev = p
                    continue
                hole = 1
            pts = _trace(img, x - hole, y, hole, mut, cap)
            found.append({"hole": hole, "trig": (x - 1, y - 1), "pts": np.array(pts, np.int32).reshape(-1, 2) - 1})
            prev = p if "no_reread" in mut else row[x]      # 8. the scanner reads the pixel again
    if "discovery_order" not in mut:              # 9.
        found.reverse()
    return found


def size_filter(borders, lo, hi, mut=()):
    lo_ok = (lambda n: n >= lo) if "size_le_min" in mut else (lambda n: n > lo)
    hi_ok = (lambda n: n <= hi) if "size_le_max" in mut else (lambda n: n < hi)
    return [c for c in borders if lo_ok(len(c["pts"])) and hi_ok(len(c["pts"]))]


# ---------------------------------------------------------------------------------------------------------------------------------------
# b. the walker formulation
# ---------------------------------------------------------------------------------------------------------------------------------------

def _first_dir(pix, x, y, s_end, mirror):
    s = s_end
    while True:
        s = (s - 1) & 7
        if pix(x + (-DX[s] if mirror else DX[s]), y + DY[s]) or s == s_end:
            break
    return -1 if s == s_end else s


def _walk(pix, hole, tx, ty, mirror, nmax, max_evals, mut):
    """One walk from the candidate's first pixel. mirror: directions are those of the x-mirrored image (the same border the other way round);
    positions stay real. -> (verdict "bad" | "closed" | "long" | "open" | "isolated", evaluations of the drop rule, points, clauses at the proof)"""
    x0, y0 = tx - hole, ty
    sgn = -1 if mirror else 1
    s = _first_dir(pix, x0, y0, (0 if hole else 4) ^ (4 if mirror else 0), mirror)
    if s < 0:
        return "isolated", 0, [(x0, y0)], ()
    x1, y1 = x0 + sgn * DX[s], y0 + DY[s]
    x, y = x0, y0
    pts = []
    reach = 0
    while True:
        # the directions examined and found clear, then the next border pixel
        ex = []
        d = s
        while True:
            d = (d + 1) & 7
            nx, ny = x + sgn * DX[d], y + DY[d]
            if pix(nx, ny):
                break
            ex.append((d, nx, ny))
        n = len(pts) + 1                                     # this evaluation's number
        fired = []
        if hole:
            for e, zx, zy in ex:
                if e & 1:
                    continue                                 # 4-neighbours only
                name = {0: "W" if mirror else "E", 2: "N", 4: "E" if mirror else "W", 6: "S"}[e]
                if "hole_no_" + name in mut:
                    continue
                before = (zy, zx) < (ty, tx)
                if "hole_%s_le" % name in mut:
                    before = (zy, zx) <= (ty, tx)
                if before:
                    fired.append(name)
        else:
            if (y, x) < (y0, x0) or ("outer_le" in mut and n > 1 and (y, x) == (y0, x0)):
                fired.append("P")
        pts.append((x, y))
        if fired:
            return "bad", n, pts, tuple(sorted(fired))
        reach = max(reach, abs(nx - x0), abs(ny - y0))
        if nx == x0 and ny == y0 and x == x1 and y == y1:
            return "closed", n, pts, ()
        if n >= nmax or 2 * (reach + (1 if "reach_gt" in mut else 0)) >= nmax:
            return "long", n, pts, ()
        if n >= max_evals:
            return "open", n, pts, ()
        x, y = nx, ny
        s = (d + 4) & 7


def stage_of(fwd):
    """where a walk that ends at its fwd-th evaluation ends: "first" pass or the number of its generation"""
    if fwd <= LEASH:
        return "first"
    g, end = 1, GEN_ENDS[0]
    while fwd > end:
        g += 1
        end = GEN_ENDS[g - 1] if g <= len(GEN_ENDS) else end + 1024
    return g


def walk_survivors(binimg, min_contour, max_contour, mut=(), probe=PROBE, traces=None):
    """-> the borders the formulation keeps, in debug_contours' order. traces (a list): one dict per candidate -
    hole, trig, n (forward evaluations), fwd / back (evaluations up to the proof, None without one), verdict (kept | probe | bad | long | small |
    isolated), stage (of a false start or a long one: probe | first | generation), clauses (of the hole rule, at the proof)"""
    b = cand_ref.binary_of(binimg)
    H, W = b.shape
    rows = b.tolist()
    pix = lambda x, y: 0 <= x < W and 0 <= y < H and rows[y][x]
    cands = cand_ref.start_candidates(b, drop_single=min_contour >= 1)
    kept = []
    for hole, name in ((0, "outer"), (1, "hole")):
        for key in cands[name].tolist():
            tx, ty = key & 0xFFFF, key >> 16
            tr = {"hole": hole, "trig": (tx, ty), "n": 0, "fwd": None, "back": None, "clauses": (), "stage": None}
            rv, rn, _, rcl = _walk(pix, hole, tx, ty, True, max_contour, 64, mut)
            if rv == "bad":
                tr["back"] = rn
            if rv == "isolated":
                tr["verdict"] = "isolated"
            elif rv == "bad" and rn <= probe:
                tr["verdict"], tr["stage"], tr["clauses"] = "probe", "probe", rcl
            else:
                v, n, pts, cl = _walk(pix, hole, tx, ty, False, max_contour, 1 << 30, mut)
                tr["n"] = n
                if v == "bad":
                    tr["verdict"], tr["fwd"], tr["clauses"], tr["stage"] = "bad", n, cl, stage_of(n)
                elif v == "long" or n >= max_contour:
                    tr["verdict"], tr["stage"] = "long", stage_of(n)
                elif n <= min_contour:
                    tr["verdict"] = "small"
                else:
                    tr["verdict"] = "kept"
                    kept.append({"hole": hole, "trig": (tx, ty), "pts": np.array(pts, np.int32)})
            if traces is not None:
                traces.append(tr)
    kept.sort(key=lambda c: -(c["trig"][1] * W + c["trig"][0]))
    return kept


# ---------------------------------------------------------------------------------------------------------------------------------------
# c. what a border and a sheet reach
# ---------------------------------------------------------------------------------------------------------------------------------------

def border_trace(c, W, H):
    pts = c["pts"]
    n = len(pts)
    x0, y0 = c["trig"][0] - c["hole"], c["trig"][1]
    _, counts = np.unique(pts[:, 1].astype(np.int64) * 65536 + pts[:, 0], return_counts=True)
    lo, hi = pts.min(0), pts.max(0)
    reach = int(np.abs(pts - np.array([x0, y0])).max())

    def crosses(a, b, g):      # a coordinate in a .. b is a multiple of g
        return (b // g) * g >= a

    return {"n": n, "mod16": n % 16, "hole": c["hole"], "start_passes": int(((pts[:, 0] == x0) & (pts[:, 1] == y0)).sum()),
            "visits": {k: int((counts == k).sum()) for k in (1, 2, 3, 4)}, "max_visits": int(counts.max()), "reach": reach,
            "frame": (int(lo[0]) - 1, int(lo[1]) - 1, W - 2 - int(hi[0]), H - 2 - int(hi[1])),      # left, top, right, bottom
            "grid": {g: (crosses(int(lo[0]), int(hi[0]), g), crosses(int(lo[1]), int(hi[1]), g)) for g in (8, 16, 32)}}


# ---------------------------------------------------------------------------------------------------------------------------------------
# e. the generator. A piece is a small bool array (set = True) cropped to its pixels; the packer puts pieces on images of a format one clear pixel
#    apart, as drawn (their borders are outer borders) or cut out of a filled rectangle (hole borders).
# ---------------------------------------------------------------------------------------------------------------------------------------

def _pad(a, k=1, value=False):
    return np.pad(np.asarray(a, bool), k, constant_values=value)


def cut_out(piece):
    """the piece as clear pixels in a filled rectangle (a wall of one pixel around the piece's bounding box), with a clear margin of its own"""
    return _pad(~_pad(piece, 1), 1)


def _longest(piece, hole):
    bs = [c for c in scan_borders(_pad(piece)) if c["hole"] == hole]
    return max(len(c["pts"]) for c in bs) if bs else 0


def snake(k, run):
    """the first k pixels of a 1-px serpentine: runs of `run` pixels on every second row, joined at alternating ends -> piece"""
    per = run + 1
    nrows = 2 * ((k + per - 1) // per) + 1
    a = np.zeros((nrows, run), bool)
    for i in range(k):
        r, j = divmod(i, per)
        if j < run:
            a[2 * r, j if r % 2 == 0 else run - 1 - j] = True
        else:
            a[2 * r + 1, run - 1 if r % 2 == 0 else 0] = True
    used = np.flatnonzero(a.any(1))
    return a[:used[-1] + 1]


def _end_of_snake(k, run):
    r, j = divmod(k - 1, run + 1)
    if j < run:
        return (j if r % 2 == 0 else run - 1 - j), 2 * r, (1 if r % 2 == 0 else -1)
    return (run - 1 if r % 2 == 0 else 0), 2 * r + 1, 0


def _capped(k, run, cap):
    """snake(k, run) with an end cap: 0 none, 1 a diagonal pixel, 2 a 3-pixel corner, 3 a 2x2 block"""
    a = snake(k, run)
    a = np.pad(a, ((0, 3), (2, 2)))
    x, y, dirx = _end_of_snake(k, run)
    x += 2
    fx = dirx if dirx else 1
    if cap == 1:
        a[y + 1, x + fx] = True
    elif cap == 2:
        a[y + 1, x] = a[y + 1, x - fx] = True
    elif cap == 3:
        a[y + 1, x] = a[y + 1, x + fx] = a[y, x + fx] = True
    used_r, used_c = np.flatnonzero(a.any(1)), np.flatnonzero(a.any(0))
    return a[used_r[0]:used_r[-1] + 1, used_c[0]:used_c[-1] + 1]


def exact_piece(n, hole, run):
    """a serpentine whose longest border of the given kind has exactly n points (searched with scan_borders over length and end cap)"""
    k = max(2, n // 2 - 3 - 2 * (n // (2 * run) + 1))
    while k < n // 2 + 8:
        best = 0
        for cap in (0, 1, 2, 3):
            p = _capped(k, run, cap)
            piece = cut_out(p) if hole else p
            got = _longest(piece, hole)
            if got == n:
                return piece
            best = max(best, got)
        k += max(1, (n - best) // 2 - 2)      # a pixel more is two points more, a turn a little less
    raise AssertionError("no serpentine with a border of %d points (hole %d, runs of %d)" % (n, hole, run))


def ring(w, h):
    a = np.ones((h, w), bool)
    a[1:-1, 1:-1] = False
    return a


def diamond(r):
    """a 1-px ring of diagonal steps only"""
    a = np.zeros((2 * r + 1, 2 * r + 1), bool)
    for i in range(r + 1):
        a[i, r - i] = a[i, r + i] = a[2 * r - i, r - i] = a[2 * r - i, r + i] = True
    return a


def line(k, dx, dy):
    a = np.zeros((1 + (k - 1) * abs(dy), 1 + (k - 1) * abs(dx)), bool)
    for i in range(k):
        a[i * dy if dy >= 0 else (k - 1 - i) * -dy, i * dx if dx >= 0 else (k - 1 - i) * -dx] = True
    return a


def arms(dirs, length=6):
    """a pixel with 1-px dead-end arms in the given directions"""
    a = np.zeros((2 * length + 1, 2 * length + 1), bool)
    a[length, length] = True
    for d in dirs:
        for i in range(1, length + 1):
            a[length + i * DY[d], length + i * DX[d]] = True
    used_r, used_c = np.flatnonzero(a.any(1)), np.flatnonzero(a.any(0))
    return a[used_r[0]:used_r[-1] + 1, used_c[0]:used_c[-1] + 1]


def comb(heights, pitch=2, mirror=False):
    """1-px tines on a base row, `pitch` columns apart; tine i is heights[i] pixels high. Descending heights: every top but the first is a false
    start whose forward proof lies on the tine to its left, about twice its height away; mirrored, the proof lies backwards"""
    hmax = max(heights)
    a = np.zeros((hmax + 1, pitch * (len(heights) - 1) + 1), bool)
    a[hmax] = True
    for i, h in enumerate(heights):
        a[hmax - h:hmax, i * pitch] = True
    return a[:, ::-1] if mirror else a


def span(h, L):
    """two tines a base of L pixels apart, the right one a pixel lower: its top is a false start whose forward proof lies h + L + h steps away"""
    a = np.zeros((h + 1, L), bool)
    a[h] = True
    a[0:h, 0] = True
    a[1:h, L - 1] = True
    return a


def span_for(fwd, hole, h):
    """span(h, L) with L such that its false start (the right tine's top; cut out: the right clear tine's top) is proven false at exactly its fwd-th
    forward evaluation: the last step of a stage or the first of the next"""
    L = fwd - 2 * h
    for _ in range(4):
        p = span(h, L)
        tr = []
        walk_survivors(np.where(_pad(cut_out(p) if hole else p, 3), 255, 0).astype(np.uint8), 0, 1 << 20, traces=tr)
        got = max(t["fwd"] for t in tr if t["hole"] == hole and t["verdict"] == "bad")
        if got == fwd:
            return p
        L += fwd - got
    raise AssertionError("no span with a forward proof at %d (hole %d)" % (fwd, hole))


HANDOVER_PROOFS = {"sheet": ((64, 20), (65, 20), (192, 50), (193, 50), (448, 120), (449, 120)), "strip": ((960, 80), (961, 80))}     # (evaluation, tine height)


def row_slots(widths, gap=1):
    """clear slots on ONE row (drawn as set pixels for cut_out), `gap` wall pixels apart, joined below by a clear row two rows down through a clear
    pixel under each slot's last column: every slot's first pixel is a hole start candidate on the trigger's own row"""
    W = sum(widths) + gap * (len(widths) - 1)
    a = np.zeros((3, W), bool)
    x = 0
    for w in widths:
        a[0, x:x + w] = True
        a[1, x + w - 1] = True
        x += w + gap
    a[2] = True
    return a


def wheel():
    """a block with an X of missing pixels whose NW arm runs out through the corner: cut out, the X is a set peninsula hanging into ONE hole from the
    wall's corner, and the hole border passes its centre four times (a pixel with four clear 4-neighbours of one hole can only be such a peninsula's:
    set pixels on two sides of it that both reached the wall would split the hole)"""
    a = np.ones((9, 9), bool)
    for i in range(-4, 3):
        a[4 + i, 4 + i] = False
    for i in (1, 2):
        a[4 - i, 4 + i] = a[4 + i, 4 - i] = False
    return a


def plus(r):
    return arms((0, 2, 4, 6), r)


def cross(r):
    return arms((1, 3, 5, 7), r)


def checker(n):
    return (np.indices((n, n)).sum(0) % 2) == 0


def pack(fmt, pieces, x0=2, y0=2):
    """shelves of pieces, one clear pixel apart, on as many images of the format as it takes -> [uint8 0/255 images]"""
    W, H = FORMATS[fmt][:2]
    out, img = [], np.zeros((H, W), bool)
    x, y, shelf = x0, y0, 0
    for p in pieces:
        ph, pw = p.shape
        assert pw <= W - 2 - x0 and ph <= H - 2 - y0, (fmt, p.shape)
        if x + pw > W - 1:
            x, y, shelf = x0, y + shelf + 1, 0
        if y + ph > H - 1:
            out.append(img)
            img = np.zeros((H, W), bool)
            x, y, shelf = x0, y0, 0
        img[y:y + ph, x:x + pw] |= p
        x += pw + 1
        shelf = max(shelf, ph)
    out.append(img)
    return [np.where(i, 255, 0).astype(np.uint8) for i in out]


def both(pieces):
    """every piece as drawn and cut out"""
    return [q for p in pieces for q in (p, cut_out(p))]


# the issue lists {11, 12} and {41, 42} around min_contour; the dropped side of that boundary is n == min_contour itself, 10 and 40, added here
SHEET_LENGTHS = (10, 11, 12, 63, 64, 65, 191, 192, 193, 447, 448, 449, 959, 960, 961, 1022, 1023, 1024)
STRIP_LENGTHS = (40, 41, 42, 63, 64, 65, 191, 192, 193, 447, 448, 449, 959, 960, 961, 1983, 1984, 1985, 3007, 3008, 3009, 4031, 4032, 4033, 4094, 4095, 4096)


def _exact(fmt, lengths, run_of):
    return pack(fmt, [exact_piece(n, hole, run_of(n)) for n in lengths for hole in (0, 1)])


def _frame_images(fmt):
    """shapes across every side and corner (the scan clears the frame), lines on row / column 1 and size - 2, starts at x = 1 and y = 1, the hole
    start-rule pixel in column W - 2 and a hole trigger at W - 3, a border along each clamped side"""
    W, H = FORMATS[fmt][:2]
    a = np.zeros((H, W), bool)
    a[0:6, 0:9] = True                                   # corners: filled blocks that reach into the frame
    a[0:7, W - 8:W] = True
    a[H - 5:H, 0:10] = True
    a[H - 9:H, W - 6:W] = True
    a[0:4, 40:60] = True                                 # across each side
    a[H - 4:H, 40:60] = True
    a[10:18, 0:4] = True
    a[10:18, W - 4:W] = True
    a[1, 70:110] = True                                  # 1-px lines on the first and last rows and columns the scan sees
    a[H - 2, 70:110] = True
    a[20:44, 1] = True
    a[20:44, W - 2] = True
    a[0:12, 120:150] = True                              # holes against the frame: the wall towards it is the cleared frame's neighbour
    a[1:8, 123:147] = False
    a[H - 12:H, 120:150] = True
    a[H - 8:H - 1, 123:147] = False
    a[46:62, 0:20] = True
    a[48:60, 1:17] = False
    a[46:62, W - 20:W] = True
    a[48:60, W - 17:W - 3] = False                       # its columns end at W - 4: the wall is W - 3 .. W - 1
    a[47, W - 2] = False                                 # a notch in column W - 2, open to the frame: a hole start-rule pixel there, no hole
    a[64:80, W - 20:W] = True
    a[66:78, W - 3] = False                              # a hole whose first pixel, its trigger, lies in column W - 3: a wall of one pixel (W - 2) inside the frame
    a[72:78, W - 17:W - 3] = False
    b = np.zeros((H, W), bool)                           # the second image: rings that run along every clamped side, and nothing else in the corners
    b[1:H - 1, 1:W - 1] = ring(W - 2, H - 2)
    b[3:H - 3, 3:W - 3] = ring(W - 6, H - 6)
    b[6:30, 6:30] = checker(24)
    return [np.where(i, 255, 0).astype(np.uint8) for i in (a, ~a, b, ~b)]


def _grid_images(fmt):
    W, H = FORMATS[fmt][:2]
    a = np.zeros((H, W), bool)
    a[9:15, 9:15] = ring(6, 6)                           # inside one 8x8 cell: touches no multiple of 8
    a[17:31, 17:31] = ring(14, 14)                       # inside one 16x16 cell
    a[33:63, 33:63] = ring(30, 30)                       # inside one 32x32 cell
    a[64, 70:140] = True                                 # 1-px lines on grid lines
    a[70:140, 64] = True
    a[96:129, 96:161] = ring(65, 33)                     # a rectangle whose sides lie on grid lines (rows 96, 128; columns 96, 160)
    a[100:125, 100:157] = True                           # and a filled one inside, not on them
    a[140:180, 31:34] = True                             # a 3-px bar across a grid column
    s = snake(150, 2)                                    # pitch 2, runs of 2 on columns 191 and 192: every run crosses the grid column
    a[70:70 + s.shape[0], 191:191 + s.shape[1]] |= s
    a[8, 200:216] = True                                 # lines along grid rows 8 and 16 only
    a[16, 200:232] = True
    out = [a, cut_out(a[2:-2, 2:-2])[:H, :W]]
    res = []
    for i in out:
        full = np.zeros((H, W), bool)
        full[:i.shape[0], :i.shape[1]] = i[:H, :W]
        res.append(np.where(full, 255, 0).astype(np.uint8))
    return res


def _noise(fmt, p, seed):
    W, H = FORMATS[fmt][:2]
    return [np.where(np.random.RandomState(seed).rand(H, W) < p, 255, 0).astype(np.uint8)]


def _thin_pieces():
    two = np.zeros((9, 9), bool)                         # two components touching by a corner
    two[0:5, 0:5] = ring(5, 5)
    two[4:9, 4:9] |= ring(5, 5)
    two[4, 4] = False
    two[3, 3] = two[5, 5] = True
    two[4, 3] = two[3, 4] = two[5, 4] = two[4, 5] = False
    inner = _pad(ring(12, 12), 0)                        # a component touching a hole's wall by a corner
    inner[1:4, 1:4] = [[0, 1, 1], [1, 1, 1], [1, 1, 0]]
    inner[5:8, 5:8] = True
    inner[4, 4] = True
    conc = ring(15, 15)                                  # concentric 1-px rings one pixel apart
    conc[2:13, 2:13] |= ring(11, 11)
    conc[4:11, 4:11] |= ring(7, 7)
    blocks = np.zeros((8, 14), bool)                     # 2x2 blocks and isolated pixels beside real starts
    blocks[0:2, 0:2] = blocks[3:5, 3:5] = blocks[0:2, 6:8] = True
    blocks[0, 10] = blocks[2, 12] = blocks[5, 0] = blocks[7, 8] = True
    blocks[4:8, 10:14] = ring(4, 4)
    return [ring(9, 7), ring(20, 3), diamond(4), diamond(9), conc, two, inner, plus(5), cross(5), cross(2), wheel(), checker(9), checker(16), blocks,
            line(9, 1, 0), line(9, 0, 1), line(9, 1, 1), line(9, -1, 1)]


def _repass_pieces():
    # the start pixel with dead-end arms: SW and SE (passed again between them), SW and E; E alone and SE alone for comparison; arms from a later pixel
    return [arms((5, 7)), arms((5, 0)), arms((0,)), arms((7,)), arms((5, 7, 0), 4), arms((1, 3, 5, 7, 0), 4), arms((0, 5, 6), 5)]


def _comb_pieces(fmt):
    res = [comb(list(range(14, 3, -1))), comb(list(range(30, 20, -1)), 3)]
    for pitch in (2, 3):                                   # mirrored: the proof lies backwards, 9, 10 and 11 evaluations away among others
        res.append(comb(list(range(8, 1, -1)), pitch, mirror=True))
    res += [span(3, 12), span(20, 60), span(40, 200)]      # forward proof in the first pass, in generation 1 and in generation 2
    if fmt == "sheet":
        res.append(span(150, 240))                         # generation 3 (about 540 steps)
    else:
        res += [span(60, 500), span(70, 900), span(85, 1000)]      # generation 3 and generation 4 (more than 960 steps)
    res += [span_for(fwd, 0, h) for fwd, h in HANDOVER_PROOFS[fmt]]
    return res


def _hole_comb_pieces(fmt):
    # drawn as the clear pixels; cut_out() turns them into holes. Clear tines rising from a clear base row, a wall of one, two or three pixels between
    # two tines: every tine top is a hole start candidate, one of them the trigger. As drawn the proofs lie forwards, mirrored backwards (9, 10 and 11
    # evaluations away among others). Then slots on the trigger's own row, and the spans for the generations.
    res = [comb(list(range(2, 12)), pitch, mirror=m) for pitch in (2, 3, 4) for m in (False, True)]
    res += [row_slots((3, 2, 4, 1, 3), 1), row_slots((2, 2, 2, 2), 2), span(3, 12), span(20, 60), span(40, 200)]
    if fmt == "sheet":
        res.append(span(150, 240))
    else:
        res += [span(60, 500), span(70, 900), span(85, 1000)]
    res += [span_for(fwd, 1, h) for fwd, h in HANDOVER_PROOFS[fmt]]
    return res


def _reach_pieces():
    # straight lines with n == 2 * reach at max_contour - 2 (kept) and max_contour (dropped): 1-px lines of 128 and 129 pixels in all four directions,
    # and the same cut out (their hole borders have 2 k + 2 points: k = 126 and 127 give 254 and 256)
    res = []
    for k in (128, 129):
        res += [line(k, 1, 0), line(k, 0, 1), line(k, 1, 1), line(k, -1, 1)]
    for k in (126, 127):
        res += [cut_out(line(k, 1, 0)), cut_out(line(k, 0, 1))]
    return res


_cache = {}


def family(name):
    """-> [(format, image uint8 0/255)]"""
    if name in _cache:
        return _cache[name]
    if name == "lengths":
        res = [("sheet", i) for i in _exact("sheet", SHEET_LENGTHS, lambda n: 120 if n > 200 else 40)]
        res += [("strip", i) for i in _exact("strip", STRIP_LENGTHS, lambda n: 330 if n > 2000 else 250 if n > 200 else 40)]
    elif name == "reach":
        res = [("reach", i) for i in pack("reach", _reach_pieces())]
    elif name == "repass":
        res = [("sheet", i) for i in pack("sheet", both(_repass_pieces()))]
    elif name == "combs":
        res = [("sheet", i) for i in pack("sheet", _comb_pieces("sheet"))] + [("strip", i) for i in pack("strip", _comb_pieces("strip"))]
    elif name == "hole_combs":
        res = [("sheet", i) for i in pack("sheet", [cut_out(p) for p in _hole_comb_pieces("sheet")])]
        res += [("strip", i) for i in pack("strip", [cut_out(p) for p in _hole_comb_pieces("strip")])]
    elif name == "thin":
        res = [("sheet", i) for i in pack("sheet", both(_thin_pieces()))] + [("odd", i) for i in pack("odd", both(_thin_pieces()), 1, 1)]
    elif name == "frame":
        res = [(f, i) for f in ("sheet", "odd", "strip") for i in _frame_images(f)]
    elif name == "grid":
        res = [("sheet", i) for i in _grid_images("sheet")]
    elif name == "noise":
        res = [("sheet", _noise("sheet", 0.5, 11)[0]), ("sheet", _noise("sheet", 0.45, 12)[0]), ("odd", _noise("odd", 0.5, 13)[0]),
               ("strip", _noise("strip", 0.5, 14)[0])]
    else:
        raise KeyError(name)
    _cache[name] = res
    return res


# Every designed family tells some misreading from the right reading (tests/test_border_edges_cpu.py prints which). What each is on the device for:
#   lengths     the size filter's bounds; the hand-over of a walk's state and checkpoint ring at 64, 192, 448, 960, 1984, 3008 and 4032 steps; n % 16 in
#               {15, 0, 1} (ncp = (n + 15) / 16, the last stretch of contour_quad's emission)
#   reach       the early exit at a chunk start
#   repass      closure only with the first neighbour as the next pixel (a start passed twice)
#   combs, hole_combs   false starts that die in the probe (9 and 10 evaluations back, and one that survives it at 11), in the first pass and in
#               generations 1, 2, 3 and 4 or later; each of the hole rule's W, E and N comparisons as a proof on its own
#   thin        pixels passed 2, 3 and 4 times, borders that share pixels, corner contacts, isolated pixels beside real starts (drop_single)
#   frame       the cleared frame, starts and triggers in the first and last rows and columns the scan sees, blocks clamped to the image
#   grid        the segment pipeline's waypoints: borders with none but their start, borders along grid lines
#   noise       bulk: dealt windows of candidates_sparse_kernel, full walker waves, generation lists with hundreds of entries
FAMILIES = ("lengths", "reach", "repass", "combs", "hole_combs", "thin", "frame", "grid", "noise")


def all_cases():
    """-> [(family, index, format, image)]"""
    return [(f, i, fmt, img) for f in FAMILIES for i, (fmt, img) in enumerate(family(f))]
