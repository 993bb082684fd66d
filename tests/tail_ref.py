"""The marker-list tail of MarkerDetector::detect (src/markerdetector.cpp:371-382, 417-447) in plain Python / numpy, line by line, and the
cases test_tail_cpu.py and test_gpu_tail_edges.py share. No device code.

finalize() is the reference's tail on one frame's decoded candidates; tail() adds what this project puts around it: the marker rows'
capacity, the overflow bit, frames given up because a threshold plane carries a status bit, the write-through rows, the one-frame header
and the flat marker list."""
import itertools

import numpy as np

from tests.recover_ref import border_rect

ST_MARKER_OVERFLOW = 32
FILL = 0xA5                      # the byte arucohip_debug_marker_tail fills the marker rows with
HALFWAY_SIZES = ((100, 60), (180, 100), (300, 140))   # W * 0.025 or H * 0.025 (and the far side) is a float32 half-way product
F32 = np.float32


def perimeter(c):
    """utils.h:39-46: a float sum of double norms of float differences."""
    c = np.asarray(c, F32).reshape(4, 2)
    s = F32(0)
    for i in range(4):
        j = (i + 1) % 4
        dx, dy = F32(c[i, 0] - c[j, 0]), F32(c[i, 1] - c[j, 1])
        s = F32(np.float64(s) + np.sqrt(np.float64(dx) * np.float64(dx) + np.float64(dy) * np.float64(dy)))
    return s


def perimeter64(c):
    """What the reference does NOT compute: the same norms summed in double."""
    c = np.asarray(c, F32).reshape(4, 2)
    s = np.float64(0)
    for i in range(4):
        j = (i + 1) % 4
        dx, dy = F32(c[i, 0] - c[j, 0]), F32(c[i, 1] - c[j, 1])
        s = s + np.sqrt(np.float64(dx) * np.float64(dx) + np.float64(dy) * np.float64(dy))
    return s


def inside(c, rect):
    """:433-444: Rect::contains(Point(corner)) of every corner; Point2f -> Point rounds half to even, the bounds are half open."""
    x0, y0, x1, y1 = rect
    for x, y in np.asarray(c, F32).reshape(4, 2):
        px, py = int(np.rint(x)), int(np.rint(y))
        if not (x0 <= px < x1 and y0 <= py < y1):
            return False
    return True


def finalize(ids, corners, rect, perimeter=perimeter):
    """The candidate indices the tail keeps, in the order it returns them."""
    ids = [int(i) for i in ids]
    corners = np.asarray(corners, F32).reshape(len(ids), 8)
    det = [i for i in range(len(ids)) if ids[i] != -1]                 # :375-382
    det.sort(key=lambda i: ids[i])                                     # :417; Python's sort is stable: equal ids keep candidate order
    rem = [False] * len(det)
    for i in range(len(det) - 1):                                      # :422-430
        if ids[det[i]] == ids[det[i + 1]] and not rem[i + 1]:
            if perimeter(corners[det[i]]) > perimeter(corners[det[i + 1]]):
                rem[i + 1] = True
            else:
                rem[i] = True
    for i in range(len(det)):                                          # :436-444
        if not inside(corners[det[i]], rect):
            rem[i] = True
    return [det[i] for i in range(len(det)) if not rem[i]]             # :447


def tail(frames, width, height, cap_markers, border_dist=0.025, out_cap=None, plane_status=None):
    """frames: [(ids, corners)] per frame. Returns a dict:
    kept [f]: candidate indices finalize() keeps; n [f]: their number, -1 for a frame given up; rows [f]: the candidate indices whose
    markers fill the frame's first rows (None for a frame given up: what its rows hold is not defined); status: the batch's status bits;
    list: the set of flat list entries; out_rows [f] (with out_cap): the candidate indices written through; hdr: (n, status) of a one-frame call."""
    rect = border_rect(width, height, border_dist)
    nf = len(frames)
    ps = np.zeros((nf, 1), np.uint32) if plane_status is None else np.asarray(plane_status, np.uint32).reshape(nf, -1)
    res = {"kept": [], "n": [], "rows": [], "status": int(np.bitwise_or.reduce(ps.reshape(-1))), "list": set(), "out_rows": [], "rect": rect}
    for f, (ids, corners) in enumerate(frames):
        kept = finalize(ids, corners, rect)
        res["kept"].append(kept)
        if len(kept) > cap_markers:
            res["status"] |= ST_MARKER_OVERFLOW
        dead = bool(ps[f].any())
        res["n"].append(-1 if dead else len(kept))
        res["rows"].append(None if dead else kept[:cap_markers])
        res["out_rows"].append(None if dead or out_cap is None else kept[:min(cap_markers, out_cap)])
        if not dead:
            res["list"] |= {(f << 16) | i for i in range(min(len(kept), cap_markers))}
    res["hdr"] = (res["n"][0], res["status"]) if nf == 1 else None
    return res


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
W, H = 640, 480                  # rectangle [16, 624) x [12, 468)


def square(x, y, side):
    """An axis-parallel square of perimeter 4 * side (exact for the sides used here)."""
    return np.array([x, y, x + side, y, x + side, y + side, x, y + side], F32)


# name -> (perimeters of a run of equal ids in candidate order, a negative one lies outside the border rectangle), and the positions in the
# run that survive, worked out by hand from :422-447
CHAINS = {
    "single": ((8,), [0]),
    "pair_first_larger": ((10, 5), [0]),
    "pair_second_larger": ((5, 10), [1]),
    "pair_tie": ((6, 6), [1]),                  # > is strict: the earlier one goes
    "triple_tie": ((6, 6, 6), [2]),
    "triple_10_5_7": ((10, 5, 7), [0, 2]),      # 5 is removed by 10; 7 is compared with the removed 5 and stays: two markers of one id
    "triple_rising": ((5, 7, 10), [2]),
    "triple_falling": ((10, 7, 5), [0]),
    "four_5_10_7_8": ((5, 10, 7, 8), [1, 3]),
    "four_falling": ((10, 9, 8, 7), [0]),
    "four_rising": ((7, 8, 9, 10), [3]),
    "four_10_5_7_6": ((10, 5, 7, 6), [0, 2]),   # 6 loses to 7, which had survived next to the removed 5
    "four_ties": ((6, 6, 7, 7), [3]),
    "winner_outside": ((-10, 5), []),           # the dedupe runs first: 5 loses to 10, then the border filter drops 10
    "loser_outside": ((10, -5), [0]),
    "triple_middle_outside": ((5, -10, 7), []),    # 5 < 10: 5 goes; 10 > 7: 7 goes; 10 lies outside: nothing is left
}


def chain_frame(names=None):
    """One frame that holds every chain case under an id of its own, the runs interleaved round robin with undecoded candidates between
    them. Returns ids, corners [n][8] and {name: candidate indices of the run's members in run order}."""
    names = sorted(CHAINS) if names is None else names
    ids, corners, members = [], [], {k: [] for k in names}
    depth = max(len(CHAINS[k][0]) for k in names)
    for level in range(depth):
        for ci, k in enumerate(names):
            per = CHAINS[k][0]
            if level >= len(per):
                continue
            side = abs(per[level]) / 4.0
            x = 20.0 + 36.0 * ci if per[level] > 0 else 2.0          # x = 2 rounds to a pixel left of the rectangle
            members[k].append(len(ids))
            ids.append(100 + 7 * ci)
            corners.append(square(x, 20.0 + 8.0 * level, side))
            if (ci + level) % 3 == 0:
                ids.append(-1)
                corners.append(square(300.0, 300.0, 4.0))
    return np.array(ids, np.int32), np.array(corners, F32), members


def near_tie_pairs(count=32, seed=5):
    """`count` pairs of equal ids (ids 2 k, one pair each) whose float32 perimeters tie or differ by an ulp or so: quad B is quad A moved by a
    whole number of pixels, which changes the rounding of its coordinates and nothing else. Half of the pairs are chosen so that summing the
    norms in double would decide the pair differently. Returns ids, corners [2 count][8] and the indices of the pairs that disagree."""
    rng = np.random.RandomState(seed)
    agree, differ = [], []
    while len(agree) < count or len(differ) < count // 2:
        a = (rng.uniform(30, 100, (4, 2)) + np.array([[0, 0], [150, 0], [150, 150], [0, 150]])).astype(F32)
        b = (a + F32(rng.randint(1, 3) * 64)).astype(F32)
        if rng.randint(2):
            a, b = b, a
        d32, d64 = perimeter(a) > perimeter(b), perimeter64(a) > perimeter64(b)
        (differ if d32 != d64 else agree).append((a, b))
    differ = differ[:count // 2]
    pairs, disagree = [], []
    for k in range(count):                                             # the disagreeing pairs at the even places
        if k % 2 == 0 and differ:
            disagree.append(k)
            pairs.append(differ.pop())
        else:
            pairs.append(agree.pop())
    ids = np.repeat(np.arange(count, dtype=np.int32) * 2, 2)
    corners = np.array([q.reshape(8) for p in pairs for q in p], F32)
    return ids, corners, disagree


def random_quads(rng, n, width=W, height=H, border_dist=0.025):
    """n convex quads with float corners inside the border rectangle, perimeters all over the place"""
    x0, y0, x1, y1 = border_rect(width, height, border_dist)
    cx, cy = rng.uniform(x0 + 40, x1 - 41, n), rng.uniform(y0 + 40, y1 - 41, n)
    r = rng.uniform(3, 38, n)
    ang = rng.uniform(0, 2 * np.pi, n)[:, None] + np.arange(4) * (np.pi / 2) + rng.uniform(-0.3, 0.3, (n, 4))
    q = np.stack([cx[:, None] + r[:, None] * np.cos(ang), cy[:, None] + r[:, None] * np.sin(ang)], 2)
    return q.reshape(n, 8).astype(F32)


BIG_IDS = (0, 1, 1023, 2 ** 31 - 1)


def order_frame(n, seed, distinct=False):
    """n candidates of one frame: every third or so undecoded (-1); ids from a small range with many repeats plus BIG_IDS, or all distinct."""
    rng = np.random.RandomState(seed)
    if distinct:
        ids = rng.choice(np.arange(2, 100000), n, replace=False)      # 0, 1, 1023 and 2^31 - 1 come in below
        ids = ids[ids != 1023] if n < 4 else np.where(ids == 1023, 1022, ids)
    else:
        ids = rng.choice(np.concatenate([np.arange(12), np.array(BIG_IDS)]), n)
    ids = np.where(rng.uniform(size=n) < 0.3, -1, ids).astype(np.int32)
    if n >= 4:
        ids[rng.choice(n, 4, replace=False)] = BIG_IDS                 # they are there whatever the draw
    return ids, random_quads(rng, n)


def border_probe(rect, where, value):
    """A 6-px square in the middle of `rect` with one corner's coordinate replaced: where = (corner, axis)."""
    x0, y0, x1, y1 = rect
    q = square((x0 + x1) // 2 - 3, (y0 + y1) // 2 - 3, 6.0).reshape(4, 2)
    q[where[0], where[1]] = value
    return q.reshape(8)


def border_values(lo, hi):
    """Coordinates around the bounds [lo, hi) of one axis: half-way values (ties to even), an ulp to either side, whole pixels, and the
    two small negative values that round to -0 and to 0."""
    out = []
    for b in (lo, hi):
        for base in (b - 0.5, b + 0.5):
            v = F32(base)
            out += [v, np.nextafter(v, F32(-1e9)), np.nextafter(v, F32(1e9))]
        out += [F32(b - 1), F32(b), F32(b + 1)]
    out += [F32(-0.5), F32(-0.49), F32(0.5), F32(0.0)]
    return [F32(v) for v in out]


def border_frame(width, height, border_dist=0.025):
    """Every border_values() coordinate in x (corner 0 and corner 2) and in y, one candidate each, ids distinct and rising"""
    rect = border_rect(width, height, border_dist)
    corners = []
    for axis, (lo, hi) in ((0, (rect[0], rect[2])), (1, (rect[1], rect[3]))):
        for v in border_values(lo, hi):
            for corner in (0, 2):
                corners.append(border_probe(rect, (corner, axis), v))
    corners = np.array(corners, F32)
    return np.arange(len(corners), dtype=np.int32), corners


RECT_TABLE_SIZES = HALFWAY_SIZES + ((420, 220), (640, 480), (33, 47), (1, 1))
RECT_TABLE_T = (0.0, 0.0125, 0.025, 0.5, 0.6)


def permutation_chains():
    """Every order of four distinct perimeters and of 10, 5, 7, 7 as a run of one id: (perimeters, corners [4][8])"""
    runs = sorted(set(itertools.permutations((5, 7, 8, 10))) | set(itertools.permutations((10, 5, 7, 7))))
    return [(p, np.array([square(30.0 + 12 * k, 40.0, s / 4.0) for k, s in enumerate(p)], F32)) for p in runs]


# ---- the oracle leg: one marker whose extreme corner is put on and next to each bound of the border rectangle ---------------------------
ORACLE_ID, ORACLE_CELL = 101, 5          # a 35-px marker: it fits the 60 rows of the smallest half-way size with room to move


def marker_frame(width, height, ax, ay, cell=ORACLE_CELL, mid=ORACLE_ID):
    """A light frame with marker `mid` drawn at whole pixels, its top-left pixel at (ax, ay)"""
    from aruco_amd import synth

    img = np.full((height, width), 230, np.uint8)
    side = 7 * cell
    assert 0 <= ax and ax + side <= width and 0 <= ay and ay + side <= height
    img[ay:ay + side, ax:ax + side] = np.kron(synth.marker_bits(mid), np.ones((cell, cell), np.uint8)) * 200 + 20
    return img


def oracle_leg(width, height, detect_corners, border_dist=0.025):
    """detect_corners(frame) -> the integer corners [4][2] the oracle gives the one marker with corner method NONE and NO border filter, or
    None. Returns None when the marker is not found at the centre of the frame, else a list of (name, frame): the marker centred, and its
    smallest / largest corner coordinate put on b0 - 1, b0, b1 - 1, b1 in x and in y (the other axis centred)."""
    x0, y0, x1, y1 = border_rect(width, height, border_dist)
    side = 7 * ORACLE_CELL
    cx, cy = (width - side) // 2, (height - side) // 2
    c = detect_corners(marker_frame(width, height, cx, cy))
    if c is None:
        return None
    c = np.asarray(c).reshape(4, 2)
    off = {"lo": (int(c[:, 0].min()) - cx, int(c[:, 1].min()) - cy), "hi": (int(c[:, 0].max()) - cx, int(c[:, 1].max()) - cy)}
    out = [("centre", marker_frame(width, height, cx, cy))]
    for axis, (b0, b1) in ((0, (x0, x1)), (1, (y0, y1))):
        for end, target in (("lo", b0 - 1), ("lo", b0), ("hi", b1 - 1), ("hi", b1)):
            a = target - off[end][axis]
            ax, ay = (a, cy) if axis == 0 else (cx, a)
            out.append(("%s %s corner on %d" % ("xy"[axis], end, target), marker_frame(width, height, ax, ay)))
    return out
