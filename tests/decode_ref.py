"""A plain float64 / integer restatement of the decode stage (aruco_amd/csrc/k_decode.hip, decode_device.h) and the seeded generators of its edge
families. Nothing here is tuned to the kernels: the homography follows homography_lane's operation order in Python floats (no contraction), the
warp is cv::warpPerspective's INTER_NEAREST as the oracle states it (IEEE division, clamp to the int range, round-half-even, BORDER_CONSTANT 0),
the histogram is np.bincount, Otsu is the sequential getThreshVal_Otsu_8u, the votes are FiducidalMarkers::detect's and HighlyReliableMarkers::detect's.
test_decode_edges_cpu.py holds all of it to the oracle and asserts what makes each family an edge case; test_gpu_decode_edges.py holds the kernels to it."""
import functools

import numpy as np

INT_MIN, INT_MAX = -2147483648.0, 2147483647.0
FLT_EPSILON = float(np.finfo(np.float32).eps)
WORDS = ((1, 0, 0, 0, 0), (1, 0, 1, 1, 1), (0, 1, 0, 0, 1), (0, 1, 1, 1, 0))
GUARD = 1e-6          # warp_gather's exact path is taken within this distance of a rounding boundary
RCP_ERROR = 2.4e-4    # error of v_rcp_f64 alone (2^-24 relative) at coordinate 4000: what the Newton step removes


# ---------------------------------------------------------------------------------------------------------------------------------------
# the stage, restated
# ---------------------------------------------------------------------------------------------------------------------------------------
def homography(quad, ws):
    """iM (9 Python floats) of homography_lane: cv::getPerspectiveTransform(quad -> patch corners) by Gaussian elimination with partial pivoting,
    then the adjugate inverse cv::warpPerspective starts with. A singular system gives zeros."""
    d = float(np.float32(ws - 1))
    dxs, dys = (0.0, d, d, 0.0), (0.0, 0.0, d, d)
    A = [[0.0] * 8 for _ in range(8)]
    b = [0.0] * 8
    for i in range(4):
        sx, sy = float(np.float32(quad[i][0])), float(np.float32(quad[i][1]))
        dx, dy = dxs[i], dys[i]
        A[i][0] = A[i + 4][3] = sx
        A[i][1] = A[i + 4][4] = sy
        A[i][2] = A[i + 4][5] = 1.0
        A[i][6], A[i][7] = -sx * dx, -sy * dx
        A[i + 4][6], A[i + 4][7] = -sx * dy, -sy * dy
        b[i], b[i + 4] = dx, dy
    ok = True
    for c in range(8):
        piv, best = c, abs(A[c][c])
        for r in range(c + 1, 8):
            if abs(A[r][c]) > best:
                best, piv = abs(A[r][c]), r
        if best == 0:
            ok = False
            break
        if piv != c:
            A[c], A[piv] = A[piv], A[c]
            b[c], b[piv] = b[piv], b[c]
        inv = 1.0 / A[c][c]
        for r in range(c + 1, 8):
            f = A[r][c] * inv
            if f == 0:
                continue
            Ar, Ac = A[r], A[c]
            for k in range(c, 8):
                Ar[k] -= f * Ac[k]
            b[r] -= f * b[c]
    if ok:
        for r in range(7, -1, -1):
            s = b[r]
            for k in range(r + 1, 8):
                s -= A[r][k] * b[k]
            b[r] = s / A[r][r]
        m = b + [1.0]
    else:
        m = [0.0] * 8 + [1.0]
    det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6])
    det = 1.0 / det if det != 0 else 0.0
    return [(m[4] * m[8] - m[5] * m[7]) * det, (m[2] * m[7] - m[1] * m[8]) * det, (m[1] * m[5] - m[2] * m[4]) * det,
            (m[5] * m[6] - m[3] * m[8]) * det, (m[0] * m[8] - m[2] * m[6]) * det, (m[2] * m[3] - m[0] * m[5]) * det,
            (m[3] * m[7] - m[4] * m[6]) * det, (m[1] * m[6] - m[0] * m[7]) * det, (m[0] * m[4] - m[1] * m[3]) * det]


def sample_positions(iM, ws):
    """(fX, fY) of every patch pixel [ws][ws], float64, as cv::warpPerspective forms them: every product and sum rounded on its own."""
    iM = [np.float64(v) for v in iM]
    y = np.arange(ws, dtype=np.float64)[:, None]
    x = np.arange(ws, dtype=np.float64)[None, :]
    X0, Y0, W0 = iM[1] * y + iM[2], iM[4] * y + iM[5], iM[7] * y + iM[8]
    Wq = W0 + iM[6] * x
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        Wd = np.where(Wq != 0, 1.0 / np.where(Wq != 0, Wq, 1.0), 0.0)
        fX = np.maximum(INT_MIN, np.minimum(INT_MAX, (X0 + iM[0] * x) * Wd))
        fY = np.maximum(INT_MIN, np.minimum(INT_MAX, (Y0 + iM[3] * x) * Wd))
    return fX, fY


def warp(frame, quad, ws, iM=None):
    """The canonical patch [ws][ws] of `quad` from `frame` [H][W] (nearest neighbour, round-half-even, 0 outside the frame)."""
    fX, fY = sample_positions(homography(quad, ws) if iM is None else iM, ws)
    assert np.isfinite(fX).all() and np.isfinite(fY).all()
    X, Y = np.rint(fX).astype(np.int64), np.rint(fY).astype(np.int64)
    H, W = frame.shape
    inside = (X >= 0) & (X < W) & (Y >= 0) & (Y < H)
    out = np.zeros((ws, ws), np.uint8)
    out[inside] = frame[Y[inside], X[inside]]
    return out


def histogram(patch):
    return np.bincount(np.asarray(patch, np.uint8).reshape(-1), minlength=256)


def otsu(patch):
    """getThreshVal_Otsu_8u: one sequential sweep in double."""
    hist = histogram(patch)
    n = int(hist.sum())
    scale = 1.0 / n
    mu = 0.0
    for i in range(256):
        mu += i * float(hist[i])
    mu *= scale
    mu1 = q1 = max_sigma = max_val = 0.0
    for i in range(256):
        p_i = float(hist[i]) * scale
        mu1 *= q1
        q1 += p_i
        q2 = 1.0 - q1
        if min(q1, q2) < FLT_EPSILON or max(q1, q2) > 1.0 - FLT_EPSILON:
            continue
        mu1 = (mu1 + i * p_i) / q1
        mu2 = (mu - q1 * mu1) / q2
        sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2)
        if sigma > max_sigma:
            max_sigma, max_val = sigma, float(i)
    return int(max_val)


def cell_blocks(patch, grid, first=0, count=None):
    """The pixels of the cells of a grid x grid division of the patch (cell side ws // grid): [count][count][cell * cell] for cells first..first+count."""
    ws = patch.shape[0]
    cell = ws // grid
    count = grid if count is None else count
    p = patch[first * cell:(first + count) * cell, first * cell:(first + count) * cell]
    return p.reshape(count, cell, count, cell).transpose(0, 2, 1, 3).reshape(count, count, cell * cell)


def cell_counts(patch, thr, grid=7, first=0, count=None):
    return (cell_blocks(patch, grid, first, count).astype(np.int32) > thr).sum(axis=2)


def cell_votes(patch, thr, grid=7, first=0, count=None):
    """more than half of the cell's pixels exceed thr"""
    cell = patch.shape[0] // grid
    return cell_counts(patch, thr, grid, first, count) > (cell * cell) // 2


def cell_medians(patch, grid=7, first=0, count=None):
    """the ((cell * cell) // 2 + 1)-th largest pixel of every cell: the vote is `median > thr`"""
    b = np.sort(cell_blocks(patch, grid, first, count), axis=2)[:, :, ::-1]
    return b[:, :, (b.shape[2] // 2 + 1) - 1]


_ROW_DIST = {row: min(sum(a != b for a, b in zip(row, w)) for w in WORDS) for row in [tuple((v >> k) & 1 for k in range(5)) for v in range(32)]}


def hamm_dist(bits):
    return sum(_ROW_DIST[tuple(int(b) for b in row)] for row in bits)


def rotate(bits):
    """FiducidalMarkers::rotate: out[i][j] = in[4 - j][i]"""
    n = len(bits)
    return [[bits[n - j - 1][i] for j in range(n)] for i in range(n)]


def fiducial_decode(votes):
    """FiducidalMarkers::detect on the 7 x 7 votes: (id, nRotations), id -1 when a border cell is white or no rotation has distance 0."""
    v = np.asarray(votes, bool)
    border = np.ones((7, 7), bool)
    border[1:6, 1:6] = False
    if (v & border).any():
        return -1, 0
    rot = [[[int(v[y + 1][x + 1]) for x in range(5)] for y in range(5)]]
    for _ in range(3):
        rot.append(rotate(rot[-1]))
    dists = [hamm_dist(r) for r in rot]
    nrot = 0
    for r in range(1, 4):
        if dists[r] < dists[nrot]:
            nrot = r
    if dists[nrot] != 0:
        return -1, nrot
    b = rot[nrot]
    return sum(((b[y][1] << 1) | b[y][3]) << (2 * (4 - y)) for y in range(5)), nrot


def fiducial_detect(patch):
    thr = otsu(patch)
    return fiducial_decode(cell_votes(patch, thr))


def hrm_rotations(votes):
    """the code of n x n votes in its four rotations, bit y * n + x: r = 1 puts (y, x) at (x, n - y - 1), r = 2 at (n - y - 1, n - x - 1), r = 3 at (n - x - 1, y)"""
    n = len(votes)
    rot = [0, 0, 0, 0]
    for y in range(n):
        for x in range(n):
            if votes[y][x]:
                for r, (ry, rx) in enumerate(((y, x), (x, n - y - 1), (n - y - 1, n - x - 1), (n - x - 1, y))):
                    rot[r] |= 1 << (ry * n + rx)
    return rot


def hrm_decode(patch, thr, n, codes, correction):
    """hrm_decode_kernel's rule: inner cells (side ws // (n + 2)) by majority, nearest entry over the four rotations, first minimum over entries and then
    rotations, accepted within `correction`: (entry, nRotations) or (-1, 0)."""
    votes = cell_votes(patch, thr, grid=n + 2, first=1, count=n)
    rot = hrm_rotations(votes)
    best = None
    for i, c in enumerate(codes):
        dm, rm = n * n, 0
        for r in range(4):
            hd = bin(int(c) ^ rot[r]).count("1")
            if hd < dm:
                dm, rm = hd, r
        if dm < n * n and (best is None or dm < best[0]):
            best = (dm, i, rm)
    if best is None or best[0] > correction:
        return -1, 0
    return best[1], best[2]


def hrm_correction(tau0, rate=1.0):
    return int(np.float32(rate) * np.float32((tau0 - 1) // 2))


def boundary_distance(fX, fY, frame):
    """Per patch sample, the distance of its source position from a rounding boundary (the nearer of x and y), counted only where the two source
    pixels on either side of that boundary lie in the frame and differ; inf elsewhere."""
    H, W = frame.shape
    out = np.full(fX.shape, np.inf)
    X, Y = np.rint(fX).astype(np.int64), np.rint(fY).astype(np.int64)
    for f, other, axis in ((fX, Y, 0), (fY, X, 1)):
        lo = np.floor(f).astype(np.int64)
        d = np.abs((f - np.floor(f)) - 0.5)
        if axis == 0:
            ok = (lo >= 0) & (lo + 1 < W) & (other >= 0) & (other < H)
            a = frame[np.clip(other, 0, H - 1), np.clip(lo, 0, W - 1)]
            b = frame[np.clip(other, 0, H - 1), np.clip(lo + 1, 0, W - 1)]
        else:
            ok = (lo >= 0) & (lo + 1 < H) & (other >= 0) & (other < W)
            a = frame[np.clip(lo, 0, H - 1), np.clip(other, 0, W - 1)]
            b = frame[np.clip(lo + 1, 0, H - 1), np.clip(other, 0, W - 1)]
        out = np.minimum(out, np.where(ok & (a != b), d, np.inf))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# patches and frames
# ---------------------------------------------------------------------------------------------------------------------------------------
def marker_bits(marker_id):
    """the 5 x 5 code of FiducidalMarkers::getMarkerMat: row y is the word that bits 2 * (4 - y) + 1, 2 * (4 - y) of the id select"""
    return [list(WORDS[(marker_id >> (2 * (4 - y))) & 3]) for y in range(5)]


def votes_patch(votes, ws, lo=40, hi=200):
    """a patch whose g x g cells (g = len(votes), side ws // g) are hi where the vote is set and lo elsewhere; what ws % g leaves over is lo"""
    g = len(votes)
    cell = ws // g
    p = np.full((ws, ws), lo, np.uint8)
    for y in range(g):
        for x in range(g):
            if votes[y][x]:
                p[y * cell:(y + 1) * cell, x * cell:(x + 1) * cell] = hi
    return p


def framed(bits):
    n = len(bits)
    v = [[0] * (n + 2) for _ in range(n + 2)]
    for y in range(n):
        for x in range(n):
            v[y + 1][x + 1] = int(bits[y][x])
    return v


def marker_patch(marker_id, rot=0, ws=56, lo=40, hi=200):
    """marker `marker_id` as the camera sees it after `rot` quarter turns: the decoder then reports nRotations that turn it back"""
    return votes_patch(np.rot90(np.array(framed(marker_bits(marker_id))), rot), ws, lo, hi)


@functools.lru_cache(maxsize=None)
def rotation_ties():
    """The 5 x 5 codes of the 1024 ids and of their one-bit neighbours whose best Hamming distance is reached by more than one rotation. Returns
    (codes, n_valid, n_neighbours): codes as 5 x 5 bit lists, valid ids first."""
    valid, near, seen = [], [], set()
    for marker_id in range(1024):
        base = marker_bits(marker_id)
        for flip in range(-1, 25):
            bits = [row[:] for row in base]
            if flip >= 0:
                bits[flip // 5][flip % 5] ^= 1
            key = tuple(map(tuple, bits))
            if key in seen:
                continue
            seen.add(key)
            rot = [bits]
            for _ in range(3):
                rot.append(rotate(rot[-1]))
            d = [hamm_dist(r) for r in rot]
            if d.count(min(d)) > 1:
                (valid if flip < 0 else near).append(bits)
    return valid + near, len(valid), len(near)


def cell_tie_patch(seed):
    """A 56 x 56 marker patch (id from the seed) of two touching noise clusters, ten of whose inner cells are ties relative to the patch's own Otsu
    threshold thr: a black cell has exactly 32 pixels above thr and its 33rd-largest pixel is thr itself, a white cell has exactly 33 above and
    its 33rd-largest is thr + 1. The fill moves thr, so every thr is tried until the patch's threshold is the one it was built for; seeds
    without such a thr are passed over. Returns (patch, marker id, tie cells)."""
    while True:
        rng = np.random.default_rng(seed)
        marker_id = int(rng.integers(0, 1024))
        votes = np.array(framed(marker_bits(marker_id)), bool)
        base = np.where(np.kron(votes, np.ones((8, 8), bool)), rng.integers(128, 226, (56, 56)), rng.integers(30, 128, (56, 56))).astype(np.uint8)
        cells = [(1 + int(c) // 5, 1 + int(c) % 5) for c in rng.permutation(25)[:10]]
        fills, perms = rng.random((10, 64)), [rng.permutation(64) for _ in range(10)]
        for thr in range(100, 160):
            p = base.copy()
            for k, (cy, cx) in enumerate(cells):
                hi = thr + 1 + np.floor(fills[k, :32] * (225 - thr))
                lo = 30 + np.floor(fills[k, 32:63] * (thr + 1 - 30))
                v = np.concatenate([hi, [thr + 1 if votes[cy, cx] else thr], lo]).astype(np.uint8)
                p[cy * 8:cy * 8 + 8, cx * 8:cx * 8 + 8] = v[perms[k]].reshape(8, 8)
            if otsu(p) == thr:
                return p, marker_id, cells
        seed += 1000


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def identity_quad(x0, y0, ws):
    s = ws - 1
    return [[x0, y0], [x0 + s, y0], [x0 + s, y0 + s], [x0, y0 + s]]


def paint(patches, ws, W, H, pitch=None, x_first=0, background=0):
    """The patches painted into one frame [H][W] on a grid (pitch ws + 1: x offsets alternate between even and odd), and the identity quads over them."""
    pitch = ws + 1 if pitch is None else pitch
    per_row = (W - x_first - ws) // pitch + 1
    assert len(patches) <= per_row * ((H - ws) // pitch + 1), "frame too small for the patches"
    frame = np.full((H, W), background, np.uint8)
    quads = []
    for i, p in enumerate(patches):
        x0, y0 = x_first + (i % per_row) * pitch, (i // per_row) * pitch
        frame[y0:y0 + ws, x0:x0 + ws] = p
        quads.append(identity_quad(x0, y0, ws))
    return frame, np.array(quads, np.int16)


def basic_patches(ws=56, seed=11):
    """(name, patch): uniform, one pixel that differs, two levels at extreme shares, every level, noise"""
    rng = np.random.default_rng(seed)
    n = ws * ws
    out = [("uniform_%d" % v, np.full((ws, ws), v, np.uint8)) for v in (0, 128, 255)]
    for base, other, where in ((0, 255, 0), (255, 0, n - 1), (128, 129, n // 2), (7, 200, 3 * ws + 5)):
        p = np.full(n, base, np.uint8)
        p[where] = other
        out.append(("one_pixel_%d_in_%d" % (other, base), p.reshape(ws, ws)))
    for lo, hi in ((10, 12), (0, 255), (100, 180)):
        for share in (1, n // 2, n - 1):
            p = np.full(n, lo, np.uint8)
            p[rng.permutation(n)[:share]] = hi
            out.append(("two_levels_%d_%d_share_%d" % (lo, hi, share), p.reshape(ws, ws)))
    ramp = (np.arange(n) * 256 // n).astype(np.uint8)
    out.append(("ramp", ramp.reshape(ws, ws)))
    out.append(("ramp_shuffled", rng.permutation(ramp).reshape(ws, ws)))
    out.append(("ramp_columns", np.ascontiguousarray(ramp.reshape(ws, ws).T)))
    for k in range(3):
        out.append(("noise_%d" % k, rng.integers(0, 256, (ws, ws), dtype=np.uint8)))
    out.append(("noise_low_bits", rng.integers(0, 4, (ws, ws), dtype=np.uint8)))
    out.append(("noise_high", rng.integers(250, 256, (ws, ws), dtype=np.uint8)))
    return out


def marker_patches():
    """(name, patch) at 56 x 56: 64 ids in four rotations, one-bit errors, one white border cell in each of the 24 positions, the rotation ties"""
    rng = np.random.default_rng(5)
    ids = sorted({0, 1, 2, 3, 341, 682, 1023, 512} | {int(v) for v in rng.integers(0, 1024, 80)})[:64]
    out = [("id%d_rot%d" % (i, r), marker_patch(i, r)) for i in ids for r in range(4)]
    for k, i in enumerate(ids[:25]):
        bits = marker_bits(i)
        bits[k // 5][k % 5] ^= 1
        out.append(("id%d_flip%d" % (i, k), votes_patch(np.rot90(np.array(framed(bits)), k % 4), 56)))
    border = [(y, x) for y in range(7) for x in range(7) if y in (0, 6) or x in (0, 6)]
    for k, (y, x) in enumerate(border):
        v = framed(marker_bits(ids[k]))
        v[y][x] = 1
        out.append(("id%d_border_%d_%d" % (ids[k], y, x), votes_patch(v, 56)))
    ties, _, _ = rotation_ties()
    for k, bits in enumerate(ties[:40]):
        out.append(("rotation_tie_%d" % k, votes_patch(framed(bits), 56)))
    return out


def marker_dictionary(extra=40, seed=9):
    """a 5 x 5 dictionary for the third kernel path: the inner codes of some painted markers and random codes; (n, codes, tau0)"""
    rng = np.random.default_rng(seed)
    codes = []
    for name, p in marker_patches()[:64:3]:
        codes.append(hrm_rotations(cell_votes(p, 100, 7, 1, 5))[0])
    codes += [int(v) for v in rng.integers(0, 1 << 25, extra)]
    return 5, codes, 5


# ---------------------------------------------------------------------------------------------------------------------------------------
# quad families on a noise frame
# ---------------------------------------------------------------------------------------------------------------------------------------
WIDE = (4096, 256)     # W, H of the wide, low frame


@functools.lru_cache(maxsize=None)
def wide_noise(seed=3):
    f = noise((WIDE[1], WIDE[0]), seed)
    f.setflags(write=False)
    return f


def edge_quads(W, H, s=55):
    """(name, quad): corners on the frame's first and last columns and rows, outside on every side, wholly outside"""
    out = []
    for name, (x0, y0) in {"col0_row0": (0, 0), "colW1_row0": (W - 1 - s, 0), "col0_rowH1": (0, H - 1 - s), "colW1_rowH1": (W - 1 - s, H - 1 - s),
                           "left_out": (-20, 40), "right_out": (W - 30, 40), "top_out": (300, -25), "bottom_out": (300, H - 31),
                           "corner_out": (-13, -17), "far_corner_out": (W - 9, H - 11), "one_past_right": (W - s, 10), "one_past_bottom": (10, H - s),
                           "wholly_left": (-200, 50), "wholly_right": (W + 10, 50), "wholly_above": (500, -300), "wholly_below": (500, H + 5),
                           "int16_min": (-32768, -32768), "int16_max": (32767 - s, 32767 - s)}.items():
        out.append((name, identity_quad(x0, y0, s + 1)))
    out.append(("tilted_over_left", [[-30, 20], [60, -10], [90, 120], [-5, 150]]))
    out.append(("tilted_over_right", [[W - 70, 30], [W + 40, 10], [W + 25, 140], [W - 90, 110]]))
    out.append(("over_all_sides", [[-50, -40], [W + 60, -30], [W + 10, H + 70], [-80, H + 20]]))
    out.append(("huge_outside", [[-30000, -30000], [30000, -29000], [31000, 30000], [-29000, 31000]]))
    return out


def extreme_quads(W, H, seed=21):
    rng = np.random.default_rng(seed)
    out = []
    for side in range(3, 11):
        x0, y0 = int(rng.integers(0, W - 12)), int(rng.integers(0, H - 12))
        out.append(("side_%d" % side, identity_quad(x0, y0, side + 1)))
        out.append(("side_%d_skew" % side, [[x0, y0], [x0 + side, y0 + 1], [x0 + side + 1, y0 + side], [x0 - 1, y0 + side - 1]]))
    out.append(("whole_frame", [[0, 0], [W - 1, 0], [W - 1, H - 1], [0, H - 1]]))
    out.append(("whole_frame_turned", [[W - 1, 0], [W - 1, H - 1], [0, H - 1], [0, 0]]))
    out.append(("whole_frame_mirrored", [[W - 1, 0], [0, 0], [0, H - 1], [W - 1, H - 1]]))
    for k, (near, far) in enumerate(((200, 20), (240, 24), (20, 200), (150, 15))):   # foreshortening: opposite sides in a ratio of ten
        x0 = 300 + 500 * k
        out.append(("foreshortened_%d" % k, [[x0, 128 - near // 2], [x0 + 300, 128 - far // 2], [x0 + 300, 128 + far // 2], [x0, 128 + near // 2]]))
        out.append(("foreshortened_%d_t" % k, [[x0 - near // 2 + 150, 10], [x0 + near // 2 + 150, 10], [x0 + far // 2 + 150, 240], [x0 - far // 2 + 150, 240]]))
    out.append(("sliver_h", [[100, 100], [3900, 101], [3900, 103], [100, 102]]))
    out.append(("sliver_v", [[2000, 2], [2002, 3], [2003, 250], [2001, 251]]))
    out.append(("sliver_diag", [[50, 10], [54, 11], [3950, 245], [3946, 244]]))
    out.append(("bowtie_x", [[500, 50], [700, 200], [700, 50], [500, 200]]))
    out.append(("bowtie_y", [[900, 40], [1100, 40], [900, 210], [1100, 210]]))
    out.append(("bowtie_narrow", [[1500, 100], [1700, 130], [1700, 100], [1500, 131]]))
    out.append(("two_equal_corners", [[300, 60], [300, 60], [420, 180], [290, 170]]))
    out.append(("opposite_equal", [[640, 60], [700, 90], [640, 60], [610, 130]]))
    out.append(("three_collinear", [[800, 50], [850, 100], [900, 150], [780, 160]]))
    out.append(("four_collinear", [[1000, 20], [1030, 50], [1060, 80], [1090, 110]]))
    out.append(("all_equal", [[1234, 123], [1234, 123], [1234, 123], [1234, 123]]))
    out.append(("concave", [[1300, 30], [1500, 40], [1390, 90], [1310, 220]]))
    return out


def random_quads(n, W, H, seed, lo=12, hi=300):
    """n seeded integer projective quads with sides of about lo..hi pixels, reaching a little over the frame's edges"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 4, 2), np.int64)
    for i in range(n):
        w, h = int(rng.integers(lo, hi + 1)), int(rng.integers(lo, min(hi, H) + 1))
        cx, cy = rng.integers(-10, W + 10 - w), rng.integers(-10, H + 10 - h)
        c = np.array([[cx, cy], [cx + w, cy], [cx + w, cy + h], [cx, cy + h]], np.int64)
        j = rng.integers(-(min(w, h) // 3), min(w, h) // 3 + 1, (4, 2))
        c = c + j
        out[i] = np.roll(c, int(rng.integers(0, 4)), axis=0)
    return out.astype(np.int16)


BANDS = ("exact", "inside_guard", "inside_rcp_error")


def band_of(d):
    return "exact" if d == 0 else "inside_guard" if d < GUARD else "inside_rcp_error" if d < RCP_ERROR else None


@functools.lru_cache(maxsize=None)
def near_boundary_quads(ws=56, want=20, seed=1234):
    """Seeded random projective quads on wide_noise() kept by the distance of their nearest (counted) sample from a rounding boundary: `want` with
    a sample exactly on one, `want` within (0, GUARD), `want` whose nearest lies in [GUARD, RCP_ERROR). Returns (quads, bands, searched)."""
    frame = wide_noise()
    W, H = WIDE
    kept = {b: [] for b in BANDS}
    searched = 0
    for rnd in range(40):
        for q in random_quads(1000, W, H, seed + rnd):
            searched += 1
            iM = homography(q, ws)
            fX, fY = sample_positions(iM, ws)
            if not (np.isfinite(fX).all() and np.isfinite(fY).all()):
                continue
            b = band_of(float(boundary_distance(fX, fY, frame).min()))
            if b is not None and len(kept[b]) < want:
                kept[b].append(q)
        if all(len(v) >= want for v in kept.values()):
            break
    quads = np.array([q for b in BANDS for q in kept[b]], np.int16)
    bands = [b for b in BANDS for _ in kept[b]]
    return quads, bands, searched


def count_quads(n, W, H, seed=77):
    """n different quads with sides of 20..120 pixels for the candidate-count family"""
    q = random_quads(2 * n, W, H, seed, 20, 120)
    _, first = np.unique(q.reshape(len(q), 8), axis=0, return_index=True)
    q = q[np.sort(first)][:n]
    assert len(q) == n
    return q


COUNTS = (1, 15, 16, 17, 47, 48, 49, 63, 64, 65, 383, 384, 385, 800)
WARP_SIZES = (10, 28, 55, 57, 63, 64, 88, 89, 96, 128)


def hrm_cases(seed=31):
    """(n, ws, codes, tau0, patches): dictionaries n = 2..8 at warp sizes where ws // (n + 2) leaves a remainder and where cell * cell is odd; patches
    of entries (entry 4095 among them where the dictionary is that long) at distance 0, exactly `correction` and `correction + 1`, turned."""
    rng = np.random.default_rng(seed)
    out = []
    for n, ws, count, tau0 in ((2, 10, 6, 1), (3, 28, 40, 3), (4, 57, 200, 5), (5, 63, 4096, 7), (6, 89, 300, 9), (7, 64, 4096, 11), (8, 96, 500, 15),
                               (5, 56, 100, 5), (8, 128, 64, 9)):
        nn = n * n
        codes = []
        while len(codes) < count:
            c = int.from_bytes(rng.bytes(8), "little") & ((1 << nn) - 1)
            if c not in codes:
                codes.append(c)
        corr = hrm_correction(tau0)
        patches = []
        for k, entry in enumerate([0, count // 2, count - 1] * 2):
            for dist in (0, corr, corr + 1):
                c = codes[entry]
                for bit in rng.permutation(nn)[:dist]:
                    c ^= 1 << int(bit)
                bits = [[(c >> (y * n + x)) & 1 for x in range(n)] for y in range(n)]
                p = votes_patch(np.rot90(np.array(framed(bits)), k % 4), ws, 30 + k, 220 - k)   # the cells turn, what ws % (n + 2) leaves over stays
                patches.append(("n%d_entry%d_dist%d_turn%d" % (n, entry, dist, k % 4), p))
        out.append((n, ws, codes, tau0, patches))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the case sets both test files run: name -> dict(ws, frame [H][W], quads int16 [n][4][2], names, hrm (n, codes, tau0) or None,
# painted: the patches under the first quads, which are identity quads, pad: bytes of row padding the device frame gets, kind: see paths_of)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _set(ws, frame, quads, names, hrm=None, painted=None, pad=0, kind="three_paths"):
    frame = np.ascontiguousarray(frame, np.uint8)
    frame.setflags(write=False)
    return {"ws": ws, "frame": frame, "quads": np.asarray(quads, np.int16).reshape(-1, 4, 2), "names": list(names), "hrm": hrm, "painted": painted, "pad": pad, "kind": kind}


def _warp_size_set(ws, seed):
    """a small frame for one warp size: painted uniform, noise, ramp and marker patches under identity quads, and projective, edge and singular quads"""
    rng = np.random.default_rng(seed)
    n = ws * ws
    flip = marker_bits(345)
    flip[2][2] ^= 1
    white_border = framed(marker_bits(77))
    white_border[6][3] = 1
    named = [("uniform_0", np.zeros((ws, ws), np.uint8)), ("uniform_255", np.full((ws, ws), 255, np.uint8)), ("uniform_77", np.full((ws, ws), 77, np.uint8)),
             ("noise_a", rng.integers(0, 256, (ws, ws), dtype=np.uint8)), ("noise_b", rng.integers(0, 256, (ws, ws), dtype=np.uint8)),
             ("ramp", (np.arange(n) * 256 // n).astype(np.uint8).reshape(ws, ws)), ("two_levels", np.where(rng.random((ws, ws)) < 0.5, 90, 92).astype(np.uint8))]
    named += [("id%d_rot%d" % (i, r), marker_patch(i, r, ws)) for i, r in ((345, 0), (1023, 1), (682, 2), (17, 3))]
    named += [("id345_flip", votes_patch(framed(flip), ws)), ("id77_white_border", votes_patch(white_border, ws))]
    W, H = 1024, 2 * (ws + 1) + 40
    frame, quads = paint([p for _, p in named], ws, W, H, background=0)
    free = frame == 0
    bg = noise((H, W), seed + 1)
    rows = np.zeros((H, W), bool)
    rows[2 * (ws + 1):] = True          # noise below the painted rows, so that the projective quads have something to sample
    frame = np.where(rows & free, bg, frame)
    extra = [("projective_%d" % k, q) for k, q in enumerate(random_quads(6, W, H, seed + 2, 12, 120))]
    extra += [("over_the_corner", identity_quad(-5, -7, ws)), ("past_the_far_corner", identity_quad(W - ws // 2, H - ws // 2, ws)),
              ("two_equal_corners", [[30, 30], [30, 30], [90, 110], [20, 100]]), ("whole_frame", [[0, 0], [W - 1, 0], [W - 1, H - 1], [0, H - 1]])]
    allq = np.concatenate([quads.reshape(-1, 4, 2), np.array([q for _, q in extra], np.int16).reshape(-1, 4, 2)])
    return _set(ws, frame, allq, [n_ for n_, _ in named] + [n_ for n_, _ in extra], painted=[p for _, p in named], kind="warp_size")


@functools.lru_cache(maxsize=None)
def case_sets():
    sets = {}
    W, H = WIDE
    basic = basic_patches()
    ties = [("cell_ties_%d" % s, cell_tie_patch(s)[0]) for s in range(6)]
    named = basic + ties
    frame, quads = paint([p for _, p in named], 56, W, H)
    sets["painted_basic"] = _set(56, frame, quads, [n for n, _ in named], hrm=marker_dictionary(), painted=[p for _, p in named])
    frame, quads = paint([p for _, p in named], 56, 4001, H, pitch=58, x_first=1, background=9)   # every x offset odd, an odd width, padded rows
    sets["painted_basic_padded"] = _set(56, frame, quads, [n for n, _ in named], hrm=marker_dictionary(), painted=[p for _, p in named], pad=39)
    named = marker_patches()
    frame, quads = paint([p for _, p in named], 56, W, 348)
    sets["painted_markers"] = _set(56, frame, quads, [n for n, _ in named], hrm=marker_dictionary(), painted=[p for _, p in named])
    for fam, named in (("frame_edges", edge_quads(W, H)), ("extreme_quads", extreme_quads(W, H))):
        sets[fam] = _set(56, wide_noise(), [q for _, q in named], [n for n, _ in named], hrm=marker_dictionary())
    q, bands, _ = near_boundary_quads()
    sets["near_boundary"] = _set(56, wide_noise(), q, ["%s_%d" % (b, i) for i, b in enumerate(bands)], hrm=marker_dictionary())
    for ws in WARP_SIZES:
        sets["warp_size_%d" % ws] = _warp_size_set(ws, 100 + ws)
    for n, ws, codes, tau0, named in hrm_cases():
        per_row = 1024 // (ws + 1)
        frame, quads = paint([p for _, p in named], ws, 1024, (ws + 1) * ((len(named) + per_row - 1) // per_row) + 8, background=0)
        sets["hrm_n%d_ws%d" % (n, ws)] = _set(ws, frame, quads, [n_ for n_, _ in named], hrm=(n, codes, tau0), painted=[p for _, p in named], kind="dictionary")
    return sets


def paths_of(s):
    """the kernel paths a set runs on: (path name, frames in the call, dictionary or None)"""
    if s["kind"] == "three_paths":
        return [("one_frame", 1, None), ("three_frames", 3, None), ("three_frames_dictionary", 3, s["hrm"])]
    if s["kind"] == "dictionary":
        return [("one_frame_dictionary", 1, s["hrm"]), ("three_frames_dictionary", 3, s["hrm"])]
    return [("one_frame", 1, None), ("three_frames", 3, None)]


def device_frames(s, nframes):
    """the frames of a call: nframes copies of the set's frame, with the set's row padding filled with a value no frame pixel needs"""
    H, W = s["frame"].shape
    f = np.full((nframes, H, W + s["pad"]), 0xA5, np.uint8)
    f[:, :, :W] = s["frame"]
    return f, W
