"""Float64 reference of the chessboard-corner (ChArUco) boards: the layout arithmetic, the board image, the interpolation of the inner
corners from a frame's markers up to the refinement's start (neighbours, start, window, frame border; include/arucohip.h states the
rules), and a renderer that gives the frames of the tests with the true position of every inner corner. Plain numpy; the refinement
itself is pixref.subpix. Test infrastructure: the library never imports it."""
import math

import numpy as np

from tests import fiducial_ref as fr

MAX_CORNERS, MAX_MARKERS, MAX_SIDE = 512, 1024, 16383
INV_SQRT2 = 0.70710678118654752
FRAGILE_MARGIN = 1e-4

# The worst distance between a refined corner (pixref.subpix from the reference start, true marker quads) and its true position over the
# frames of SCENES, as `pytest tests/test_charuco_cpu.py -k refined -s` prints it. For information only: nothing is held to it.
REFINED_WORST_PX = 0.194


# ---------------------------------------------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------------------------------------------
def board_size(L):
    """(width, height, markers, corners) of layout L = (squares_x, squares_y, square_px, marker_px); None outside the limits"""
    sx, sy, sq, mp = L
    if not (2 <= sx <= 64 and 2 <= sy <= 64) or mp < 7 or sq - mp < 2:
        return None
    W, H = sx * sq, sy * sq
    nm, nc = sx * sy // 2, (sx - 1) * (sy - 1)
    if W > MAX_SIDE or H > MAX_SIDE or nc > MAX_CORNERS or nm > MAX_MARKERS:
        return None
    return W, H, nm, nc


def white_squares(L):
    """(sx, sy) of the white squares in row-major order: marker k sits in the k-th"""
    return [(x, y) for y in range(L[1]) for x in range(L[0]) if (x + y) % 2 == 1]


def marker_quad(L, square):
    """board-pixel corners of the marker in a white square, in the corner order of arucohip_fiducial_board_image"""
    m = (L[2] - L[3]) // 2
    x0, y0 = square[0] * L[2] + m, square[1] * L[2] + m
    return np.array([[x0, y0], [x0 + L[3], y0], [x0 + L[3], y0 + L[3]], [x0, y0 + L[3]]], np.float64)


def corner_xy(L, c):
    ix, iy = c % (L[0] - 1), c // (L[0] - 1)
    return (ix + 1) * L[2], (iy + 1) * L[2]


def neighbours(L, c):
    """The two markers around corner c, in marker order: [(marker index, white square)]"""
    ix, iy = c % (L[0] - 1), c // (L[0] - 1)
    ws = white_squares(L)
    out = [(ws.index(s), s) for s in ((ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1)) if (s[0] + s[1]) % 2 == 1]
    assert len(out) == 2
    return sorted(out)


def board_image(L, ids):
    W, H, nm, _ = board_size(L)
    assert len(ids) == nm
    img = np.full((H, W), 255, np.uint8)
    for y in range(L[1]):
        for x in range(L[0]):
            if (x + y) % 2 == 0:
                img[y * L[2]:(y + 1) * L[2], x * L[2]:(x + 1) * L[2]] = 0
    for k, s in enumerate(white_squares(L)):
        q = marker_quad(L, s).astype(int)
        img[q[0, 1]:q[0, 1] + L[3], q[0, 0]:q[0, 0] + L[3]] = fr.marker_image(int(ids[k]), L[3])
    return img


def objects(L, centered=False):
    """(obj float32 [markers][4][3], corner_obj float32 [corners][3]) in board pixels"""
    W, H, nm, nc = board_size(L)
    shift = np.array([W // 2, H // 2], np.float64) if centered else np.zeros(2)
    obj = np.zeros((nm, 4, 3), np.float32)
    for k, s in enumerate(white_squares(L)):
        obj[k, :, :2] = marker_quad(L, s) - shift
    cobj = np.zeros((nc, 3), np.float32)
    for c in range(nc):
        cobj[c, :2] = np.array(corner_xy(L, c), np.float64) - shift
    return obj, cobj


# ---------------------------------------------------------------------------------------------------------------------------------
# interpolation, steps 1-4
# ---------------------------------------------------------------------------------------------------------------------------------
def homography4(src, dst):
    """the exact 4-point solve, float64: the 8 coefficients (h22 = 1), or None for a singular system"""
    A, b = np.zeros((8, 8)), np.zeros(8)
    for i in range(4):
        x, y, u, v = float(src[i][0]), float(src[i][1]), float(dst[i][0]), float(dst[i][1])
        A[i] = [x, y, 1, 0, 0, 0, -x * u, -y * u]
        A[i + 4] = [0, 0, 0, x, y, 1, -x * v, -y * v]
        b[i], b[i + 4] = u, v
    try:
        return np.linalg.solve(A, b)
    except np.linalg.LinAlgError:
        return None


def interpolate(L, ids, markers, W, H, min_markers=2, max_win=5):
    """markers: [(id, corners float32 [4][2])] of one frame, in the frame's order (None: a frame the batch gave up). Per corner a dict:
    found, markers, win, start (float64, unrounded) and start32 (what the device stores), fragile (window-fragile: a decision of step 3 or
    4 within FRAGILE_MARGIN of its threshold; such a corner may take the neighbouring value)."""
    out = []
    for c in range(board_size(L)[3]):
        X, Y = corner_xy(L, c)
        proj, corners = [], []
        for k, s in neighbours(L, c):
            hit = [m for m in (markers or []) if int(m[0]) == int(ids[k])]
            if not hit:
                continue
            q = np.asarray(hit[0][1], np.float32).reshape(4, 2).astype(np.float64)
            h = homography4(marker_quad(L, s), q)
            if h is None:
                continue
            w = h[6] * X + h[7] * Y + 1.0
            if not w > 0:
                continue
            proj.append(((h[0] * X + h[1] * Y + h[2]) / w, (h[3] * X + h[4] * Y + h[5]) / w))
            corners.append(q)
        r = {"found": False, "markers": len(proj), "win": 0, "start": np.zeros(2), "start32": np.zeros(2, np.float32), "fragile": False}
        if proj:
            r["start"] = np.array([sum(p[0] for p in proj) / len(proj), sum(p[1] for p in proj) / len(proj)])
            r["start32"] = r["start"].astype(np.float32)
        if proj and len(proj) >= min_markers:
            d = min(math.sqrt((r["start"][0] - p[0]) ** 2 + (r["start"][1] - p[1]) ** 2) for q in corners for p in q)
            v = d * INV_SQRT2
            wv = math.floor(v) - 1.0
            r["win"] = max_win if wv > max_win else int(wv)
            r["fragile"] = abs(v - round(v)) < FRAGILE_MARGIN
            lim = r["win"] + 1
            s32 = r["start32"].astype(np.float64)
            tests = [s32[0] - lim, (W - 1) - (s32[0] + lim), s32[1] - lim, (H - 1) - (s32[1] + lim)]
            r["found"] = r["win"] >= 2 and all(t >= 0 for t in tests)
            r["fragile"] = r["fragile"] or any(abs(t) < FRAGILE_MARGIN for t in tests)
        out.append(r)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# frames
# ---------------------------------------------------------------------------------------------------------------------------------
K = np.array([[600.0, 0.0, 320.0], [0.0, 600.0, 240.0], [0.0, 0.0, 1.0]])
W, H = 640, 480
UNIT = 0.001          # metres per board pixel
PAD = 40              # white sheet around the board, board pixels
BLACK, WHITE, GREY = 30.0, 225.0, 128.0
SS, STRIP = 6, 96     # sub-samples per pixel and axis of the renderer, rows painted at a time


def render(L, ids, rvec, tvec, seed=1, cover=(), noise=1.0, width=W, height=H, Kc=K):
    """The board on a white sheet of PAD pixels around it, seen through the pinhole camera Kc at (rvec, tvec) (board x right, y down, centred,
    UNIT metres per pixel) in a grey room. cover: marker indices hidden under a grey patch. Returns (frame uint8 [H][W], the true inner
    corners float64 [corners][2], the true marker quads float64 [markers][4][2])."""
    import torch
    from aruco_amd import synth

    Wb, Hb, nm, nc = board_size(L)
    tab = np.where(board_image(L, ids) > 0, WHITE, BLACK).astype(np.float32)
    for k in cover:
        q = marker_quad(L, white_squares(L)[k]).astype(int)
        tab[q[0, 1] - 2:q[2, 1] + 2, q[0, 0] - 2:q[2, 0] + 2] = GREY
    side = max(Wb, Hb) + 2 * PAD
    ox, oy = (side - Wb) // 2, (side - Hb) // 2
    sheet = np.full((side, side), WHITE, np.float32)
    sheet[oy:oy + Hb, ox:ox + Wb] = tab

    def to3(p):   # board pixels -> metres on the plane z = 0, centred
        p = np.asarray(p, np.float64).reshape(-1, 2)
        return np.concatenate([(p - np.array([Wb / 2.0, Hb / 2.0])) * UNIT, np.zeros((len(p), 1))], axis=1)

    x0, y0 = -ox, -oy
    quad = synth.project(Kc, rvec, tvec, to3([[x0, y0], [x0 + side, y0], [x0 + side, y0 + side], [x0, y0 + side]]))
    img = torch.full((height, width), GREY, dtype=torch.float32)
    # SS x SS samples a pixel put an edge within 1 / (2 SS) px of where it belongs; a strip of rows at a time keeps the samples in cache
    for y0 in range(0, height, STRIP):
        synth._paint_quad(img[y0:y0 + STRIP], quad - np.array([0.0, float(y0)]), sheet, side, 0, ss=SS)
    rng = np.random.RandomState(seed)
    out = img.numpy().astype(np.float64) + rng.normal(0.0, noise, (height, width))
    frame = np.clip(np.rint(out), 0, 255).astype(np.uint8)
    corners = synth.project(Kc, rvec, tvec, to3([corner_xy(L, c) for c in range(nc)]))
    quads = np.stack([synth.project(Kc, rvec, tvec, to3(marker_quad(L, s))) for s in white_squares(L)])
    return frame, corners, quads


def z_for(square_px_image, L):
    """the distance at which a frontal square is square_px_image pixels wide"""
    return K[0, 0] * UNIT * L[2] / square_px_image


# the GPU test's batch: 5 x 4 squares (12 corners, 10 markers), squares of about 90-110 px in the image
LAYOUT = (5, 4, 100, 70)
IDS = [7, 42, 100, 233, 311, 500, 640, 777, 901, 1010]
COVERED = 3       # the marker under the grey patch in frame "covered"


def scenes():
    """name -> (rvec, tvec, seed, covered markers) of the batch's rendered frames; "empty" is a plain grey frame"""
    L = LAYOUT
    return {
        "frontal": ((0.05, -0.04, 0.02), (0.004, -0.003, z_for(100, L)), 11, ()),
        "tilted": ((0.5, 0.0, 0.03), (-0.002, 0.012, z_for(98, L)), 12, ()),
        "covered": ((-0.08, 0.1, -0.03), (0.0, 0.002, z_for(104, L)), 23, (COVERED,)),
        "outside": ((0.03, 0.06, 0.0), (0.1393, -0.046, z_for(108, L)), 34, ()),
        "turned": ((0.1, -0.12, 0.3), (0.003, 0.0, z_for(92, L)), 15, ()),
    }


_frames = {}


def frame(name):
    """(frame, true corners, true quads) of a scene, rendered once per process"""
    if name not in _frames:
        if name == "empty":
            rng = np.random.RandomState(3)
            _frames[name] = (np.clip(np.rint(GREY + rng.normal(0, 1.0, (H, W))), 0, 255).astype(np.uint8), None, None)
        else:
            rv, tv, seed, cover = scenes()[name]
            _frames[name] = render(LAYOUT, IDS, rv, tv, seed, cover)
    return _frames[name]


BATCH = ("frontal", "tilted", "covered", "outside", "empty", "turned")


def true_markers(name, L=LAYOUT, ids=IDS, cover=()):
    """the frame's marker list had every uncovered marker been found at its true quad (float32), in id order"""
    quads = frame(name)[2]
    if quads is None:
        return []
    inside = lambda q: q[:, 0].min() >= 2 and q[:, 0].max() <= W - 3 and q[:, 1].min() >= 2 and q[:, 1].max() <= H - 3
    return sorted(((int(i), q.astype(np.float32)) for k, (i, q) in enumerate(zip(ids, quads)) if k not in cover and inside(q)), key=lambda m: m[0])


# margins between marker and square that give the window max_win (5), 4, 2 and 1 at squares of about 110 px in the image:
# (square_px, marker_px, the window). The margin m = (square_px - marker_px) / 2 is 110 m / square_px pixels wide there, and win = floor(that) - 1.
WINDOW_LAYOUTS = ((100, 70, 5), (101, 91, 4), (98, 91, 2), (96, 91, 1))


def window_frame(square_px, marker_px):
    L = (5, 4, square_px, marker_px)
    return L, render(L, IDS, (0.02, 0.03, 0.01), (0.002, -0.001, z_for(110, L)), seed=20 + square_px)


# the calibration's board and views: 6 x 5 squares (20 corners, 15 markers); the last view shows half the board
CALIB_LAYOUT = (6, 5, 80, 56)
CALIB_IDS = [3, 19, 77, 130, 201, 256, 340, 415, 499, 512, 603, 688, 750, 833, 999]
CALIB_POSES = (((0.0, 0.0, 0.0), (0.0, 0.0, 0.52)), ((0.45, 0.0, 0.05), (0.01, 0.02, 0.60)), ((-0.4, 0.1, -0.04), (-0.02, -0.01, 0.58)),
               ((0.05, 0.5, 0.02), (0.02, 0.0, 0.62)), ((0.1, -0.45, 0.1), (-0.03, 0.01, 0.60)), ((0.3, 0.3, -0.2), (0.0, -0.01, 0.64)),
               ((-0.3, 0.35, 0.25), (0.01, 0.01, 0.66)), ((-0.25, -0.3, 0.6), (0.0, 0.0, 0.7)), ((0.02, 0.04, 0.0), (0.26, 0.03, 0.5)))


def calib_frames():
    if "calib" not in _frames:
        _frames["calib"] = [render(CALIB_LAYOUT, CALIB_IDS, rv, tv, seed=40 + i) for i, (rv, tv) in enumerate(CALIB_POSES)]
    return _frames["calib"]
