"""Float64 numpy statement of the fisheye calls (include/arucohip.h, "Fisheye lenses"): the equidistant model, its inverse with the
validity rule, the remap table and the remap itself, the marker-list mapping, and the frames the tests detect on: the golden board
rendered through a pinhole camera and resampled into a fisheye frame."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
W, H = 640, 480
K = np.array([[230.0, 0, 319.5], [0, 230.0, 239.5], [0, 0, 1]])
D = np.array([-0.03, 0.01, -0.004, 0.001])          # a lens of roughly 200 degrees at 640 x 480
KNEW = np.array([[200.0, 0, 319.5], [0, 200.0, 239.5], [0, 0, 1]])
K2 = np.array([[236.0, 0, 316.0], [0, 233.0, 242.5], [0, 0, 1]])   # a second lens for the interleaved streams
D2 = np.array([-0.02, 0.004, 0.001, -0.0005])
UNIT = 0.039 / 100.0                                 # board units -> metres (marker side 0.039)
MARKER_SIZE = 0.039
# the two poses at which the CPU detector finds all 24 markers of the fisheye frame
POSES = [(np.array([0.1, -0.15, 0.05]), np.array([0.0, 0.0, 0.22])), (np.array([0.3, 0.2, -0.1]), np.array([0.03, -0.02, 0.2]))]
NEWTON_STEPS, RESIDUAL, DEFAULT_MAX_ANGLE = 10, 1e-12, 1.4
# The CPU chain (oracle detect on the fisheye frame -> marker undistortion -> oracle board pose with Knew) against the true pose,
# measured with tests/test_fisheye_cpu.py on the two poses at which all 24 markers are found: rotation between the two poses in
# radians, translation relative to its largest component. The detector fits straight lines to slightly curved edges (corners 1.19 and 0.98 px from the
# true fisheye corners), which is what these errors are. The rendering is deterministic; the test allows twice the measured value
# for libm differences between machines.
CHAIN_MEASURED = [(2.1842e-3, 9.7145e-4), (1.4390e-3, 5.8118e-4)]
PIN_W, PIN_H, PIN_F = 1600, 1200, 460.0


def max_angle_of(max_angle):
    """the double the library compares with: max_angle travels as a float, <= 0 selects the default"""
    return float(np.float32(max_angle)) if max_angle > 0 else DEFAULT_MAX_ANGLE


def theta_d(D, th):
    t2 = th * th
    return th * (1 + t2 * (D[0] + t2 * (D[1] + t2 * (D[2] + t2 * D[3]))))


def dtheta_d(D, th):
    t2 = th * th
    return 1 + t2 * (3 * D[0] + t2 * (5 * D[1] + t2 * (7 * D[2] + t2 * 9 * D[3])))


def project(K, D, P):
    """camera-frame points (n, 3) -> (fisheye pixels (n, 2), field angles (n,))"""
    P = np.asarray(P, np.float64)
    r = np.hypot(P[:, 0], P[:, 1])
    th = np.arctan2(r, P[:, 2])
    s = np.where(r > 0, theta_d(D, th) / np.where(r > 0, r, 1.0), 0.0)
    return np.stack([K[0, 0] * (P[:, 0] * s) + K[0, 2], K[1, 1] * (P[:, 1] * s) + K[1, 2]], axis=1), th


def unproject(K, D, px, max_angle=0.0):
    """fisheye pixels (n, 2) -> (ideal normalised points (n, 2), valid (n,), margin (n,)). margin: how far the point is from the
    nearest edge of the validity rule (inf where the derivative test decided): a test compares flags only where it is large against
    the evaluation error."""
    px = np.asarray(px, np.float64).reshape(-1, 2)
    ma = max_angle_of(max_angle)
    x, y = (px[:, 0] - K[0, 2]) / K[0, 0], (px[:, 1] - K[1, 2]) / K[1, 1]
    thd = np.hypot(x, y)
    th = thd.copy()
    rising = np.ones(len(px), bool)
    for _ in range(NEWTON_STEPS):
        d = dtheta_d(D, th)
        rising &= d > 0
        step = (theta_d(D, th) - thd) / np.where(rising, d, 1.0)
        th = np.where(rising, th - step, th)
    res = np.abs(theta_d(D, th) - thd)
    bound = RESIDUAL * np.maximum(thd, 1.0)
    valid = rising & (res <= bound) & (th <= ma)
    # the angle's margin in radians. The residual's bound is itself 1e-12, so its margin is taken as a ratio: a converged iteration
    # sits near 1e-16 and a failed one orders above the bound; a residual within a factor 100 of the bound counts as no margin at all
    clear = (res <= bound / 100) | (res >= bound * 100)
    margin = np.where(rising, np.where(clear, np.where(res <= bound, np.abs(th - ma), np.inf), 0.0), np.inf)
    with np.errstate(all="ignore"):
        s = np.where(thd > 0, np.tan(th) / np.where(thd > 0, thd, 1.0), 1.0)
    zero = thd == 0
    valid = valid | zero
    margin = np.where(zero, np.inf, margin)
    return np.stack([x * s, y * s], axis=1), valid, margin


def undistort_points(px, K, D, Knew=None, max_angle=0.0):
    """fisheye pixels -> (ideal pixels under Knew in float64, zeros where invalid; valid; margin)"""
    Kn = K if Knew is None else np.asarray(Knew, np.float64).reshape(3, 3)
    n, valid, margin = unproject(K, D, px, max_angle)
    h = np.concatenate([n, np.ones((len(n), 1))], axis=1) @ Kn.T
    with np.errstate(all="ignore"):
        out = h[:, :2] / h[:, 2:3]
    return np.where(valid[:, None], out, 0.0), valid, margin


def distort_points(px, K, D, Knew=None):
    """ideal pixels under Knew -> fisheye pixels, float64"""
    Kn = K if Knew is None else np.asarray(Knew, np.float64).reshape(3, 3)
    px = np.asarray(px, np.float64).reshape(-1, 2)
    rays = np.concatenate([px, np.ones((len(px), 1))], axis=1) @ np.linalg.inv(Kn).T
    return project(K, D, rays)[0]


def build_map(width, height, K, D, Knew=None, max_angle=0.0):
    """The remap table: (32 u, 32 v) in float64 [H][W] each, and the mask of destination pixels beyond max_angle."""
    ys, xs = np.mgrid[0:height, 0:width]
    Kn = K if Knew is None else np.asarray(Knew, np.float64).reshape(3, 3)
    rays = np.stack([xs.ravel(), ys.ravel(), np.ones(width * height)], axis=1).astype(np.float64) @ np.linalg.inv(Kn).T
    uv, th = project(K, D, rays)
    beyond = ~(th <= max_angle_of(max_angle))
    return (uv[:, 0] * 32).reshape(height, width), (uv[:, 1] * 32).reshape(height, width), beyond.reshape(height, width)


def near_rounding_boundary(u32, v32, eps=1e-8):
    """destination pixels whose 32 u or 32 v lies within eps of a half: there the rounded table entry may differ"""
    def near(a):
        return np.abs((a - np.floor(a)) - 0.5) <= eps
    return near(u32) | near(v32)


def remap(img, u32, v32, beyond):
    """The fixed-point bilinear remap (5 fractional bits, 15-bit weights, constant 0 outside) of an 8-bit image [H][W] or [H][W][3]."""
    img = np.asarray(img, np.uint8)
    hgt, wid = img.shape[:2]
    lo, hi = -32768.0 * 32, 32767.0 * 32 + 31
    iu = np.rint(np.clip(u32, lo, hi)).astype(np.int64)   # rint: round half to even
    iv = np.rint(np.clip(v32, lo, hi)).astype(np.int64)
    sx, sy, fx, fy = iu >> 5, iv >> 5, iu & 31, iv & 31
    src = img.reshape(hgt, wid, -1).astype(np.int64)

    def tap(yy, xx):
        inside = (xx >= 0) & (xx < wid) & (yy >= 0) & (yy < hgt)
        return np.where(inside[..., None], src[np.clip(yy, 0, hgt - 1), np.clip(xx, 0, wid - 1)], 0)

    w00, w01, w10, w11 = (32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32
    v = (tap(sy, sx) * w00[..., None] + tap(sy, sx + 1) * w01[..., None] + tap(sy + 1, sx) * w10[..., None] + tap(sy + 1, sx + 1) * w11[..., None]
         + (1 << 14)) >> 15
    v = np.where(beyond[..., None], 0, v)
    return np.clip(v, 0, 255).astype(np.uint8).reshape(img.shape)


POINTS_MAX_ANGLE = 1.2
D_NOT_MONOTONE = np.array([-0.5, 0.0, 0.0, 0.0])   # theta_d(theta) turns back at theta = sqrt(2 / 3), theta_d = 0.544


def point_cases():
    """The fisheye pixels the point tests undistort under (K, D, KNEW, POINTS_MAX_ANGLE), float32 (n, 2): a grid over the frame (its
    corners lie beyond max_angle), the principal point (theta_d = 0), points far beyond max_angle, and along two directions the
    float32 pixels nearest to theta = max_angle on either side whose margin still exceeds 1e-9 rad (a float32 pixel cannot sit on
    the angle itself: its neighbours are 1e-7 rad apart). Returns (pixels, index of the first near-edge point): the near-edge points
    come in pairs (inside, beyond)."""
    ys, xs = np.mgrid[3:H:43, 5:W:47]
    pts = [np.stack([xs.ravel() + 0.25, ys.ravel() + 0.75], axis=1), [[K[0, 2], K[1, 2]]], [[-150.0, 239.5], [319.5, 700.0], [900.0, 900.0]]]
    edge_from = sum(len(p) for p in pts)
    ma = max_angle_of(POINTS_MAX_ANGLE)
    for d in (np.array([1.0, 0.0]), np.array([-0.6, 0.8])):
        c = np.array([K[0, 2], K[1, 2]]) + np.array([K[0, 0], K[1, 1]]) * d * theta_d(D, ma)
        c32 = c.astype(np.float32)
        near = np.array([[np.float32(c32[0] + k * np.spacing(c32[0])), c32[1]] for k in range(-6, 7)], np.float32)
        _, valid, margin = unproject(K, D, near, POINTS_MAX_ANGLE)
        good = margin > 1e-9
        inside = [i for i in range(len(near)) if good[i] and valid[i]]
        beyond = [i for i in range(len(near)) if good[i] and not valid[i]]
        pts.append([near[min(inside, key=lambda i: margin[i])], near[min(beyond, key=lambda i: margin[i])]])
    return np.concatenate([np.asarray(p, np.float64) for p in pts]).astype(np.float32), edge_from


def not_monotone_cases():
    """Pixels under (K, D_NOT_MONOTONE): theta_d = 0.3 has a root below the turning point (valid), 0.6 and 0.9 have none (invalid)."""
    return np.array([[K[0, 2] + K[0, 0] * t, K[1, 2]] for t in (0.3, 0.6, 0.9)], np.float32)


def undistort_markers(markers, K, D, Knew=None, max_angle=0.0):
    """One frame's markers (dicts with id and corners (4, 2)) -> (the kept markers with float32 ideal corners, in order; dropped;
    the smallest validity margin over all corners)."""
    out, dropped, margin = [], 0, np.inf
    for m in markers:
        c, valid, mg = undistort_points(np.asarray(m["corners"], np.float32).reshape(4, 2), K, D, Knew, max_angle)
        margin = min(margin, float(mg.min()))
        if valid.all():
            out.append({"id": int(m["id"]), "corners": c.astype(np.float32)})
        else:
            dropped += 1
    return out, dropped, margin


def rodrigues(r):
    r = np.asarray(r, np.float64)
    th = np.linalg.norm(r)
    if th < 1e-300:
        return np.eye(3)
    k = r / th
    X = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.cos(th) * np.eye(3) + (1 - np.cos(th)) * np.outer(k, k) + np.sin(th) * X


def board():
    """The 24-marker golden board: ids [24], obj [24][4][3] in board units (PIX, 100 units per marker side)."""
    bc = json.load(open(os.path.join(GOLDEN, "board.json")))["board_conf"]
    return list(bc["ids"]), np.asarray(bc["obj"], np.float64)


def true_corners(rvec, tvec, K=K, D=D):
    """the board's marker corners [24][4][2] as the fisheye lens sees them at a pose"""
    _, obj = board()
    P = (obj.reshape(-1, 3) * UNIT) @ rodrigues(rvec).T + np.asarray(tvec, np.float64)
    return project(K, D, P)[0].reshape(-1, 4, 2)


def fisheye_from_pinhole(big, Kbig, K, D, width=W, height=H):
    """Resample a pinhole image into the frame a fisheye lens (K, D) sees: every fisheye pixel reads the pinhole image bilinearly where
    its ray lands (0 where the ray leaves the pinhole image or the pixel is not valid)."""
    ys, xs = np.mgrid[0:height, 0:width]
    n, valid, _ = unproject(K, D, np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.float64), 1.5)
    u = Kbig[0, 0] * n[:, 0] + Kbig[0, 2]
    v = Kbig[1, 1] * n[:, 1] + Kbig[1, 2]
    hb, wb = big.shape
    ok = valid & (u >= 0) & (u <= wb - 1) & (v >= 0) & (v <= hb - 1)
    u, v = np.where(ok, u, 0.0), np.where(ok, v, 0.0)
    x0, y0 = np.minimum(np.floor(u).astype(int), wb - 2), np.minimum(np.floor(v).astype(int), hb - 2)
    a, b = u - x0, v - y0
    src = big.astype(np.float64)
    val = (src[y0, x0] * (1 - a) + src[y0, x0 + 1] * a) * (1 - b) + (src[y0 + 1, x0] * (1 - a) + src[y0 + 1, x0 + 1] * a) * b
    return np.where(ok, np.rint(val), 0).astype(np.uint8).reshape(height, width)


_FRAMES = {}


def fisheye_frame(pose, K=K, D=D, seed=11):
    """The golden board at POSES[pose] through the lens (K, D): uint8 [480][640]. Deterministic; computed once per (pose, lens)."""
    key = (pose, tuple(K.ravel()), tuple(D), seed)
    if key not in _FRAMES:
        from aruco_amd import synth

        ids, obj = board()
        Kbig = np.array([[PIN_F, 0, (PIN_W - 1) / 2], [0, PIN_F, (PIN_H - 1) / 2], [0, 0, 1]])
        rvec, tvec = POSES[pose]
        big, _ = synth.render_board(ids, obj, Kbig, rvec, tvec, PIN_W, PIN_H, np.random.RandomState(seed), unit=UNIT)
        _FRAMES[key] = fisheye_from_pinhole(big.numpy(), Kbig, K, D)
    return _FRAMES[key]


# ---- calibration: intr = fx fy cx cy k1 k2 k3 k4
INTR_TRUE = np.array([230.0, 228.0, 322.0, 236.0, -0.03, 0.01, -0.004, 0.001])
FLAGS = {"USE_INTRINSIC_GUESS": 1, "FIX_ASPECT_RATIO": 2, "FIX_PRINCIPAL_POINT": 4, "FIX_K1": 8, "FIX_K2": 16, "FIX_K3": 32, "FIX_K4": 64}


def intr_of(K, D):
    K = np.asarray(K, np.float64).reshape(3, 3)
    return np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]] + list(np.asarray(D, np.float64).reshape(4)))


def model_of(intr):
    return np.array([[intr[0], 0, intr[2]], [0, intr[1], intr[3]], [0, 0, 1.0]]), np.array(intr[4:8], np.float64)


def project_view(intr, rvec, tvec, obj):
    """points in front of the camera; also for complex arguments (complex-step derivatives)"""
    from tests.calib_ref import rodrigues as rod   # sqrt(r . r): complex-safe

    P = obj @ rod(rvec).T + tvec
    r = np.sqrt(P[:, 0] * P[:, 0] + P[:, 1] * P[:, 1])
    th = np.arctan(r / P[:, 2])
    s = theta_d(intr[4:8], th) / r
    return np.stack([intr[0] * (P[:, 0] * s) + intr[2], intr[1] * (P[:, 1] * s) + intr[3]], axis=1)


def make_views(nviews=12, noise=0.0, seed=5, intr=INTR_TRUE, size=(W, H)):
    """nviews poses of the golden board (96 corners, metres) in front of the lens: rvec uniform +-0.5 (z +-0.2), t = (+-0.15, +-0.1,
    0.12 .. 0.25); a view with a point within 2 px of the border is drawn again. Points projected in float64, returned as float32."""
    rng = np.random.RandomState(seed)
    obj = board()[1].reshape(-1, 3) * UNIT
    objs, imgs = [], []
    while len(objs) < nviews:
        r = rng.uniform(-0.5, 0.5, 3) * np.array([1, 1, 0.4])
        t = np.array([rng.uniform(-0.15, 0.15), rng.uniform(-0.1, 0.1), rng.uniform(0.12, 0.25)])
        m = project_view(intr, r, t, obj)
        if (m < 2).any() or (m[:, 0] > size[0] - 3).any() or (m[:, 1] > size[1] - 3).any():
            continue
        if noise:
            m = m + rng.normal(0, noise, m.shape)
        objs.append(obj.astype(np.float32))
        imgs.append(m.astype(np.float32))
    return objs, imgs


def start_points(intr, img):
    """a view's pixels undistorted with the start model, each angle clamped to 1.5 rad: the normalised points (n, 2) float64 from which
    the start pose is made"""
    m = np.asarray(img, np.float64)
    x, y = (m[:, 0] - intr[2]) / intr[0], (m[:, 1] - intr[3]) / intr[1]
    thd = np.hypot(x, y)
    th = thd.copy()
    for _ in range(NEWTON_STEPS):
        th = th - (theta_d(intr[4:8], th) - thd) / dtheta_d(intr[4:8], th)
    sc = np.where(thd > 0, np.tan(np.clip(th, 0, 1.5)) / np.where(thd > 0, thd, 1), 1.0)
    return np.stack([x * sc, y * sc], axis=1)


MIXED_COUNTS = (20, 31, 63, 64, 65, 96, 24, 40, 96, 70, 33, 50)   # below 32, either side of 64, and the whole board


def mixed_views():
    """make_views(12, noise=0.3) with view v cut down to a seeded subset of MIXED_COUNTS[v] of its 96 corners, in corner order"""
    objs, imgs = make_views(12, noise=0.3)
    rng = np.random.RandomState(77)
    keep = [np.sort(rng.choice(96, n, replace=False)) for n in MIXED_COUNTS]
    return [o[k] for o, k in zip(objs, keep)], [m[k] for m, k in zip(imgs, keep)]


def calib_start(objs, imgs, size, flags=0, model=None):
    """The start of arucohip_fisheye_calibrate: cx, cy at the image centre, fx = fy = max(w, h) / pi, D = 0 (or the given model); every
    view's pose from the homography of its points undistorted with that model, each angle clamped to 1.5 rad."""
    from tests.calib_ref import homography

    Kin = np.zeros((3, 3)) if model is None else np.asarray(model[0], np.float64).reshape(3, 3)
    aspect = Kin[0, 0] / Kin[1, 1] if Kin[0, 0] > 0 and Kin[1, 1] > 0 else 1.0
    if flags & 1:
        intr = intr_of(Kin, model[1])
    else:
        f = max(size) / np.pi
        intr = np.array([f, f, (size[0] - 1) * 0.5, (size[1] - 1) * 0.5, 0, 0, 0, 0.0])
    if flags & 2:
        intr[0] = aspect * intr[1]
    poses = []
    for o, m in zip(objs, imgs):
        Hm = homography(np.asarray(o, np.float64), start_points(intr, m))
        s = 2 / (np.linalg.norm(Hm[:, 0]) + np.linalg.norm(Hm[:, 1]))
        r1, r2 = Hm[:, 0] / np.linalg.norm(Hm[:, 0]), Hm[:, 1] / np.linalg.norm(Hm[:, 1])
        U, _, Vt = np.linalg.svd(np.stack([r1, r2, np.cross(r1, r2)], axis=1))
        R = U @ Vt
        t = Hm[:, 2] * s - float(o[0][2]) * R[:, 2]
        ang = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
        w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
        poses.append(np.concatenate([w * ang / (2 * np.sin(ang)) if ang > 1e-12 else np.zeros(3), t]))
    return intr, aspect, np.array(poses)


def _Problem(objs, imgs, size, flags, model):
    """The cost both solvers minimise (calib_ref.Problem with this model's projection): residuals over the free intrinsics (masked as the
    device masks them) and every view's pose, from calib_start."""
    from tests.calib_ref import Problem

    intr0, aspect, poses0 = calib_start(objs, imgs, size, flags, model)
    free = np.ones(8, bool)
    for bit, idx in ((2, [0]), (4, [2, 3]), (8, [4]), (16, [5]), (32, [6]), (64, [7])):
        if flags & bit:
            free[idx] = False
    return Problem(project_view, objs, imgs, intr0, poses0, free, aspect if flags & 2 else None)


def lm_calibrate(objs, imgs, size, flags=0, model=None, max_iter=30):
    """The device's Levenberg-Marquardt, dense (calib_ref.lm_solve: CvLevMarq's rule, at most max_iter accepted steps), on this model."""
    from tests.calib_ref import lm_solve

    return lm_solve(_Problem(objs, imgs, size, flags, model), max_iter)


def scipy_calibrate(objs, imgs, size, flags=0, model=None):
    """scipy's least_squares on the same cost from the same start: its minimum"""
    from scipy.optimize import least_squares

    p = _Problem(objs, imgs, size, flags, model)
    r = least_squares(p.resid, p.x0, jac=p.jac, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=500)
    return p.result(r.x)


def intr_of_result(res):
    return intr_of(res["K"], res["D"])


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
