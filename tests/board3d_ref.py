"""Float64 numpy restatement of how cv::solvePnP(ITERATIVE) starts on object points that are not all in z = 0, the fixtures of boards out
of a plane (a fold, a lifted planar board, cube faces) and their renderer. No oracle, no device code: numpy.linalg.eigh / svd where the
device uses Jacobi rotations. Shared by test_board3d_cpu.py, test_gpu_board3d.py and test_gpu_board3d_shim.py.

The rule, with n points M (metres) and pixels m:
  b. Mc = mean(M), MM = sum (M - Mc)(M - Mc)^T, eigenvalues w0 >= w1 >= w2 with unit eigenvectors v0, v1, v2.
  c. w2 / w1 < 1e-3: R_tr = rows v0, v1, v2 (negated when det < 0), T_tr = -R_tr Mc; least-squares homography from the first two
     coordinates of R_tr M + T_tr to the undistorted normalised image points; h1, h2, h1 x h2 -> nearest rotation R_h, t_h; the start is
     R = R_h R_tr, t = R_h T_tr + t_h.
  d. else, n >= 6 (fewer: no pose): rows [P, 0, -x P], [0, P, -y P] with P = (X, Y, Z, 1); the right singular vector of the smallest
     singular value as [RR | tt], negated when det RR < 0; R = U V^T of RR's SVD, t = tt sqrt(3) / |RR|_F.
The final pose is pose_ref.polished_minimum from that start, on the original 3-D points."""
import numpy as np

from tests import pose_ref
from tests.planar_ref import brown_project, homography, object_points, rodrigues, rodrigues_inv, undistort

PLANAR_RATIO = 1e-3      # OpenCV's constant
MARKER_SIZE = pose_ref.MARKER_SIZE
HINGE_GAP = 0.02         # metres from the hinge to the first column of a panel
PITCH = MARKER_SIZE + 0.01
FOLD_ANGLES = (90.0, 45.0, 10.0)
FOLD_SIZES = (2, 3, 15, 16, 17, 64, 128)      # 8 points (the smallest DLT) .. 512
FOLD_POSES = ("mild", "dist8")
LIFT = (np.array([0.3, -0.5, 0.2]), np.array([0.1, -0.05, 0.25]))   # the fixed rigid transform of lifted()


def spread(obj):
    """(w [3] descending, eigenvectors as rows [3,3], Mc) of the points' scatter matrix."""
    M = np.asarray(obj, np.float64).reshape(-1, 3)
    Mc = M.mean(axis=0)
    w, v = np.linalg.eigh((M - Mc).T @ (M - Mc))
    return w[::-1], v[:, ::-1].T, Mc


def spread_ratio(obj):
    w = spread(obj)[0]
    return float(abs(w[2]) / w[1]) if w[1] > 0 else float("nan")


def _nearest_rotation(A):
    U, _, Vt = np.linalg.svd(A)
    return U @ Vt


def start_pose(obj, img, K, dist):
    """(rvec, tvec, branch 'c' or 'd') of the start, or None where the rule gives no pose."""
    M = np.asarray(obj, np.float64).reshape(-1, 3)
    m = np.asarray(img, np.float64).reshape(-1, 2)
    if len(M) < 4 or not (np.all(np.isfinite(M)) and np.all(np.isfinite(m))):
        return None
    xy = undistort(m, np.asarray(K, np.float64).reshape(3, 3), dist)
    w, Rtr, Mc = spread(M)
    if abs(w[2]) / w[1] < PLANAR_RATIO:
        if np.linalg.det(Rtr) < 0:
            Rtr = -Rtr
        Ttr = -Rtr @ Mc
        flat = M @ Rtr.T + Ttr
        H = homography(flat[:, :2], xy)
        h1, h2 = H[:, 0], H[:, 1]
        n1, n2 = np.linalg.norm(h1), np.linalg.norm(h2)
        h1, h2 = h1 / n1, h2 / n2
        Rh = _nearest_rotation(np.stack([h1, h2, np.cross(h1, h2)], axis=1))
        th = H[:, 2] * 2.0 / (n1 + n2)
        R, t, branch = Rh @ Rtr, Rh @ Ttr + th, "c"
    else:
        if len(M) < 6:
            return None
        P = np.hstack([M, np.ones((len(M), 1))])
        Z = np.zeros_like(P)
        L = np.vstack([np.hstack([P, Z, -xy[:, :1] * P]), np.hstack([Z, P, -xy[:, 1:] * P])])
        p = np.linalg.svd(L)[2][-1].reshape(3, 4)
        if np.linalg.det(p[:, :3]) < 0:
            p = -p
        R = _nearest_rotation(p[:, :3])
        t, branch = p[:, 3] * np.sqrt(3.0) / np.linalg.norm(p[:, :3]), "d"
    if not (np.all(np.isfinite(R)) and np.all(np.isfinite(t))):
        return None
    return rodrigues_inv(R), t, branch


def solve(obj, img, K, dist):
    """The reference's pose: polished_minimum from the start. dict(rvec, tvec, start_rvec, start_tvec, branch) or None."""
    s = start_pose(obj, img, K, dist)
    if s is None:
        return None
    r, t = pose_ref.polished_minimum(obj, img, np.asarray(K, np.float64).reshape(3, 3), dist, (s[0], s[1]))
    return {"rvec": r, "tvec": t, "start_rvec": s[0], "start_tvec": s[1], "branch": s[2]}


def compose(r0, t0, lift=LIFT):
    """The pose of a board moved by `lift` (p -> R_l p + t_l), from the pose (r0, t0) of the board where it was: (R, t)."""
    Rl = rodrigues(lift[0])
    R = rodrigues(r0) @ Rl.T
    return R, np.asarray(t0, np.float64) - R @ lift[1]


# ---------------------------------------------------------------------------------------------
# fixtures: METERS boards of 0.05 m markers, y up, facing +z (pose_ref's poses turn +z towards the camera)
# ---------------------------------------------------------------------------------------------
def panel_axes(angle_deg):
    """Unit 'right' vector of panel 0 and panel 1 of a fold whose panels enclose angle_deg and meet on the y axis. Each panel leaves the
    hinge towards +z, so the fold opens towards the camera and neither panel hides the other."""
    h = np.radians(angle_deg) / 2.0
    return np.array([np.sin(h), 0.0, -np.cos(h)]), np.array([np.sin(h), 0.0, np.cos(h)])


def _panel_grid(n):
    cols = int(np.ceil(np.sqrt(n)))
    return cols, (n + cols - 1) // cols


def fold(nm, angle_deg):
    """(ids [nm], obj [nm,4,3] float32, panel [nm]) of nm markers dealt alternately to two panels hinged on the y axis: marker i goes to panel
    i % 2 as its entry i // 2, row-major on a grid of ceil(sqrt(n)) columns that begins HINGE_GAP from the hinge."""
    P = object_points(MARKER_SIZE)
    axes = panel_axes(angle_deg)
    up = np.array([0.0, 1.0, 0.0])
    obj = np.zeros((nm, 4, 3))
    for i in range(nm):
        p, k = i % 2, i // 2
        cols, rows = _panel_grid((nm + 1 - p) // 2)
        u = HINGE_GAP + MARKER_SIZE / 2 + (k % cols) * PITCH
        v = ((rows - 1) / 2.0 - k // cols) * PITCH
        right = axes[p]
        centre = (u if p else -u) * right + v * up
        obj[i] = centre + P[:, :1] * right + P[:, 1:2] * up
    return np.arange(nm, dtype=np.int32) + 100, obj.astype(np.float32), np.arange(nm) % 2


def lifted(board, lift=LIFT):
    """(ids, obj) of a planar board moved by the fixed rigid transform LIFT, rounded to float32 as a board file holds it."""
    ids, obj = board
    moved = np.asarray(obj, np.float64).reshape(-1, 3) @ rodrigues(lift[0]).T + lift[1]
    return ids, moved.reshape(-1, 4, 3).astype(np.float32)


def cube_faces(side=0.08):
    """(ids [3], obj [3,4,3]) of one marker on each of the three faces of a cube that meet at its corner (+, +, +), the corner towards +z."""
    P = object_points(MARKER_SIZE)
    h = side / 2.0
    faces = [(np.array([1.0, 0, 0]), np.array([0, 1.0, 0]), np.array([0, 0, 1.0])),     # front, z = +h
             (np.array([0, 0, -1.0]), np.array([0, 1.0, 0]), np.array([1.0, 0, 0])),    # right, x = +h
             (np.array([1.0, 0, 0]), np.array([0, 0, -1.0]), np.array([0, 1.0, 0]))]    # top, y = +h
    obj = np.array([h * n + P[:, :1] * r + P[:, 1:2] * u for r, u, n in faces])
    # turn the corner (1, 1, 1) / sqrt(3) onto +z so that the three faces are seen alike
    c = np.ones(3) / np.sqrt(3.0)
    axis = np.cross(c, [0, 0, 1.0])
    Rc = rodrigues(axis / np.linalg.norm(axis) * np.arccos(c[2]))
    return np.arange(3, dtype=np.int32) + 100, (obj.reshape(-1, 3) @ Rc.T).reshape(3, 4, 3).astype(np.float32)


Z_RANGE = (0.4, 0.7)     # metres before the board's own size is added


def view(board, pose, noise, K, seed, z_range=Z_RANGE):
    """pose_ref.board_view for any board (ids, obj, ...): a seeded pose of family `pose`, float32 corners, optional Gaussian corner noise.
    The boards stand nearer than pose_ref's (0.4 - 1.5 m): the linear start of eight noisy points degrades with the square of the
    distance, and past a metre a two-marker fold (60 px wide there) with 0.3 px of corner noise starts further from its minimum than the
    judging gate allows (0.1); that is a property of the rule, seen in this file's restatement alone."""
    tilt, dist = pose_ref.BOARD_POSES[pose]
    ids, obj = board[0], board[1]
    rng = np.random.default_rng(seed)
    R = pose_ref.facing_rotation(rng, rng.uniform(*tilt))
    t = pose_ref.translation(rng, z_range)
    pts = np.asarray(obj, np.float64).reshape(-1, 3)
    t[2] += 2.0 * np.max(np.linalg.norm(pts, axis=1))
    px = brown_project(pts, R, t, K, dist)
    if noise > 0:
        px = px + rng.normal(0.0, noise, px.shape)
    return {"ids": ids, "obj": obj, "R": R, "t": t, "corners": px.astype(np.float32).reshape(len(ids), 4, 2), "K": K, "dist": dist}


def fold_case(angle, nm, pose, noise):
    """One seeded view of fold(nm, angle)."""
    seed = 31000 + 1000 * FOLD_ANGLES.index(angle) + 10 * nm + 2 * FOLD_POSES.index(pose) + (1 if noise > 0 else 0)
    return view(fold(nm, angle), pose, noise, pose_ref.K_MAIN, seed)


def gate(v):
    """The judging gate of one view, from the reference alone: dict(judged, ref (solve's dict or None), start_dev, final_dev). A case is
    judged when the pose polished from the reference's start equals the pose polished from the generating pose within CONVERGED_TOL and
    the start lies within 0.1 of it, both in both measures of pose_ref.pose_dev."""
    obj = np.asarray(v["obj"], np.float64).reshape(-1, 3)
    img = v["corners"].reshape(-1, 2)
    ref = solve(obj, img, v["K"], v["dist"])
    if ref is None:
        return {"judged": False, "ref": None, "start_dev": np.inf, "final_dev": np.inf}
    tr, tt = pose_ref.polished_minimum(obj, img, v["K"], v["dist"], (rodrigues_inv(v["R"]), v["t"]))
    final = max(pose_ref.pose_dev(ref["rvec"], ref["tvec"], tr, tt))
    start = max(pose_ref.pose_dev(ref["start_rvec"], ref["start_tvec"], ref["rvec"], ref["tvec"]))
    return {"judged": bool(final < pose_ref.CONVERGED_TOL and start < 0.1), "ref": ref, "start_dev": start, "final_dev": final}


_cases = {}


def judged_cases():
    """Every fold case with its gate, computed once per process: list of dict(angle, nm, pose, noise, view, gate). Noise-free: all angles;
    0.3 px: 90 and 45 degrees (10 degrees with noise is not asked for: with two markers the reference itself lands in another minimum)."""
    if "all" not in _cases:
        out = []
        for angle in FOLD_ANGLES:
            for nm in FOLD_SIZES:
                for pose in FOLD_POSES:
                    for noise in (0.0, pose_ref.NOISE):
                        if noise > 0 and angle == 10.0:
                            continue
                        v = fold_case(angle, nm, pose, noise)
                        out.append({"angle": angle, "nm": nm, "pose": pose, "noise": noise, "view": v, "gate": gate(v)})
        _cases["all"] = out
    return _cases["all"]


# ---------------------------------------------------------------------------------------------
# frames: the 12-marker 90 degree fold through a 640 x 480 camera
# ---------------------------------------------------------------------------------------------
W, H = 640, 480
K_FRAME = np.array([[600.0, 0.0, 320.0], [0.0, 600.0, 240.0], [0.0, 0.0, 1.0]])
# (rotation vector applied before the board is turned to face the camera, tvec)
FRAME_POSES = [(np.array([0.0, 0.0, 0.0]), np.array([0.0, 0.0, 0.62])),
               (np.array([0.12, -0.15, 0.05]), np.array([0.01, 0.0, 0.66])),
               (np.array([-0.1, 0.2, -0.08]), np.array([-0.02, 0.01, 0.7])),
               (np.array([0.2, 0.1, 0.3]), np.array([0.0, -0.01, 0.75])),
               (np.array([-0.15, -0.1, -0.2]), np.array([0.02, 0.0, 0.68]))]


def frame_pose(i):
    """(rvec, tvec, R) of frame pose i: the board turned to face the camera, then FRAME_POSES[i]."""
    R = rodrigues(FRAME_POSES[i][0]) @ pose_ref.RX_PI
    return rodrigues_inv(R), FRAME_POSES[i][1], R


def render(board, rvec, tvec, angle_deg=90.0, panels=(0, 1), seed=5, noise=1.5, pad=0.012, damage=None):
    """uint8 frame [H][W] of a fold: one white synth._paint_quad sheet per panel of `panels` through synth.project, then that panel's
    markers. damage {board index: [(cy, cx), ...]}: those cells of the marker's 7 x 7 grid take the opposite colour.
    panels = (): the plain background."""
    import torch

    from aruco_amd import synth

    ids, obj, panel = board
    rng = np.random.RandomState(seed)
    img = torch.full((H, W), float(rng.uniform(90, 130)), dtype=torch.float32)
    white = rng.uniform(215, 240)
    axes = panel_axes(angle_deg)
    up = np.array([0.0, 1.0, 0.0])
    for p in panels:
        mine = np.asarray(obj, np.float64)[panel == p].reshape(-1, 3)
        u = mine @ axes[p]
        lo_u, hi_u = (HINGE_GAP / 4, u.max() + pad) if p else (u.min() - pad, -HINGE_GAP / 4)
        lo_v, hi_v = mine[:, 1].min() - pad, mine[:, 1].max() + pad
        sheet = np.array([lo_u * axes[p] + lo_v * up, hi_u * axes[p] + lo_v * up, hi_u * axes[p] + hi_v * up, lo_u * axes[p] + hi_v * up])
        synth._paint_quad(img, synth.project(K_FRAME, rvec, tvec, sheet), np.full((1, 1), white, np.float32), 1, 0)
    for i, (mid, o) in enumerate(zip(ids, obj)):
        if panel[i] not in panels:
            continue
        q = synth.project(K_FRAME, rvec, tvec, np.asarray(o, np.float64))
        synth._paint_quad(img, q, synth._marker_table(int(mid), 0, rng.uniform(15, 40), white), 7, 0)
        for cy, cx in (damage or {}).get(i, ()):
            Hm = synth._homography([(0, 0), (7, 0), (7, 7), (0, 7)], [tuple(c) for c in q])
            cell = []
            for a, b in ((cx, cy), (cx + 1, cy), (cx + 1, cy + 1), (cx, cy + 1)):
                c = Hm @ np.array([a, b, 1.0])
                cell.append(c[:2] / c[2])
            colour = 25.0 if synth.marker_bits(int(mid))[cy, cx] else 228.0
            synth._paint_quad(img, np.array(cell), np.full((1, 1), colour, np.float32), 1, 0)
    if noise > 0:
        gen = torch.Generator()
        gen.manual_seed(int(rng.randint(0, 2 ** 31 - 1)))
        img = img + torch.randn(img.shape, generator=gen) * noise
    return img.round().clamp(0, 255).to(torch.uint8).numpy()


def batch_frames():
    """(board, frames uint8 [5][H][W], shown [5]: how many of the 12 markers each frame is meant to show). Frame 2 shows panel 1 only
    (six coplanar markers: the tilted-plane branch), frame 3 is empty."""
    board = fold(12, 90.0)
    shows = [(0, 1), (0, 1), (1,), (), (0, 1)]
    frames = np.stack([render(board, *frame_pose(i)[:2], panels=shows[i], seed=5 + i) for i in range(5)])
    return board, frames, [12, 12, 6, 0, 12]
