"""Plain float64 reference for the pose solver at its edges (numpy + scipy): seeded families of marker and board poses with their
float32 corners, the two measures every pose comparison of these tests uses, and a polished reprojection minimum. Used by
test_pose_edges_cpu.py, which pins the CPU restatement on them, and by test_gpu_pose_edges.py, which holds the device solver to the same
cases (arucohip_calculate_extrinsics and arucohip_board_detect take corners directly). Rodrigues, the Brown projection and the marker's object points are planar_ref's."""
import numpy as np
from scipy.optimize import least_squares

from tests.planar_ref import brown_project, object_points, rodrigues

MARKER_SIZE = 0.05
K_MAIN = np.array([[1400.0, 0.0, 960.0], [0.0, 1400.0, 540.0], [0.0, 0.0, 1.0]])   # the matrix suite's camera
K_OFF = np.array([[1400.0, 0.0, 1160.0], [0.0, 1250.0, 540.0], [0.0, 0.0, 1.0]])   # fx != fy, principal point 200 px off centre
DIST8 = np.array([-0.35, 0.2, 2e-3, -1e-3, -0.05, 0.01, -0.02, 0.003])
POSE_TOL = 1e-4          # the project's pose tolerance
CONVERGED_TOL = 1e-5     # a tenth of it: the oracle's pose against the polished minimum started there
N_CASES = 48             # three launches' worth of 16-marker workgroups
NOISE = 0.3              # px, detection-sized

# name: (tilt range, z range, distortion coefficients, camera, noise levels)
FAMILIES = {
    "frontal": ((0.0, 0.02), (0.4, 1.5), None, K_MAIN, (0.0, NOISE)),
    "mild": ((0.1, 0.6), (0.4, 1.5), None, K_MAIN, (0.0, NOISE)),
    "steep": ((1.2, 1.45), (0.4, 1.5), None, K_MAIN, (0.0, NOISE)),
    "far": ((0.2, 1.0), (4.0, 8.0), None, K_MAIN, (0.0, NOISE)),      # markers of about 9 - 17 px
    "near": ((0.1, 0.8), (0.12, 0.2), None, K_MAIN, (0.0, NOISE)),
    "dist4": ((0.1, 1.0), (0.4, 1.5), DIST8[:4], K_MAIN, (0.0, NOISE)),
    "dist5": ((0.1, 1.0), (0.4, 1.5), DIST8[:5], K_MAIN, (0.0, NOISE)),
    "dist8": ((0.1, 1.0), (0.4, 1.5), DIST8, K_MAIN, (0.0, NOISE)),
    "pi": (None, (0.4, 1.5), None, K_MAIN, (0.0,)),                   # a rotation by exactly pi
    "identity": (None, (0.4, 1.5), None, K_MAIN, (0.0,)),             # rotation angle 0, 1e-9, 1e-6, 1e-3, seen from behind
    "turned": (None, (0.4, 1.5), None, K_MAIN, (0.0,)),               # rotateXAxis of the pose is a rotation by exactly pi (tilt up to 0.9)
    "offaxis": ((0.1, 1.0), (0.4, 1.5), DIST8[:5], K_OFF, (NOISE,)),
}
NOISE_FREE = [(f, 0.0) for f, v in FAMILIES.items() if 0.0 in v[4]]
ALL_CASES = [(f, s) for f, v in FAMILIES.items() for s in v[4]]
_SEEDS = {name: 7001 + 13 * i for i, name in enumerate(FAMILIES)}


def rot_z(a):
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


RX_PI = np.diag([1.0, -1.0, -1.0])   # the marker turned to face the camera


def facing_rotation(rng, tilt):
    """Rtilt(axis in the image plane, tilt) * Rz(uniform 0..2 pi) * Rx(pi)."""
    phi = rng.uniform(0.0, 2 * np.pi)
    return rodrigues(np.array([np.cos(phi), np.sin(phi), 0.0]) * tilt) @ rot_z(rng.uniform(0.0, 2 * np.pi)) @ RX_PI


def translation(rng, zr):
    return np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.1, 0.1), rng.uniform(*zr)])


def family(name, noise=0.0):
    """48 seeded cases of one family: dict with R [48,3,3], t [48,3], corners [48,4,2] float32 (the generating pose's projection plus
    Gaussian corner noise, rounded to float32), K, dist. The poses of a family are the same at every noise level."""
    tilt, zr, dist, K, levels = FAMILIES[name]
    assert noise in levels
    rng = np.random.default_rng(_SEEDS[name])
    Rs, ts = [], []
    for i in range(N_CASES):
        if name == "pi":
            a = (0.0, np.pi / 2, np.pi, 3 * np.pi / 2)[i] if i < 4 else rng.uniform(0.0, 2 * np.pi)
            R = rot_z(a) @ RX_PI
        elif name == "identity":
            axis = rng.normal(size=3)
            R = rodrigues(axis / np.linalg.norm(axis) * (0.0, 1e-9, 1e-6, 1e-3)[i % 4])
        elif name == "turned":   # R Rx(pi / 2) = 2 u u^T - I: the marker's normal is 2 u u_y - e_y, towards the camera where u_y u_z < 0
            u = rng.normal(size=3)
            while not 2 * u[1] * u[2] / (u @ u) < -0.62:
                u = rng.normal(size=3)
            R = (2 * np.outer(u, u) / (u @ u) - np.eye(3)) @ np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]])
        else:
            R = facing_rotation(rng, rng.uniform(*tilt))
        Rs.append(R), ts.append(translation(rng, zr))
    P = object_points(MARKER_SIZE)
    px = np.array([brown_project(P, R, t, K, dist) for R, t in zip(Rs, ts)])
    if noise > 0:
        px = px + np.random.default_rng(_SEEDS[name] + 1).normal(0.0, noise, px.shape)
    return {"name": name, "noise": noise, "R": np.array(Rs), "t": np.array(ts), "corners": px.astype(np.float32), "K": K, "dist": dist}


def pose_dev(r, t, R_ref, t_ref):
    """The two measures of every comparison here: max |R(r) - R_ref| and max |t - t_ref| / max |t_ref|. R_ref: a matrix or a vector."""
    R_ref = np.asarray(R_ref, np.float64)
    if R_ref.shape == (3,):
        R_ref = rodrigues(R_ref)
    t, t_ref = np.asarray(t, np.float64), np.asarray(t_ref, np.float64)
    return float(np.max(np.abs(rodrigues(r) - R_ref))), float(np.max(np.abs(t - t_ref)) / np.max(np.abs(t_ref)))


def polished_minimum(obj, img, K, dist, start):
    """The minimum of the reprojection residuals that `start` (rvec, tvec) leads to, as far as float64 goes: (rvec, tvec)."""
    obj = np.asarray(obj, np.float64).reshape(-1, 3)
    img = np.asarray(img, np.float64).reshape(-1, 2)

    def residuals(p):
        return (brown_project(obj, rodrigues(p[:3]), p[3:], K, dist) - img).reshape(-1)

    x0 = np.concatenate([np.asarray(start[0], np.float64), np.asarray(start[1], np.float64)])
    sol = least_squares(residuals, x0, jac="3-point", method="trf", x_scale="jac", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=200)
    return sol.x[:3], sol.x[3:]


_side = {}


def reference_side(name, noise, solve_pnp):
    """The reference side of one family, computed once per process: solve_pnp(obj, img, K, dist) -> (ok, rvec, tvec) (the oracle's, handed
    in by the caller: this module knows no oracle) on every case, and the convergence mask: a case is converged when that pose is within
    CONVERGED_TOL of polished_minimum started from it, in both measures. Returns the family's dict with ok, rvec, tvec, converged, polish_dev."""
    key = (name, noise)
    if key not in _side:
        fam = family(name, noise)
        P = object_points(MARKER_SIZE)
        ok, rv, tv, dev = [], [], [], []
        for c in fam["corners"]:
            o, r, t = solve_pnp(P, c, fam["K"].reshape(-1), fam["dist"])
            ok.append(o), rv.append(r), tv.append(t)
            if o and np.all(np.isfinite(r)) and np.all(np.isfinite(t)):
                pr, pt = polished_minimum(P, c, fam["K"], fam["dist"], (r, t))
                dev.append(max(pose_dev(r, t, pr, pt)))
            else:
                dev.append(np.inf)
        fam.update(ok=np.array(ok), rvec=np.array(rv), tvec=np.array(tv), polish_dev=np.array(dev))
        fam["converged"] = fam["polish_dev"] < CONVERGED_TOL
        _side[key] = fam
    return _side[key]


# ---- planar boards of 0.05 m markers on a grid, 0.01 m apart, centred, in metres (BoardConfiguration's METERS)
BOARD_SIZES = (1, 2, 15, 16, 17, 64, 128)
BOARD_POSES = {"mild": ((0.1, 0.6), None), "steep": ((1.2, 1.45), None), "dist8": ((0.1, 1.0), DIST8)}


def board(nm):
    """(ids [nm], obj [nm,4,3]) of an nm-marker grid of rows of 16 (the last row as long as it gets)."""
    cols = min(nm, 16)
    rows = (nm + cols - 1) // cols
    pitch = MARKER_SIZE + 0.01
    P = object_points(MARKER_SIZE)
    obj = np.zeros((nm, 4, 3))
    for i in range(nm):
        cx = (i % cols - (cols - 1) / 2.0) * pitch
        cy = ((rows - 1) / 2.0 - i // cols) * pitch
        obj[i] = P + [cx, cy, 0.0]
    return np.arange(nm, dtype=np.int32) + 100, obj.astype(np.float32)


def board_view(nm, pose, noise, K, seed):
    """One seeded view of the nm-marker board: dict with ids, obj, R, t, corners [nm,4,2] float32, K, dist. The board stands a full
    diagonal further away than a marker of the same family would, so that its far edge stays in front of the camera at every tilt."""
    tilt, dist = BOARD_POSES[pose]
    ids, obj = board(nm)
    rng = np.random.default_rng(seed)
    R = facing_rotation(rng, rng.uniform(*tilt))
    t = translation(rng, (0.4, 1.5))
    pts = obj.reshape(-1, 3).astype(np.float64)
    t[2] += 2.0 * np.max(np.linalg.norm(pts, axis=1))
    px = brown_project(pts, R, t, K, dist)
    if noise > 0:
        px = px + rng.normal(0.0, noise, px.shape)
    return {"ids": ids, "obj": obj, "R": R, "t": t, "corners": px.astype(np.float32).reshape(nm, 4, 2), "K": K, "dist": dist}
