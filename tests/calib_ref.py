"""Host model of the camera calibration (cv::calibrateCamera, pinhole + k1 k2 p1 p2 k3) for the calibration tests: synthetic views,
the start values of OpenCV's planar initialisation and a scipy.optimize.least_squares solve of the same problem."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K_TRUE = np.array([[1400.0, 0, 965.0], [0, 1390.0, 535.0], [0, 0, 1]])
DIST_TRUE = np.array([-0.12, 0.05, 1e-3, -8e-4, 0.01])
SIZE = (1920, 1080)
FLAGS = {"USE_INTRINSIC_GUESS": 1, "FIX_ASPECT_RATIO": 2, "FIX_PRINCIPAL_POINT": 4, "ZERO_TANGENT_DIST": 8, "FIX_FOCAL_LENGTH": 16,
         "FIX_K1": 32, "FIX_K2": 64, "FIX_K3": 128}


def board_points():
    """The 6x4 board of tests/golden/board.json in metres (marker side 0.039), 96 corners at z = 0."""
    bc = json.load(open(os.path.join(GOLDEN, "board.json")))["board_conf"]
    obj = np.asarray(bc["obj"], np.float64).reshape(-1, 3)
    return obj * (0.039 / 100.0)


def rodrigues(r):
    """also for complex r (complex-step derivatives): the norm is sqrt(r . r), not |r|"""
    r = np.asarray(r)
    th = np.sqrt(np.sum(r * r))
    if abs(th) < 1e-300:
        return np.eye(3)
    k = r / th
    X = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.cos(th) * np.eye(3) + (1 - np.cos(th)) * np.outer(k, k) + np.sin(th) * X


def project(intr, rvec, tvec, obj):
    """intr = fx fy cx cy k1 k2 p1 p2 k3; obj (n, 3) -> (n, 2) float64"""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = intr
    P = obj @ rodrigues(rvec).T + tvec
    x, y = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]
    r2 = x * x + y * y
    cd = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 ** 3
    xd = x * cd + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * cd + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return np.stack([fx * xd + cx, fy * yd + cy], axis=1)


def intr_of(K, dist):
    K = np.asarray(K, np.float64).reshape(3, 3)
    return np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]] + list(np.asarray(dist, np.float64).reshape(5)))


def make_views(nviews=20, noise=0.0, seed=5, K=K_TRUE, dist=DIST_TRUE):
    """nviews poses of the board in front of the camera; points projected in float64, returned as float32."""
    rng = np.random.RandomState(seed)
    obj = board_points()
    intr = intr_of(K, dist)
    objs, imgs = [], []
    for _ in range(nviews):
        r = rng.uniform(-0.45, 0.45, 3) * np.array([1, 1, 0.3])
        t = np.array([rng.uniform(-0.06, 0.06), rng.uniform(-0.04, 0.04), rng.uniform(0.55, 0.8)])
        m = project(intr, r, t, obj)
        if noise:
            m = m + rng.normal(0, noise, m.shape)
        objs.append(obj.astype(np.float32))
        imgs.append(m.astype(np.float32))
    return objs, imgs


def homography(obj, img, normal=False):
    """normalised DLT plane (X, Y) -> pixel, h33 = 1. normal: the same least squares by its normal equations (as the device solves it)
    instead of lstsq; the distance between the two is what the start-value tests take as the reference's own error."""
    X, m = obj[:, :2].astype(np.float64), img.astype(np.float64)
    cM, cm = X.mean(0), m.mean(0)
    sM, sm = 1 / np.abs(X - cM).mean(0), 1 / np.abs(m - cm).mean(0)
    Xn, mn = (X - cM) * sM, (m - cm) * sm
    rows, rhs = [], []
    for (a, b), (x, y) in zip(Xn, mn):
        rows += [[a, b, 1, 0, 0, 0, -x * a, -x * b], [0, 0, 0, a, b, 1, -y * a, -y * b]]
        rhs += [x, y]
    A, b = np.array(rows), np.array(rhs)
    h = np.linalg.solve(A.T @ A, A.T @ b) if normal else np.linalg.lstsq(A, b, rcond=None)[0]
    H0 = np.append(h, 1).reshape(3, 3)
    Tm = np.array([[1 / sm[0], 0, cm[0]], [0, 1 / sm[1], cm[1]], [0, 0, 1]])
    TM = np.array([[sM[0], 0, -cM[0] * sM[0]], [0, sM[1], -cM[1] * sM[1]], [0, 0, 1]])
    H = Tm @ H0 @ TM
    return H / H[2, 2]


def start_values(objs, imgs, size, flags=0, K=None, dist=None, normal=False):
    """OpenCV's planar start: principal point at the image centre, fx, fy from the vanishing points of every view
    (initIntrinsicParams2D), distortion 0, pose from H and K; or K / dist with USE_INTRINSIC_GUESS. normal: see homography."""
    Kin = np.zeros((3, 3)) if K is None else np.asarray(K, np.float64).reshape(3, 3)
    aspect = Kin[0, 0] / Kin[1, 1] if Kin[0, 0] > 0 and Kin[1, 1] > 0 else 1.0
    if flags & 1:
        intr = intr_of(Kin, dist if dist is not None else np.zeros(5))
    else:
        cx, cy = (size[0] - 1) * 0.5, (size[1] - 1) * 0.5
        A, b = [], []
        for o, m in zip(objs, imgs):
            H = homography(o, m, normal)
            H[0] -= H[2] * cx
            H[1] -= H[2] * cy
            h, v = H[:, 0], H[:, 1]
            d1, d2 = (h + v) * 0.5, (h - v) * 0.5
            h, v, d1, d2 = h / np.linalg.norm(h), v / np.linalg.norm(v), d1 / np.linalg.norm(d1), d2 / np.linalg.norm(d2)
            A += [[h[0] * v[0], h[1] * v[1]], [d1[0] * d2[0], d1[1] * d2[1]]]
            b += [-h[2] * v[2], -d1[2] * d2[2]]
        A, b = np.array(A), np.array(b)
        f = np.linalg.solve(A.T @ A, A.T @ b) if normal else np.linalg.lstsq(A, b, rcond=None)[0]
        fx, fy = np.sqrt(abs(1 / f[0])), np.sqrt(abs(1 / f[1]))
        if flags & 2:
            tf = (fx + fy) / (aspect + 1)
            fx, fy = aspect * tf, tf
        intr = np.array([fx, fy, cx, cy, 0, 0, 0, 0, 0.0])
    if flags & 8:
        intr[6:8] = 0
    poses = []
    Km = np.array([[intr[0], 0, intr[2]], [0, intr[1], intr[3]], [0, 0, 1]])
    for o, m in zip(objs, imgs):
        H = np.linalg.solve(Km, homography(o, m, normal))
        s = 2 / (np.linalg.norm(H[:, 0]) + np.linalg.norm(H[:, 1]))
        r1, r2 = H[:, 0] / np.linalg.norm(H[:, 0]), H[:, 1] / np.linalg.norm(H[:, 1])
        U, _, Vt = np.linalg.svd(np.stack([r1, r2, np.cross(r1, r2)], axis=1))
        R = U @ Vt
        t = H[:, 2] * s - float(o[0, 2]) * R[:, 2]
        th = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
        w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
        rv = w * th / (2 * np.sin(th)) if th > 1e-12 else np.zeros(3)
        poses.append(np.concatenate([rv, t]))
    return intr, aspect, np.array(poses)


def free_of(flags):
    """which of the nine intrinsics a run with these flags leaves free, as the device solver masks them"""
    free = np.ones(9, bool)
    for bit, idx in ((2, [0]), (16, [0, 1]), (4, [2, 3]), (8, [6, 7]), (32, [4]), (64, [5]), (128, [8])):
        if flags & bit:
            free[idx] = False
    return free


def scipy_calibrate(objs, imgs, size, flags=0, K=None, dist=None, sparse=False):
    """least_squares over the free intrinsics (masked as the device solver masks them) and every view's rvec, tvec. sparse: a
    sparse Jacobian and an iterative trust-region solve, for thousands of views."""
    from scipy.optimize import least_squares

    intr0, aspect, poses0 = start_values(objs, imgs, size, flags, K, dist)
    free = free_of(flags)
    nf, V = int(free.sum()), len(objs)
    o64 = [np.asarray(o, np.float64) for o in objs]
    m64 = [np.asarray(m, np.float64) for m in imgs]

    def unpack(x):
        intr = intr0.astype(x.dtype)
        intr[free] = x[:nf]
        if flags & 2:
            intr[0] = aspect * intr[1]
        return intr, x[nf:].reshape(V, 6)

    def resid(x):
        intr, poses = unpack(x)
        return np.concatenate([(project(intr, p[:3], p[3:], o) - m).ravel() for o, m, p in zip(o64, m64, poses)])

    rows = np.cumsum([0] + [2 * len(o) for o in objs])
    H = 1e-30

    def jac_parts(x):
        """complex-step derivatives (exact to rounding): one evaluation per free intrinsic, six for all poses at once. Returns the
        intrinsic columns (m, nf) and the pose derivatives (m, 6): row i's pose columns belong to the view that holds row i."""
        Ji = np.zeros((rows[-1], nf))
        Jp = np.zeros((rows[-1], 6))
        for j in range(nf):
            xc = x.astype(complex)
            xc[j] += 1j * H
            Ji[:, j] = resid(xc).imag / H
        for k in range(6):
            xc = x.astype(complex)
            xc[nf + k::6] += 1j * H
            Jp[:, k] = resid(xc).imag / H
        return Ji, Jp

    view_of_row = np.repeat(np.arange(V), np.diff(rows))

    def jac(x):
        Ji, Jp = jac_parts(x)
        J = np.zeros((rows[-1], x.size))
        J[:, :nf] = Ji
        for v in range(V):
            J[rows[v]:rows[v + 1], nf + 6 * v:nf + 6 * v + 6] = Jp[rows[v]:rows[v + 1]]
        return J

    def jac_sparse(x):
        from scipy.sparse import csr_matrix

        Ji, Jp = jac_parts(x)
        m = rows[-1]
        r = np.concatenate([np.repeat(np.arange(m), nf), np.repeat(np.arange(m), 6)])
        c = np.concatenate([np.tile(np.arange(nf), m), (nf + 6 * view_of_row[:, None] + np.arange(6)[None, :]).ravel()])
        return csr_matrix((np.concatenate([Ji.ravel(), Jp.ravel()]), (r, c)), shape=(m, x.size))

    x0 = np.concatenate([intr0[free], poses0.ravel()])
    if sparse:
        r = least_squares(resid, x0, jac=jac_sparse, method="trf", tr_solver="lsmr", x_scale="jac", xtol=1e-15, ftol=1e-15, gtol=1e-15,
                          max_nfev=100)
    else:
        r = least_squares(resid, x0, jac=jac, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=500)
    intr, poses = unpack(r.x)
    res = resid(r.x)
    n = sum(len(o) for o in objs)
    return {"intr": intr, "rms": float(np.sqrt(np.sum(res ** 2) / n)), "rvecs": poses[:, :3], "tvecs": poses[:, 3:], "start": intr0}


def intr_of_result(res):
    return intr_of(res["K"], res["dist"])


# ---- the device's Levenberg-Marquardt restated, for any projection (the fisheye model's is tests/fisheye_ref.py's)
class Problem:
    """The cost the solvers minimise: residuals over the free intrinsics and every view's pose. project(intr, rvec, tvec, obj) -> (n, 2),
    complex-safe; intr0 / poses0: the start; free: mask of the free intrinsics; aspect: fx = aspect * fy is kept when it is not None."""

    def __init__(self, project, objs, imgs, intr0, poses0, free, aspect=None):
        self.project, self.intr0, self.poses0, self.aspect = project, np.asarray(intr0, np.float64), np.asarray(poses0, np.float64), aspect
        self.free = np.asarray(free, bool)
        self.nf, self.V = int(self.free.sum()), len(objs)
        self.o64 = [np.asarray(o, np.float64) for o in objs]
        self.m64 = [np.asarray(m, np.float64) for m in imgs]
        self.rows = np.cumsum([0] + [2 * len(o) for o in objs])
        self.npoints = sum(len(o) for o in objs)
        self.x0 = np.concatenate([self.intr0[self.free], self.poses0.ravel()])

    def unpack(self, x):
        intr = self.intr0.astype(x.dtype)
        intr[self.free] = x[:self.nf]
        if self.aspect is not None:
            intr[0] = self.aspect * intr[1]
        return intr, x[self.nf:].reshape(self.V, 6)

    def resid(self, x):
        intr, poses = self.unpack(x)
        return np.concatenate([(self.project(intr, p[:3], p[3:], o) - m).ravel() for o, m, p in zip(self.o64, self.m64, poses)])

    def jac(self, x):
        """complex-step derivatives, exact to rounding"""
        step = 1e-30
        J = np.zeros((self.rows[-1], x.size))
        for j in range(self.nf):
            xc = x.astype(complex)
            xc[j] += 1j * step
            J[:, j] = self.resid(xc).imag / step
        for k in range(6):
            xc = x.astype(complex)
            xc[self.nf + k::6] += 1j * step
            col = self.resid(xc).imag / step
            for v in range(self.V):
                J[self.rows[v]:self.rows[v + 1], self.nf + 6 * v + k] = col[self.rows[v]:self.rows[v + 1]]
        return J

    def result(self, x, **more):
        intr, poses = self.unpack(x)
        res = self.resid(x)
        per_view = np.array([np.sqrt(np.sum(res[a:b] ** 2) / ((b - a) // 2)) for a, b in zip(self.rows[:-1], self.rows[1:])])
        return dict({"intr": intr, "rms": float(np.sqrt(np.sum(res ** 2) / self.npoints)), "rvecs": poses[:, :3], "tvecs": poses[:, 3:],
                     "per_view_rms": per_view, "start": self.intr0}, **more)


def lm_solve(p, max_iter=30):
    """The device's Levenberg-Marquardt on a Problem, dense: (J^T J + lambda diag(J^T J)) step = J^T r is what the per-view Schur
    elimination solves. CvLevMarq's rule as in lm_device.h: lambda = 10^lg from lg = -3; a candidate whose cost is not larger is taken and
    lg falls by one, else lg rises by one (stop above 16); stop after max_iter accepted steps or when |step| < DBL_EPSILON |parameters|."""
    x, lg, iters = p.x0.copy(), -3, 0
    r = p.resid(x)
    cost = float(r @ r)
    J = p.jac(x)
    while True:
        A, g = J.T @ J, J.T @ r
        A[np.diag_indices_from(A)] *= 1 + 10.0 ** lg
        step = np.linalg.solve(A, g)
        xc = x - step
        rc = p.resid(xc)
        cc = float(rc @ rc)
        if np.isfinite(cc) and cc <= cost:
            full_old = np.concatenate([p.unpack(x)[0], x[p.nf:]])
            full_new = np.concatenate([p.unpack(xc)[0], xc[p.nf:]])
            x, r, cost, lg, iters = xc, rc, cc, max(lg - 1, -16), iters + 1
            if iters >= max_iter or np.linalg.norm(full_new - full_old) < np.finfo(float).eps * np.linalg.norm(full_old):
                break
            J = p.jac(x)
        else:
            lg += 1
            if lg > 16:
                break
    return p.result(x, iterations=iters)


def pinhole_problem(objs, imgs, size, flags=0, K=None, dist=None, perturb=0.0):
    """calibrate_camera's cost from start_values; perturb: every start pose entry moved by a seeded uniform +-perturb (a stand-in for a
    solver whose start poses are not these)."""
    intr0, aspect, poses0 = start_values(objs, imgs, size, flags, K, dist)
    if perturb:
        poses0 = poses0 + np.random.RandomState(99).uniform(-perturb, perturb, poses0.shape)
    return Problem(project, objs, imgs, intr0, poses0, free_of(flags), aspect if flags & 2 else None)


def lm_calibrate(objs, imgs, size, flags=0, K=None, dist=None, max_iter=30, perturb=0.0):
    """lm_solve on the pinhole model: what arucohip_calibrate_camera does, in dense float64"""
    return lm_solve(pinhole_problem(objs, imgs, size, flags, K, dist, perturb), max_iter)


def pose_minimum(obj, img, intr, start, project=project):
    """One view's pose-only minimum with the intrinsics fixed, from start (6): scipy over rvec, tvec -> (6,)"""
    from scipy.optimize import least_squares

    o, m = np.asarray(obj, np.float64), np.asarray(img, np.float64)
    intr = np.asarray(intr, np.float64)

    def resid(x):
        return (project(intr.astype(x.dtype), x[:3], x[3:], o) - m).ravel()

    def jac(x):
        J = np.zeros((2 * len(o), 6))
        for k in range(6):
            xc = x.astype(complex)
            xc[k] += 1e-30j
            J[:, k] = resid(xc).imag / 1e-30
        return J

    return least_squares(resid, np.asarray(start, np.float64), jac=jac, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=500).x


def view_cost(intr, pose, obj, img, project=project):
    """sum of squared residuals of one view in float64"""
    r = project(np.asarray(intr, np.float64), pose[:3], pose[3:], np.asarray(obj, np.float64)) - np.asarray(img, np.float64)
    return float(np.sum(r * r))


# ---- the edge families of tests/test_calib_edges_cpu.py and tests/test_gpu_calib_edges.py
def planar_grid(nx, ny, pitch, z0=0.0):
    """nx * ny points of a centred grid in the plane z = z0, row after row: (nx * ny, 3) float64"""
    ys, xs = np.mgrid[0:ny, 0:nx]
    return np.stack([(xs.ravel() - (nx - 1) / 2) * pitch, (ys.ravel() - (ny - 1) / 2) * pitch, np.full(nx * ny, float(z0))], axis=1)


GRID = (32, 16, 0.009)     # 512 points, 0.279 m x 0.135 m: CALIB_MAX_POINTS of them, about the golden board's size
EDGE_NOISE = 0.2
EDGE_COUNTS = {
    "strides": (4, 5, 7, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512),
    "small": (4, 4, 5, 6, 8, 9, 12, 16, 20, 24, 31, 33),
    "planes": (33, 40, 65, 96, 17, 50, 70, 31),
    "poses": (96,) * 13,    # the seven named rotations, then six ordinary views that condition k2 and k3
    "one": (96,),
    "two": (96, 96),
}
PLANES_Z0 = (0.0, 0.25, -0.1, 0.5, 0.0, 0.03, -0.3, 0.2)
POSES_RVEC = ((0.0, 0.0, 0.0), (0.0, 0.0, np.pi - 1e-4), (0.0, 0.0, np.pi / 2), (1.0, 0.0, 0.0), (0.0, -1.0, 0.1), (0.7, 0.7, 0.0), (-0.6, 0.5, 3.0))
ONE_GUESS = (K_TRUE * np.array([[1.02, 1, 1], [1, 0.98, 1], [1, 1, 1]]), np.array([-0.1, 0.05, 0.0, 0.0, 0.01]))
EDGE_FLAGS = {"strides": 0, "small": FLAGS["FIX_K3"], "planes": 0, "poses": 0, "two": FLAGS["FIX_K3"],
              "one": FLAGS["USE_INTRINSIC_GUESS"] | FLAGS["FIX_PRINCIPAL_POINT"] | FLAGS["ZERO_TANGENT_DIST"] | FLAGS["FIX_K2"] | FLAGS["FIX_K3"]}
ALL_FIXED = sum(FLAGS[k] for k in ("USE_INTRINSIC_GUESS", "FIX_FOCAL_LENGTH", "FIX_PRINCIPAL_POINT", "ZERO_TANGENT_DIST", "FIX_K1", "FIX_K2", "FIX_K3"))
# name: (flags, K, dist, family): the flag cases of the edge tests, each on a family of uneven counts
FLAG_CASES = {
    "fix_k1": (FLAGS["FIX_K1"], None, None, "strides"),
    "fix_k2": (FLAGS["FIX_K2"], None, None, "strides"),
    "two_free": (FLAGS["FIX_ASPECT_RATIO"] | FLAGS["FIX_PRINCIPAL_POINT"] | FLAGS["ZERO_TANGENT_DIST"] | FLAGS["FIX_K2"] | FLAGS["FIX_K3"],
                 np.array([[700.0, 0, 0], [0, 695.0, 0], [0, 0, 1]]), None, "strides"),
    "nothing_free": (ALL_FIXED, ONE_GUESS[0], ONE_GUESS[1], "small"),
}
_EDGE_SEED = {name: 4101 + 17 * i for i, name in enumerate(EDGE_COUNTS)}
_edge = {}


def _subset(rng, n, grid):
    """n of the grid's points, in grid order: its four outer corners for n = 4; else a random subset that spans at least 60 % of the
    grid either way (drawn again otherwise), so that a handful of points still fixes a homography"""
    nx, ny = GRID[0], GRID[1]
    if n == 4:
        return np.array([0, nx - 1, nx * (ny - 1), nx * ny - 1])
    if n == len(grid):
        return np.arange(n)
    ext = grid[:, :2].max(0) - grid[:, :2].min(0)
    while True:
        idx = np.sort(rng.choice(len(grid), n, replace=False))
        if np.all(grid[idx, :2].max(0) - grid[idx, :2].min(0) >= 0.6 * ext):
            return idx


def edge_views(name):
    """One named family of calibration views at the solver's edges (computed once): dict with objs / imgs (float32 lists), counts, flags, K
    / dist (the guess, or None), and what made them: poses [V, 6], exact (the float64 projection plus the 0.2 px noise, before rounding).
      strides  counts around every stride of the kernels (4 .. 512), subsets of the 512-point grid
      small    few points per view, FIX_K3
      planes   every view in its own plane z = z0
      poses    the golden board frontal, turned by about pi and pi / 2 about the axis, and tilted by about 1 rad
      one      a single tilted view, only fx, fy and k1 free, from a guess
      two      two views"""
    if name in _edge:
        return _edge[name]
    rng = np.random.RandomState(_EDGE_SEED[name])
    counts = EDGE_COUNTS[name]
    intr = intr_of(K_TRUE, DIST_TRUE)
    grid = planar_grid(*GRID)
    objs, imgs, poses, exact = [], [], [], []
    for v, n in enumerate(counts):
        if name in ("poses", "one", "two"):
            obj = board_points()
        else:
            obj = grid[_subset(rng, n, grid)].copy()
        if name == "planes":
            obj[:, 2] = np.float32(PLANES_Z0[v])
        obj = obj.astype(np.float32)
        if name == "poses" and v < len(POSES_RVEC):
            r = np.array(POSES_RVEC[v])
            t = np.array([rng.uniform(-0.03, 0.03), rng.uniform(-0.02, 0.02), rng.uniform(0.6, 0.75)])
        elif name in ("one", "two"):
            r = np.array([(0.5, -0.4, 0.1), (-0.45, 0.5, -0.2)][v])
            t = np.array([(0.02, -0.01, 0.6), (-0.03, 0.02, 0.7)][v])
        else:
            r = rng.uniform(-0.45, 0.45, 3) * np.array([1, 1, 0.3])
            t = np.array([rng.uniform(-0.06, 0.06), rng.uniform(-0.04, 0.04), rng.uniform(0.55, 0.8)])
        t = t - float(obj[0, 2]) * rodrigues(r)[:, 2]   # the plane stays where z0 = 0 would put it: only t knows about z0
        m = project(intr, r, t, obj.astype(np.float64)) + rng.normal(0, EDGE_NOISE, (n, 2))
        objs.append(obj), imgs.append(m.astype(np.float32)), poses.append(np.concatenate([r, t])), exact.append(m)
    K, dist = ONE_GUESS if name == "one" else (None, None)
    _edge[name] = {"name": name, "objs": objs, "imgs": imgs, "counts": counts, "flags": EDGE_FLAGS[name], "K": K, "dist": dist,
                   "poses": np.array(poses), "exact": exact}
    return _edge[name]


def scaled_diff(got_intr, ref_intr, dist_scale=1.0):
    """|got - ref| in the units of test_gpu_calib.assert_matches_scipy: f and c relative, distortion coefficients against max(|k|, 1)"""
    ref_intr = np.asarray(ref_intr, np.float64)
    scale = np.concatenate([np.abs(ref_intr[:4]), np.maximum(np.abs(ref_intr[4:]), dist_scale)])
    return np.abs(np.asarray(got_intr, np.float64) - ref_intr) / scale


_ref = {}


def edge_reference(name, flags=None, K=None, dist=None):
    """scipy's minimum of a family (with the family's own flags and guess, or the given ones), computed once"""
    key = (name, flags, None if K is None else tuple(np.ravel(K)), None if dist is None else tuple(np.ravel(dist)))
    if key not in _ref:
        fam = edge_views(name)
        if flags is None:
            flags, K, dist = fam["flags"], fam["K"], fam["dist"]
        _ref[key] = scipy_calibrate(fam["objs"], fam["imgs"], SIZE, flags=flags, K=K, dist=dist)
    return _ref[key]
