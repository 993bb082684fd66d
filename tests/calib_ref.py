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


def homography(obj, img):
    """normalised DLT plane (X, Y) -> pixel, h33 = 1"""
    X, m = obj[:, :2].astype(np.float64), img.astype(np.float64)
    cM, cm = X.mean(0), m.mean(0)
    sM, sm = 1 / np.abs(X - cM).mean(0), 1 / np.abs(m - cm).mean(0)
    Xn, mn = (X - cM) * sM, (m - cm) * sm
    rows, rhs = [], []
    for (a, b), (x, y) in zip(Xn, mn):
        rows += [[a, b, 1, 0, 0, 0, -x * a, -x * b], [0, 0, 0, a, b, 1, -y * a, -y * b]]
        rhs += [x, y]
    h = np.linalg.lstsq(np.array(rows), np.array(rhs), rcond=None)[0]
    H0 = np.append(h, 1).reshape(3, 3)
    Tm = np.array([[1 / sm[0], 0, cm[0]], [0, 1 / sm[1], cm[1]], [0, 0, 1]])
    TM = np.array([[sM[0], 0, -cM[0] * sM[0]], [0, sM[1], -cM[1] * sM[1]], [0, 0, 1]])
    H = Tm @ H0 @ TM
    return H / H[2, 2]


def start_values(objs, imgs, size, flags=0, K=None, dist=None):
    """OpenCV's planar start: principal point at the image centre, fx, fy from the vanishing points of every view
    (initIntrinsicParams2D), distortion 0, pose from H and K; or K / dist with USE_INTRINSIC_GUESS."""
    Kin = np.zeros((3, 3)) if K is None else np.asarray(K, np.float64).reshape(3, 3)
    aspect = Kin[0, 0] / Kin[1, 1] if Kin[0, 0] > 0 and Kin[1, 1] > 0 else 1.0
    if flags & 1:
        intr = intr_of(Kin, dist if dist is not None else np.zeros(5))
    else:
        cx, cy = (size[0] - 1) * 0.5, (size[1] - 1) * 0.5
        A, b = [], []
        for o, m in zip(objs, imgs):
            H = homography(o, m)
            H[0] -= H[2] * cx
            H[1] -= H[2] * cy
            h, v = H[:, 0], H[:, 1]
            d1, d2 = (h + v) * 0.5, (h - v) * 0.5
            h, v, d1, d2 = h / np.linalg.norm(h), v / np.linalg.norm(v), d1 / np.linalg.norm(d1), d2 / np.linalg.norm(d2)
            A += [[h[0] * v[0], h[1] * v[1]], [d1[0] * d2[0], d1[1] * d2[1]]]
            b += [-h[2] * v[2], -d1[2] * d2[2]]
        f = np.linalg.lstsq(np.array(A), np.array(b), rcond=None)[0]
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
        H = np.linalg.solve(Km, homography(o, m))
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


def scipy_calibrate(objs, imgs, size, flags=0, K=None, dist=None, sparse=False):
    """least_squares over the free intrinsics (masked as the device solver masks them) and every view's rvec, tvec. sparse: a
    sparse Jacobian and an iterative trust-region solve, for thousands of views."""
    from scipy.optimize import least_squares

    intr0, aspect, poses0 = start_values(objs, imgs, size, flags, K, dist)
    free = np.ones(9, bool)
    for bit, idx in ((2, [0]), (16, [0, 1]), (4, [2, 3]), (8, [6, 7]), (32, [4]), (64, [5]), (128, [8])):
        if flags & bit:
            free[idx] = False
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
