"""numpy restatement of the two planar pose solutions of a square marker (infinitesimal plane-based pose estimation, Collins and
Bartoli, IJCV 2014), the analytic step only (refine = 0). Written from the method's description, independently of the device code:
SVD / lstsq where the device code uses closed forms and normal equations. Shared by test_planar_cpu.py and test_gpu_planar.py."""
import numpy as np

K_DEFAULT = np.array([[1000.0, 0.0, 640.0], [0.0, 1000.0, 360.0], [0.0, 0.0, 1.0]])
MARKER_SIZE = 0.1


def object_points(size=MARKER_SIZE):
    """Marker::getObjectPoints: (-,-), (-,+), (+,+), (+,-), centred, z = 0."""
    h = float(np.float32(np.float64(np.float32(size)) / 2.0))
    return np.array([[-h, -h, 0.0], [-h, h, 0.0], [h, h, 0.0], [h, -h, 0.0]])


def rodrigues(r):
    r = np.asarray(r, np.float64)
    th = np.linalg.norm(r)
    if th < 1e-300:
        return np.eye(3)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def rodrigues_inv(R):
    """Rotation matrix -> rotation vector (angles below pi)."""
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.linalg.norm(w) / 2.0
    c = np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)
    th = np.arctan2(s, c)
    if s < 1e-12:
        if c > 0:
            return np.zeros(3)
        # angle pi: the axis from the symmetric part
        A = (R + np.eye(3)) / 2.0
        i = int(np.argmax(np.diag(A)))
        k = A[:, i] / np.sqrt(A[i, i])
        return th * k
    return w / (2.0 * s) * th


def brown_project(P, R, t, K, dist):
    """cv::projectPoints: pinhole + Brown model (k1 k2 p1 p2 k3 k4 k5 k6, zero padded)."""
    d = np.zeros(8)
    if dist is not None:
        d[:len(dist)] = np.asarray(dist, np.float64)
    Xc = P @ R.T + t
    x, y = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
    r2 = x * x + y * y
    rad = (1 + d[0] * r2 + d[1] * r2 ** 2 + d[4] * r2 ** 3) / (1 + d[5] * r2 + d[6] * r2 ** 2 + d[7] * r2 ** 3)
    xd = x * rad + 2 * d[2] * x * y + d[3] * (r2 + 2 * x * x)
    yd = y * rad + d[2] * (r2 + 2 * y * y) + 2 * d[3] * x * y
    return np.stack([K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]], axis=1)


def undistort(px, K, dist):
    """cv::undistortPoints without R / P: five fixed-point iterations of the inverse Brown model."""
    d = np.zeros(8)
    if dist is not None:
        d[:len(dist)] = np.asarray(dist, np.float64)
    x0 = (px[:, 0] - K[0, 2]) / K[0, 0]
    y0 = (px[:, 1] - K[1, 2]) / K[1, 1]
    x, y = x0.copy(), y0.copy()
    for _ in range(5):
        r2 = x * x + y * y
        icd = (1 + ((d[7] * r2 + d[6]) * r2 + d[5]) * r2) / (1 + ((d[4] * r2 + d[1]) * r2 + d[0]) * r2)
        dx = 2 * d[2] * x * y + d[3] * (r2 + 2 * x * x)
        dy = d[2] * (r2 + 2 * y * y) + 2 * d[3] * x * y
        x, y = (x0 - dx) * icd, (y0 - dy) * icd
    return np.stack([x, y], axis=1)


def homography(obj_xy, uv):
    """Least squares, 8 unknowns, H22 = 1."""
    rows, rhs = [], []
    for (X, Y), (u, v) in zip(obj_xy, uv):
        rows.append([X, Y, 1, 0, 0, 0, -u * X, -u * Y]), rhs.append(u)
        rows.append([0, 0, 0, X, Y, 1, -v * X, -v * Y]), rhs.append(v)
    A, b = np.array(rows), np.array(rhs)
    # column scaling keeps the system well conditioned for a 0.1 m marker (the device code normalises both point sets)
    sc = np.linalg.norm(A, axis=0)
    h = np.linalg.lstsq(A / sc, b, rcond=None)[0] / sc
    return np.append(h, 1.0).reshape(3, 3)


def planar_poses(corners_px, K=K_DEFAULT, dist=None, size=MARKER_SIZE):
    """Both solutions for one marker: dict with R [2,3,3], rvec [2,3], tvec [2,3], rms [2] (ordered, sigma = +1 first on a tie);
    None for input the method cannot solve."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    px = np.asarray(corners_px, np.float64).reshape(4, 2)
    P = object_points(size)
    uv = undistort(px, K, dist)
    H = homography(P[:, :2], uv)
    p, q = H[0, 2], H[1, 2]
    J = np.array([[H[0, 0] - H[2, 0] * p, H[0, 1] - H[2, 1] * p], [H[1, 0] - H[2, 0] * q, H[1, 1] - H[2, 1] * q]])
    s = np.sqrt(p * p + q * q + 1.0)
    hpq = np.hypot(p, q)
    Rv = np.eye(3) if hpq == 0 else rodrigues(np.array([q, -p, 0.0]) / hpq * np.arccos(1.0 / s))
    B = (np.array([[1.0, 0.0, -p], [0.0, 1.0, -q]]) @ Rv.T)[:, :2]
    A = np.linalg.solve(B, J)
    gamma = np.linalg.svd(A, compute_uv=False)[0]
    if not (gamma > 0 and np.isfinite(gamma)):
        return None
    R22 = A / gamma
    b = np.eye(2) - R22.T @ R22
    c = np.array([np.sqrt(max(b[0, 0], 0.0)), np.sqrt(max(b[1, 1], 0.0))])
    if b[0, 1] < 0:
        c[1] = -c[1]
    Rs, ts, es = [], [], []
    for sg in (1.0, -1.0):
        c1 = np.array([R22[0, 0], R22[1, 0], sg * c[0]])
        c2 = np.array([R22[0, 1], R22[1, 1], sg * c[1]])
        R = Rv.T @ np.stack([c1, c2, np.cross(c1, c2)], axis=1)
        rows, rhs = [], []
        for Pi, (u, v) in zip(P, uv):
            rp = R @ Pi
            rows.append([1, 0, -u]), rhs.append(u * rp[2] - rp[0])
            rows.append([0, 1, -v]), rhs.append(v * rp[2] - rp[1])
        t = np.linalg.lstsq(np.array(rows), np.array(rhs), rcond=None)[0]
        if not t[2] > 0:
            return None
        e = brown_project(P, R, t, K, dist) - px
        Rs.append(R), ts.append(t), es.append(np.sqrt(np.mean(np.sum(e * e, axis=1))))
    order = [1, 0] if es[1] < es[0] else [0, 1]
    Rs, ts, es = [Rs[i] for i in order], [ts[i] for i in order], [es[i] for i in order]
    return {"R": np.array(Rs), "rvec": np.array([rodrigues_inv(R) for R in Rs]), "tvec": np.array(ts), "rms": np.array(es)}


def rotate_x_axis(rvec):
    """aruco::rotateXAxis: the rotation times a quarter turn about x, in float (cv::Matx33f), the vector kept at float precision."""
    R = rodrigues(rvec).astype(np.float32)
    ang = np.float32(np.pi / 2)
    cs, sn = np.float32(np.cos(np.float64(ang))), np.float32(np.sin(np.float64(ang)))
    RX = np.array([[1, 0, 0], [0, cs, -sn], [0, sn, cs]], np.float32)
    Q = np.zeros((3, 3), np.float32)
    for i in range(3):
        for j in range(3):
            Q[i, j] = np.float32(np.float32(R[i, 0] * RX[0, j] + R[i, 1] * RX[1, j]) + R[i, 2] * RX[2, j])
    U, _, Vt = np.linalg.svd(Q.astype(np.float64))   # cv::Rodrigues takes the nearest rotation of its input
    return rodrigues_inv(U @ Vt).astype(np.float32).astype(np.float64)


def generate_poses(n, seed=20141):
    """Seeded poses of a 0.1 m marker facing the camera: tilted 0.1 - 1.2 rad about a random axis, t in +-0.3 x +-0.2 x 0.4 - 1.5 m.
    Returns (R [n,3,3], t [n,3], corners [n,4,2] float64 pixels through K_DEFAULT without distortion)."""
    rng = np.random.default_rng(seed)
    Rs, ts, cs = [], [], []
    P = object_points()
    for _ in range(n):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        R = rodrigues(axis * rng.uniform(0.1, 1.2))
        t = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2), rng.uniform(0.4, 1.5)])
        Rs.append(R), ts.append(t), cs.append(brown_project(P, R, t, K_DEFAULT, None))
    return np.array(Rs), np.array(ts), np.array(cs)
