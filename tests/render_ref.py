"""NumPy restatement of the mesh rendering rule that include/arucohip.h states at arucohip_render_markers_batch: integers (int64) where the
rule is integer, float64 in the rule's order elsewhere. It also reports what is knife-edge, so that a comparison with the device can be
exact everywhere else: sin, cos and sqrt may differ in the last place between two libraries, and only a value that sits on a rounding
boundary can turn that into another byte."""
import numpy as np

CULL_BACK, UNLIT = 1, 2
LIMIT = 1048576.0


def rodrigues(rvec):
    r = np.asarray(rvec, np.float64)
    theta = np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    if theta < np.finfo(np.float64).eps:
        return np.eye(3)
    c, s = np.cos(theta), np.sin(theta)
    c1, it = 1.0 - c, 1.0 / theta
    x, y, z = r[0] * it, r[1] * it, r[2] * it
    rrt = np.array([[x * x, x * y, x * z], [x * y, y * y, y * z], [x * z, y * z, z * z]])
    rx = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return c * np.eye(3) + c1 * rrt + s * rx


def transform(vertices, R, t, s):
    """camera-frame points [n][3] of float32 vertices, step 1"""
    v = np.asarray(vertices, np.float32).astype(np.float64) * np.float64(s)
    X, Y, Z = v[:, 0], v[:, 1], v[:, 2]
    return np.stack([((R[i, 0] * X + R[i, 1] * Y) + R[i, 2] * Z) + t[i] for i in range(3)], axis=1)


def project(cam, K, dist):
    """pixels (px, py) of camera-frame points through K (float32) and the Brown model"""
    K = np.asarray(K, np.float32).astype(np.float64).reshape(3, 3)
    k = np.zeros(8)
    if dist is not None:
        d = np.asarray(dist, np.float32).astype(np.float64).ravel()
        k[:len(d)] = d
    with np.errstate(all="ignore"):
        z = np.where(cam[:, 2] != 0, 1.0 / cam[:, 2], 1.0)
        x, y = cam[:, 0] * z, cam[:, 1] * z
        r2 = x * x + y * y
        r4 = r2 * r2
        r6 = r4 * r2
        a1, a2, a3 = 2 * x * y, r2 + 2 * x * x, r2 + 2 * y * y
        cdist = 1 + k[0] * r2 + k[1] * r4 + k[4] * r6
        icd = 1.0 / (1 + k[5] * r2 + k[6] * r4 + k[7] * r6)
        xd = x * cdist * icd + k[2] * a1 + k[3] * a2
        yd = y * cdist * icd + k[2] * a3 + k[3] * a1
        return xd * K[0, 0] + K[0, 2], yd * K[1, 1] + K[1, 2]


def gray_of(b, g, r):
    return (b * 1868 + g * 9617 + r * 4899 + 8192) >> 14


def _near_half(v, tol):
    return np.abs((v - np.floor(v)) - 0.5) < tol


def render(frame, instances, K, dist, vertices, triangles, colors=None, flags=CULL_BACK, opacity=255, ambient=64, light=(0.0, 0.0, -1.0),
           color=(0, 200, 0), mask=None):
    """frame: uint8 [H][W] or [H][W][3]; instances: (rvec, tvec, s) in slot order. Returns (the painted frame, info): info["painted"] the
    pixels a triangle covers (mask and opacity aside), info["fragile_depth"] those whose two largest iz lie within 1e-9 relative,
    info["fragile_vertex"] / info["vertex_coords"] and info["fragile_shade"] / info["shaded"] the knife-edge counts and their totals,
    info["owner"] the (instance, triangle) that owns each painted pixel, -1 elsewhere."""
    H, W = frame.shape[:2]
    vertices = np.asarray(vertices, np.float32).reshape(-1, 3)
    triangles = np.asarray(triangles, np.int64).reshape(-1, 3)
    lf = np.asarray(light, np.float32).astype(np.float64)
    l = lf / np.sqrt((lf[0] * lf[0] + lf[1] * lf[1]) + lf[2] * lf[2])
    best = np.zeros((H, W))
    second = np.full((H, W), -np.inf)
    painted = np.zeros((H, W), bool)
    col = np.zeros((H, W, 3), np.int64)
    owner = np.full((H, W, 2), -1, np.int64)
    info = {"fragile_vertex": 0, "vertex_coords": 0, "fragile_shade": 0, "shaded": 0}
    for ii, (rvec, tvec, s) in enumerate(instances):
        cam = transform(vertices, rodrigues(rvec), np.asarray(tvec, np.float64), s)
        px, py = project(cam, K, dist)
        with np.errstate(all="ignore"):
            ok = (cam[:, 2] > 0) & (np.abs(px) <= LIMIT) & (np.abs(py) <= LIMIT)
        X = np.where(ok, np.rint(np.where(ok, px, 0) * 16), 0).astype(np.int64)
        Y = np.where(ok, np.rint(np.where(ok, py, 0) * 16), 0).astype(np.int64)
        info["vertex_coords"] += 2 * int(ok.sum())
        info["fragile_vertex"] += int(_near_half(px[ok] * 16, 1e-3).sum() + _near_half(py[ok] * 16, 1e-3).sum())
        with np.errstate(all="ignore"):
            izv = 1.0 / cam[:, 2]
        for ti, tri in enumerate(triangles):
            if (tri < 0).any() or (tri >= len(vertices)).any() or not ok[tri].all():
                continue
            a, b, c = (int(v) for v in tri)
            A = (X[b] - X[a]) * (Y[c] - Y[a]) - (Y[b] - Y[a]) * (X[c] - X[a])
            if A == 0 or ((flags & CULL_BACK) and A > 0):
                continue
            q = 255
            if not flags & UNLIT:
                u, v = cam[b] - cam[a], cam[c] - cam[a]
                n = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])
                ln = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
                d = (n[0] * l[0] + n[1] * l[1]) + n[2] * l[2]
                if A > 0:
                    d = -d
                with np.errstate(all="ignore"):
                    lam = d / ln
                if not lam > 0:
                    lam = 0.0
                arg = ambient + (255 - ambient) * lam
                info["shaded"] += 1
                info["fragile_shade"] += int(_near_half(np.float64(arg), 1e-6))
                q = min(max(int(np.rint(arg)), 0), 255)
            base = color if colors is None else colors[ti]
            C = [(int(base[k]) * q + 127) // 255 for k in range(3)]
            if A < 0:
                b, c, A = c, b, -A
            x0, x1 = max(-((-min(X[a], X[b], X[c])) // 16), 0), min(max(X[a], X[b], X[c]) // 16, W - 1)
            y0, y1 = max(-((-min(Y[a], Y[b], Y[c])) // 16), 0), min(max(Y[a], Y[b], Y[c]) // 16, H - 1)
            if x0 > x1 or y0 > y1:
                continue
            Py, Px = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.int64) * 16
            cover = np.ones(Px.shape, bool)
            E = []
            for i, j in ((b, c), (c, a), (a, b)):
                dx, dy = X[j] - X[i], Y[j] - Y[i]
                e = dx * (Py - Y[i]) - dy * (Px - X[i])
                owns = dy < 0 or (dy == 0 and dx > 0)
                cover &= (e >= 0) if owns else (e > 0)
                E.append(e.astype(np.float64))
            if not cover.any():
                continue
            Af = np.float64(A)
            iz = ((E[0] / Af) * izv[a] + (E[1] / Af) * izv[b]) + (E[2] / Af) * izv[c]
            sl = (slice(y0, y1 + 1), slice(x0, x1 + 1))
            was, bst, sec = painted[sl], best[sl], second[sl]
            take = cover & (~was | (iz > bst))
            lose = cover & ~take
            second[sl] = np.where(take & was, bst, np.where(lose, np.maximum(sec, iz), sec))
            best[sl] = np.where(take, iz, bst)
            painted[sl] = was | cover
            col[sl] = np.where(take[..., None], np.array(C, np.int64), col[sl])
            owner[sl] = np.where(take[..., None], np.array([ii, ti], np.int64), owner[sl])
    with np.errstate(all="ignore"):
        info["fragile_depth"] = painted & (np.abs(best - second) <= 1e-9 * np.abs(best))
    info["painted"], info["owner"] = painted, owner
    out = frame.copy()
    write = painted if mask is None else painted & (np.asarray(mask) != 0)
    if frame.ndim == 2:
        C = gray_of(col[..., 0], col[..., 1], col[..., 2])
        out[write] = ((C * opacity + frame.astype(np.int64) * (255 - opacity) + 127) // 255)[write].astype(np.uint8)
    else:
        out[write] = ((col * opacity + frame.astype(np.int64) * (255 - opacity) + 127) // 255)[write].astype(np.uint8)
    return out, info


def marker_instances(markers, count, scale=1.0):
    """the instances of one frame's marker list (MARKER_DTYPE records): the first min(count, cap) markers that have a pose"""
    n = min(int(count), len(markers))
    return [(m["rvec"], m["tvec"], np.float64(np.float32(scale)) * np.float64(m["ssize"])) for m in markers[:max(n, 0)] if m["has_pose"]]


def board_instances(board, scale=1.0):
    return [(board["rvec"], board["tvec"], np.float64(np.float32(scale)))] if board["has_pose"] else []
