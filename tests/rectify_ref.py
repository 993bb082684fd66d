"""Plane rectification in numpy float64: the rule include/arucohip.h states at arucohip_warp_plane_batch, line for line, and the map
builder and window of arucohip_board_rectify_batch. numpy's float64 operations are IEEE and unfused, as the library's are."""
import numpy as np


def positions(M, out_w, out_h, K=None, dist=None):
    """Steps 1-4 for every output pixel: (px * 32, py * 32 as float64 [out_h][out_w], ok: False where the pixel is 0 by steps 1 or 4)."""
    M = np.asarray(M, np.float64).reshape(9)
    v, u = np.meshgrid(np.arange(out_h, dtype=np.float64), np.arange(out_w, dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):
        X = (M[0] * u + M[1] * v) + M[2]
        Y = (M[3] * u + M[4] * v) + M[5]
        W = (M[6] * u + M[7] * v) + M[8]
        ok = W > 0                      # False for NaN as well
        x, y = X / W, Y / W
        if K is None:
            px, py = x, y
        else:
            Kf = np.asarray(K, np.float32).reshape(9).astype(np.float64)
            k = np.zeros(8, np.float64)
            if dist is not None:
                d = np.asarray(dist, np.float32).reshape(-1).astype(np.float64)
                k[:d.size] = d
            fx, fy, u0, v0 = Kf[0], Kf[4], Kf[2], Kf[5]
            k1, k2, p1, p2, k3, k4, k5, k6 = k
            x2, y2 = x * x, y * y
            r2, _2xy = x2 + y2, 2 * x * y
            kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
            px = fx * (x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)) + u0
            py = fy * (y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy) + v0
        ok = ok & np.isfinite(px) & np.isfinite(py)
        return px * 32, py * 32, ok


def sample(src, qx, qy, ok):
    """Steps 5-6. src: uint8 [H][W] or [H][W][cn]; qx, qy = px * 32, py * 32."""
    img = src if src.ndim == 3 else src[:, :, None]
    H, W, cn = img.shape
    with np.errstate(all="ignore"):
        iu = np.rint(np.clip(np.where(ok, qx, 0.0), -2147483648.0, 2147483647.0)).astype(np.int64)   # rint: ties to even
        iv = np.rint(np.clip(np.where(ok, qy, 0.0), -2147483648.0, 2147483647.0)).astype(np.int64)
    sx, ax, sy, ay = iu >> 5, iu & 31, iv >> 5, iv & 31
    pad = np.zeros((H + 2, W + 2, cn), np.int64)    # taps outside the source count 0
    pad[1:-1, 1:-1] = img
    inside = ok & (sx >= -1) & (sx < W) & (sy >= -1) & (sy < H)
    cx, cy = np.clip(sx, -1, W - 1) + 1, np.clip(sy, -1, H - 1) + 1
    w00, w01, w10, w11 = (32 - ax) * (32 - ay) * 32, ax * (32 - ay) * 32, (32 - ax) * ay * 32, ax * ay * 32
    acc = (pad[cy, cx] * w00[..., None] + pad[cy, cx + 1] * w01[..., None] + pad[cy + 1, cx] * w10[..., None] +
           pad[cy + 1, cx + 1] * w11[..., None] + (1 << 14)) >> 15
    out = np.where(inside[..., None], acc, 0).astype(np.uint8)
    return out if src.ndim == 3 else out[:, :, 0]


def warp_plane(src, M, out_w, out_h, K=None, dist=None, valid=True):
    """One frame of arucohip_warp_plane_batch."""
    shape = (out_h, out_w) + src.shape[2:]
    if not valid:
        return np.zeros(shape, np.uint8)
    qx, qy, ok = positions(M, out_w, out_h, K, dist)
    return sample(src, qx, qy, ok)


def rodrigues(r):
    """pnp_device.h's rodrigues_vec2mat."""
    r = np.asarray(r, np.float64)
    theta = np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    if theta < np.finfo(np.float64).eps:
        return np.eye(3)
    c, s = np.cos(theta), np.sin(theta)
    x, y, z = r * (1.0 / theta)
    rrt = np.array([[x * x, x * y, x * z], [x * y, y * y, y * z], [x * z, y * z, z * z]])
    rx = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return c * np.eye(3) + (1.0 - c) * rrt + s * rx


def plane_map(rvec, tvec, has_pose, win):
    """(M as 9 float64, valid) of plane_maps_kernel. win: dict or object with x0, y0, ux, uy, vx, vy (float32 values)."""
    g = (lambda n: float(win[n])) if isinstance(win, dict) else (lambda n: float(getattr(win, n)))
    R = rodrigues(rvec)
    t = np.asarray(tvec, np.float64)
    M = np.zeros((3, 3))
    with np.errstate(all="ignore"):
        for i in range(3):
            M[i, 0] = R[i, 0] * g("ux") + R[i, 1] * g("uy")
            M[i, 1] = R[i, 0] * g("vx") + R[i, 1] * g("vy")
            M[i, 2] = (R[i, 0] * g("x0") + R[i, 1] * g("y0")) + t[i]
    ok = bool(has_pose) and bool(np.all(np.isfinite(M)))
    return (M.reshape(9) if ok else np.zeros(9)), int(ok)


def board_window(obj, info_type, marker_size, px_per_unit, margin, flip_y=False):
    """arucohip_rectify_board_window as a dict (out_width, out_height, x0, y0, ux, uy, vx, vy with float32 values)."""
    o = np.asarray(obj, np.float32).reshape(-1, 3)
    unit = 1.0
    if info_type == 0 and marker_size > 0:
        d = (o[0] - o[1]).astype(np.float64)      # Point3f difference in float, the norm in double
        unit = float(np.float32(marker_size)) / np.sqrt(np.sum(d * d))
    p = o[:, :2].astype(np.float64) * unit
    lo, hi = p.min(axis=0), p.max(axis=0)
    ppu, m = float(np.float32(px_per_unit)), float(np.float32(margin))
    step = 1.0 / ppu
    size = []
    for k in range(2):
        px = (hi[k] - lo[k] + 2 * m) * ppu
        size.append(int(max(1.0, np.ceil(px - 1e-6 * px))))
    f = np.float32
    return {"out_width": size[0], "out_height": size[1], "x0": f(lo[0] - m + step / 2), "ux": f(step), "uy": f(0), "vx": f(0),
            "y0": f(hi[1] + m - step / 2) if flip_y else f(lo[1] - m + step / 2), "vy": f(-step) if flip_y else f(step)}


# ---- the round trip: a painted board, seen through a camera, detected, posed and rectified back onto its own pixels
RT_IDS = [471, 5, 26, 99, 182, 253]
RT_GRID, RT_SIDE, RT_DIST = (3, 2), 70, 14      # a panel of 3 x 2 markers of 70 px (cells of 10 px), 14 px apart: 238 x 154
RT_MARKER_M = 0.07                              # the marker side in metres: a board pixel is a millimetre
RT_W, RT_H = 640, 480
RT_K = np.array([[600, 0, 320], [0, 600, 240], [0, 0, 1]], np.float32)
RT_POSES = [((0.0, 0.0, 0.0), (0.0, 0.0, 0.42)), ((0.25, -0.15, 0.05), (0.01, -0.005, 0.45)), ((-0.2, 0.3, -0.1), (-0.01, 0.01, 0.44))]


def round_trip_frames(obj):
    """Three 640 x 480 frames of the board with object points obj [6][4][3] (board pixels), uint8 [3][480][640]."""
    from aruco_amd import synth

    unit = RT_MARKER_M / RT_SIDE
    frames = []
    for k, (rvec, tvec) in enumerate(RT_POSES):
        fr, _ = synth.render_board(RT_IDS, obj, RT_K.astype(float), np.array(rvec), np.array(tvec), RT_W, RT_H, np.random.RandomState(100 + k), unit=unit)
        frames.append(fr.numpy())
    return np.stack(frames)


def round_trip_mismatches(board_img, rectified):
    """Cell centres (49 per marker) at which the rectified image, thresholded at 128, differs from the painted board."""
    pitch = RT_SIDE + RT_DIST
    bad = []
    for my in range(RT_GRID[1]):
        for mx in range(RT_GRID[0]):
            for cy in range(7):
                for cx in range(7):
                    x, y = mx * pitch + 10 * cx + 5, my * pitch + 10 * cy + 5
                    if (rectified[y, x] >= 128) != (board_img[y, x] >= 128):
                        bad.append((mx, my, cx, cy))
    return bad
