"""Plane compositing in numpy float64: the rule include/arucohip.h states at arucohip_composite_plane_batch, line for line, and the map of
arucohip_board_composite_batch. numpy's float64 operations are IEEE and unfused, as the library's are. The sampler, the plane map and the
window are tests/rectify_ref.py's."""
import numpy as np

from tests.rectify_ref import board_window, plane_map, sample  # noqa: F401  (board_window: for the callers of this module)


def rays(width, height, K=None, dist=None):
    """Step 3 for every frame pixel: (x, y) as float64 [height][width]."""
    v, u = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    if K is None:
        return u, v
    Kf = np.asarray(K, np.float32).reshape(9).astype(np.float64)
    fx, fy, cx, cy = Kf[0], Kf[4], Kf[2], Kf[5]
    with np.errstate(all="ignore"):
        ifx, ify = 1.0 / fx, 1.0 / fy
        x0, y0 = (u - cx) * ifx, (v - cy) * ify
        if dist is None or len(dist) == 0:
            return x0, y0
        k = np.zeros(8, np.float64)
        d = np.asarray(dist, np.float32).reshape(-1).astype(np.float64)
        k[:d.size] = d
        x, y = x0, y0
        for _ in range(5):
            r2 = x * x + y * y
            ic = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
            dx = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x)
            dy = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y
            x, y = (x0 - dx) * ic, (y0 - dy) * ic
    return x, y


def positions(N, width, height, K=None, dist=None):
    """Steps 3-4: (s * 32, t * 32 as float64 [height][width], ok: False where step 4 leaves the pixel untouched)."""
    N = np.asarray(N, np.float64).reshape(9)
    x, y = rays(width, height, K, dist)
    with np.errstate(all="ignore"):
        S = (N[0] * x + N[1] * y) + N[2]
        T = (N[3] * x + N[4] * y) + N[5]
        Q = (N[6] * x + N[7] * y) + N[8]
        ok = Q > 0                      # False for NaN as well
        s, t = S / Q, T / Q
        ok = ok & np.isfinite(s) & np.isfinite(t)
        return s * 32, t * 32, ok


def fixed(q, ok):
    """Step 5's integer: rint (ties to even) of the clamped s * 32; 0 where ok is False."""
    with np.errstate(all="ignore"):
        return np.rint(np.clip(np.where(ok, q, 0.0), -2147483648.0, 2147483647.0)).astype(np.int64)


def composite(frame, tex, N, K=None, dist=None, valid=True, opacity=255, mask=None):
    """One frame of arucohip_composite_plane_batch: (the painted frame, painted bool [H][W]). frame: uint8 [H][W] or [H][W][3]; tex: uint8
    [th][tw] or [th][tw][C] with C the frame's channels or one more (alpha last); mask: uint8 [H][W] or None."""
    H, W = frame.shape[:2]
    cn = 1 if frame.ndim == 2 else frame.shape[2]
    t3 = tex if tex.ndim == 3 else tex[:, :, None]
    th, tw, tcn = t3.shape
    assert tcn in (cn, cn + 1) and 0 <= opacity <= 255
    out = frame.copy()
    if not valid:
        return out, np.zeros((H, W), bool)
    qs, qt, ok = positions(N, W, H, K, dist)
    if mask is not None:
        ok = ok & (np.asarray(mask) != 0)
    i_s, i_t = fixed(qs, ok), fixed(qt, ok)
    painted = ok & (i_s >= 0) & (i_s <= 32 * (tw - 1)) & (i_t >= 0) & (i_t <= 32 * (th - 1))
    smp = sample(t3, qs, qt, painted).astype(np.int64)                  # step 6, every channel of the texture
    A = smp[:, :, cn] if tcn == cn + 1 else np.full((H, W), 255, np.int64)
    w = (A * opacity + 127) // 255
    painted = painted & (w > 0)
    fr = (frame if frame.ndim == 3 else frame[:, :, None]).astype(np.int64)
    blend = (smp[:, :, :cn] * w[:, :, None] + fr * (255 - w[:, :, None]) + 127) // 255
    o3 = out if out.ndim == 3 else out[:, :, None]
    o3[painted] = blend[painted].astype(np.uint8)
    return out, painted


def inverse_map(M):
    """(N as 9 float64, valid): the signed adjugate of M, products unfused; a zero map when det is zero or not finite."""
    M = np.asarray(M, np.float64).reshape(9)
    with np.errstate(all="ignore"):
        N = np.array([M[4] * M[8] - M[5] * M[7], M[2] * M[7] - M[1] * M[8], M[1] * M[5] - M[2] * M[4],
                      M[5] * M[6] - M[3] * M[8], M[0] * M[8] - M[2] * M[6], M[2] * M[3] - M[0] * M[5],
                      M[3] * M[7] - M[4] * M[6], M[1] * M[6] - M[0] * M[7], M[0] * M[4] - M[1] * M[3]])
        det = (M[0] * N[0] + M[1] * N[3]) + M[2] * N[6]
    if not np.isfinite(det) or det == 0:
        return np.zeros(9), 0
    return (-N if det < 0 else N), 1


def board_map(rvec, tvec, has_pose, win):
    """(N, valid, M) of arucohip_board_composite_batch for one board: rectify_ref.plane_map's M inverted."""
    M, ok = plane_map(rvec, tvec, has_pose, win)
    if not ok:
        return np.zeros(9), 0, M
    N, valid = inverse_map(M)
    return N, valid, M
