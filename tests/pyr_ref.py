"""Reference of MarkerDetector::pyrDown(level) (helper, no test).

pyr_down(gray): cv::pyrDown for 8-bit single-channel images as the exact integer definition of aruco_amd/csrc/k_pyrdown.hip
(OpenCV's documentation; no OpenCV exists here to check it against):
    Wo = (W + 1) / 2, Ho = (H + 1) / 2, k = {1, 4, 6, 4, 1}
    R(p, n): n == 1 -> 0; otherwise reflect p at 0 and n - 1 until 0 <= p < n          (BORDER_REFLECT_101)
    h(y, xo)    = sum_t k[t] * src(y, R(2 xo - 2 + t, W))
    dst(yo, xo) = (sum_t k[t] * h(R(2 yo - 2 + t, H), xo) + 128) >> 8

chain(full, level, ...): the whole option, composed from the oracle's stage functions only: the rectangle stage on the reduced image,
everything else on the frame, and the tail of MarkerDetector::detect restated here.
"""
import numpy as np

from oracle import orc

KERNEL = (1, 4, 6, 4, 1)
LINES, SUBPIX, HARRIS, NONE = 3, 2, 1, 0


def reflect101(p, n):
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * n - 2 - p
    return p


def pyr_down(gray):
    g = np.ascontiguousarray(gray, dtype=np.uint8).astype(np.int32)
    H, W = g.shape
    Wo, Ho = (W + 1) // 2, (H + 1) // 2
    h = np.zeros((H, Wo), np.int32)
    for t, k in enumerate(KERNEL):
        cols = np.array([reflect101(2 * xo - 2 + t, W) for xo in range(Wo)], np.int64)
        h += np.int32(k) * g[:, cols]
    v = np.zeros((Ho, Wo), np.int32)
    for t, k in enumerate(KERNEL):
        rows = np.array([reflect101(2 * yo - 2 + t, H) for yo in range(Ho)], np.int64)
        v += np.int32(k) * h[rows, :]
    return ((v + 128) >> 8).astype(np.uint8)


def pyr_down_levels(gray, levels):
    g = np.ascontiguousarray(gray, dtype=np.uint8)
    for _ in range(levels):
        g = pyr_down(g)
    return g


def pyr_down_brute(gray):
    """The definition as a double loop over the output pixels."""
    g = np.asarray(gray, dtype=np.uint8)
    H, W = g.shape
    Wo, Ho = (W + 1) // 2, (H + 1) // 2
    out = np.zeros((Ho, Wo), np.uint8)
    for yo in range(Ho):
        for xo in range(Wo):
            acc = 0
            for ty in range(5):
                y = reflect101(2 * yo - 2 + ty, H)
                hs = 0
                for tx in range(5):
                    hs += KERNEL[tx] * int(g[y, reflect101(2 * xo - 2 + tx, W)])
                acc += KERNEL[ty] * hs
            out[yo, xo] = (acc + 128) >> 8
    return out


def _perimeter(c):
    """src/utils.h:39-46: float accumulator, double norms of float differences."""
    c = np.asarray(c, np.float32)
    s = np.float32(0)
    for i in range(4):
        d = c[i] - c[(i + 1) % 4]
        s = np.float32(float(s) + float(np.sqrt(float(d[0]) * float(d[0]) + float(d[1]) * float(d[1]))))
    return s


def border_rect(W, H, t=0.025):
    """Rect(Point(size) * t, Point(size) * (1 - t)) with cvRound, float32 arithmetic: x0, y0, x1, y1 of [x0, x1) x [y0, y1)."""
    t = np.float32(t)
    x1, y1 = int(np.rint(np.float32(W) * t)), int(np.rint(np.float32(H) * t))
    x2, y2 = int(np.rint(np.float32(W) * (np.float32(1.0) - t))), int(np.rint(np.float32(H) * (np.float32(1.0) - t)))
    return min(x1, x2), min(y1, y2), max(x1, x2), max(y1, y2)


def chain(full, level, K=None, dist=None, size=-1.0, corner_method=LINES, details=None):
    """Markers ({"id", "corners" (4 x 2 float32), "has_pose", "rvec", "tvec"}) of the frame `full` with pyrDown(level).
    details (a dict, optional) receives "reduced", "quads" (every candidate's integer quad in full-frame coordinates, in order) and "ids"."""
    full = np.ascontiguousarray(full, dtype=np.uint8)
    H, W = full.shape
    s = 1 << level
    reduced = pyr_down_levels(full, level)
    o = orc.Oracle(corner_method=corner_method) if corner_method != LINES else orc.Oracle()
    o.detect(reduced)
    cands = o.candidates(with_contour=True)
    det = []
    quads, ids = [], []
    for c in cands:
        q = (c["quad0"] * np.float32(s)).astype(np.float32)
        cid, nrot = orc.fiducial_detect(orc.warp(full, q, 56))
        quads.append(q.copy()), ids.append(cid)
        if cid == -1:
            continue
        corners = q
        if corner_method == LINES:
            corners = orc.refine_lines(c["contour"] * s, q, K, dist)
        det.append({"id": cid, "corners": np.roll(corners, nrot, axis=0).astype(np.float32)})
    if details is not None:
        details.update(reduced=reduced, quads=quads, ids=ids)
    if det and corner_method in (SUBPIX, HARRIS):
        pts = np.concatenate([m["corners"] for m in det]).astype(np.float32)
        win = int(o.get_params().thres_p1)
        pts = orc.corner_subpix(full, pts, win=win) if corner_method == SUBPIX else orc.corner_harris(full, pts)
        for i, m in enumerate(det):
            m["corners"] = pts.reshape(-1, 2)[4 * i:4 * i + 4].copy()
    det.sort(key=lambda m: m["id"])   # stable
    rem = [False] * len(det)
    for i in range(len(det) - 1):
        if det[i]["id"] == det[i + 1]["id"] and not rem[i + 1]:
            if _perimeter(det[i]["corners"]) > _perimeter(det[i + 1]["corners"]):
                rem[i + 1] = True
            else:
                rem[i] = True
    x0, y0, x1, y1 = border_rect(W, H)
    for i, m in enumerate(det):
        p = np.rint(m["corners"].astype(np.float64)).astype(np.int64)
        if not (np.all(p[:, 0] >= x0) and np.all(p[:, 0] < x1) and np.all(p[:, 1] >= y0) and np.all(p[:, 1] < y1)):
            rem[i] = True
    out = [m for i, m in enumerate(det) if not rem[i]]
    for m in out:
        m["has_pose"], m["rvec"], m["tvec"] = 0, np.zeros(3), np.zeros(3)
    if K is not None and size > 0:
        hs = np.float32(size) / np.float32(2)
        obj = np.array([[-hs, -hs, 0], [-hs, hs, 0], [hs, hs, 0], [hs, -hs, 0]], np.float32)
        for m in out:
            ok, r, t = orc.solve_pnp(obj, m["corners"], K, dist)
            m["has_pose"], m["rvec"], m["tvec"] = int(ok), r, t
    return out


# ---- the test frames of the option
CAM_K = [600, 0, 320, 0, 600, 240, 0, 0, 1]
CAM_DIST = [0.05, -0.1, 0.001, 0.001]
CAM_SIZE = 0.05
FRAME_SETS = {"640x480": (640, 480, 4, (100, 160)), "1280x720": (1280, 720, 8, (100, 200))}
_cache = {}


def frames_of(name):
    """(frames [3][H][W] uint8, truth ids per frame, sorted) of a frame set, rendered once per process."""
    if name not in _cache:
        from aruco_amd import synth
        W, H, n, sr = FRAME_SETS[name]
        rng = np.random.RandomState(7)
        frames, truth = [], []
        for _ in range(3):
            lay = synth.frame_layout(rng, W, H, n_markers=n, side_range=sr, margin=40)
            frames.append(np.asarray(synth.render_frame(lay, W, H, rng).numpy(), np.uint8))
            truth.append(sorted(int(m["id"]) for m in lay))
        _cache[name] = (np.stack(frames), truth)
    return _cache[name]


_chains = {}


def chain_cached(name, f, level, cam=False, corner_method=LINES):
    """chain() of frame f of a frame set, computed once per process and shared: (markers, details)."""
    key = (name, f, level, cam, corner_method)
    if key not in _chains:
        frames, _ = frames_of(name)
        d = {}
        m = chain(frames[f], level, CAM_K if cam else None, CAM_DIST if cam else None, CAM_SIZE if cam else -1.0, corner_method, details=d)
        _chains[key] = (m, d)
    return _chains[key]
