"""NumPy restatement of the reference's ChromaticMask / EMClassifier (src/chromaticmask.cpp), in the reference's float / double
operation order, with the EM fit the library defines ("Board occlusion mask"). The device kernels (k_chromatic.hip)
are checked against it: geometry to 1e-9 relative, cell maps, histograms and masks byte for byte, the EM to 1e-12 relative (exp and
log of the device and of the host libm may differ in the last bit). No OpenCV: the OpenCV calls are restated here."""
import math

import numpy as np

F32 = np.float32
CELL = 20
NELEM = 200
DBL_EPS = np.finfo(np.float64).eps
FLT_EPS = float(np.finfo(np.float32).eps)


def neighbour_lists(mc, nc):
    """setParams :178-187 with the reference's unsigned loops: max(j - 1, 0u) wraps at j == 0, so the first row and column get
    empty lists; the bounds use mc for both loops."""
    U = 1 << 32
    out = []
    for j in range(nc):
        for i in range(mc):
            lst = []
            nj = max((j - 1) % U, 0)
            while nj < min(mc, j + 1):
                ni = max((i - 1) % U, 0)
                while ni < min(mc, i + 1):
                    lst.append(nj * mc + ni)
                    ni += 1
                nj += 1
            out.append(lst)
    return out


def centers(mc, nc):
    """_centers[j * mc + i] = (i + 0.5, j + 0.5)"""
    return [(F32(i + 0.5), F32(j + 0.5)) for j in range(nc) for i in range(mc)]


def board_corners(obj, info_type, marker_size=-1.0):
    """setParams(.., BC, markersize) :122-165 (info_type 1 = METERS): 4 x 3 float32 corners"""
    o = np.asarray(obj, F32).reshape(-1, 4, 3)
    if info_type != 1 and marker_size == -1:
        raise ValueError("invalid markersize")
    ms = F32(marker_size)
    if info_type == 1:
        d = o[0, 0] - o[0, 1]
        ms = F32(math.sqrt(float(d[0]) * float(d[0]) + float(d[1]) * float(d[1]) + float(d[2]) * float(d[2])))
    mn, mx = o[0, 0].copy(), o[0, 0].copy()
    for i in range(len(o)):
        for j in range(4):
            p = o[i, j]
            if p[0] <= mn[0] and p[1] <= mn[1]:
                mn = p.copy()
            if p[0] >= mx[0] and p[1] >= mx[1]:
                mx = p.copy()
    pix = float(abs(F32(ms / (o[0, 1, 0] - o[0, 0, 0]))))
    mn[0], mn[1] = F32(float(mn[0]) * pix), F32(float(mn[1]) * pix)
    mx[0], mx[1] = F32(float(mx[0]) * pix), F32(float(mx[1]) * pix)
    return np.array([mn, [mn[0], mx[1], 0], mx, [mx[0], mn[1], 0]], F32)


def rodrigues(r):
    r = np.asarray(r, float)
    th = math.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    if th < DBL_EPS:
        return np.eye(3)
    c, s = math.cos(th), math.sin(th)
    c1 = 1.0 - c
    u = r / th
    rrt = np.outer(u, u)
    rx = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    return c * np.eye(3) + c1 * rrt + s * rx


def project(pts3, rvec, tvec, K, dist):
    """cv::projectPoints (k1 k2 p1 p2 k3), result as Point2f"""
    K = np.asarray(K, F32).reshape(3, 3).astype(float)
    k = np.zeros(8)
    if dist is not None:
        d = np.asarray(dist, F32).reshape(-1).astype(float)
        k[: len(d)] = d
    R = rodrigues(rvec)
    out = []
    for X in np.asarray(pts3, F32).astype(float):
        p = R @ X + np.asarray(tvec, float)
        z = 1.0 / p[2] if p[2] else 1.0
        x, y = p[0] * z, p[1] * z
        r2 = x * x + y * y
        r4, r6 = r2 * r2, r2 * r2 * r2
        cd = (1 + k[0] * r2 + k[1] * r4 + k[4] * r6) / (1 + k[5] * r2 + k[6] * r4 + k[7] * r6)
        xd = x * cd + k[2] * 2 * x * y + k[3] * (r2 + 2 * x * x)
        yd = y * cd + k[2] * (r2 + 2 * y * y) + k[3] * 2 * x * y
        out.append((xd * K[0, 0] + K[0, 2], yd * K[1, 1] + K[1, 2]))
    return np.array(out).astype(F32)


def perspective_transform(src, dst):
    """cv::getPerspectiveTransform on Point2f corners (products src * dst in float), solved by Gaussian elimination"""
    src, dst = np.asarray(src, F32).reshape(4, 2), np.asarray(dst, F32).reshape(4, 2)
    A, b = np.zeros((8, 8)), np.zeros(8)
    for i in range(4):
        sx, sy, dx, dy = src[i, 0], src[i, 1], dst[i, 0], dst[i, 1]
        A[i, 0] = A[i + 4, 3] = sx
        A[i, 1] = A[i + 4, 4] = sy
        A[i, 2] = A[i + 4, 5] = 1
        A[i, 6], A[i, 7] = -sx * dx, -sy * dx
        A[i + 4, 6], A[i + 4, 7] = -sx * dy, -sy * dy
        b[i], b[i + 4] = dx, dy
    try:
        x = np.linalg.solve(A, b)
    except np.linalg.LinAlgError:
        x = np.zeros(8)
    return np.append(x, 1.0).reshape(3, 3)


def geometry(corners3d, rvec, tvec, K, dist, mc, nc, W, H):
    """(corners2d, H_train, H_classify, rect [x0, y0, x1, y1)) of calculateGridImage / classify2"""
    c2 = project(corners3d, rvec, tvec, K, dist)
    ex, ey = F32(CELL) * F32(mc) - F32(1), F32(CELL) * F32(nc) - F32(1)
    Ht = perspective_transform(c2, [[0, 0], [ex, 0], [ex, ey], [0, ey]])
    Hc = perspective_transform(c2, [[0, 0], [mc - 1, 0], [mc - 1, nc - 1], [0, nc - 1]])
    return c2, Ht, Hc, rect(c2, W, H)


def rect(c2, W, H):
    """cv::boundingRect of float points (floor of the extremes, width = floor(max) - floor(min) + 1), then fitRectToSize as the
    reference writes it: x, y clamped to 0 first, the end = clamped start + unclamped width, clipped to the frame. Returns
    [x0, x1) x [y0, y1) (empty when x1 <= x0 or y1 <= y0)."""
    x, y = math.floor(float(c2[:, 0].min())), math.floor(float(c2[:, 1].min()))
    w, h = math.floor(float(c2[:, 0].max())) - x + 1, math.floor(float(c2[:, 1].max())) - y + 1
    x, y = max(x, 0), max(y, 0)
    endx, endy = min(x + w, W), min(y + h, H)
    return x, y, endx, endy


def cell_map(Ht, mc, nc, W, H):
    """calculateGridImage :222-268: cv::perspectiveTransform (double) of every 2x2 block's top-left pixel, / 20 in float, inside
    Rect(0, 0, mc, nc), cell (uint)y * nc + (uint)x; an odd last row / column stays 0"""
    m = np.asarray(Ht, float).reshape(9)
    by, bx = np.mgrid[0:H // 2, 0:W // 2]
    fx, fy = (2 * bx).astype(F32).astype(float), (2 * by).astype(F32).astype(float)
    w = fx * m[6] + fy * m[7] + m[8]
    ok = np.abs(w) > FLT_EPS
    with np.errstate(divide="ignore", invalid="ignore"):
        wi = 1.0 / w
        px = np.where(ok, ((fx * m[0] + fy * m[1] + m[2]) * wi).astype(F32), F32(0))
        py = np.where(ok, ((fx * m[3] + fy * m[4] + m[5]) * wi).astype(F32), F32(0))
    px, py = px / F32(CELL), py / F32(CELL)
    inside = (F32(0) <= px) & (px < F32(mc)) & (F32(0) <= py) & (py < F32(nc))
    cell = np.where(inside, py, 0).astype(np.uint32) * np.uint32(nc) + np.where(inside, px, 0).astype(np.uint32)
    v = np.where(inside, (cell.astype(np.uint8) + 1).astype(np.uint8), 0).astype(np.uint8)
    out = np.zeros((H, W), np.uint8)
    for dy in (0, 1):
        for dx in (0, 1):
            out[dy:2 * (H // 2):2, dx:2 * (W // 2):2] = v
    return out


def raw_hist(cellmap, img, ncell, mask=None):
    """the samples of every cell: pixels whose cell map (times the mask, saturating, for update) is not 0"""
    cm = cellmap.astype(np.int32)
    if mask is not None:
        cm = np.minimum(cm * mask.astype(np.int32), 255)
    sel = cm != 0
    idx = (cm[sel] - 1) * 256 + img[sel].astype(np.int32)
    return np.bincount(idx, minlength=ncell * 256).reshape(ncell, 256)[:ncell].astype(np.int64)


def hist_count(raw):
    """EMClassifier::train :60-90: the smoothed histogram (3 / 2 / 1), normalised, histCount = (unsigned)(200 * hist)"""
    r = np.asarray(raw, np.int64)
    h = 3 * r.copy()
    h[:-1] += 2 * r[1:]
    h[1:] += 2 * r[:-1]
    h[:-2] += r[2:]
    h[2:] += r[:-2]
    h = h.astype(float)
    s = _wsum(h)
    if s == 0:
        return np.zeros(256, np.int64)
    return np.trunc(200.0 * (h / s)).astype(np.int64)


def _wsum(t):
    """the device's sum over 256 levels: lane l adds levels 4l .. 4l+3 in order, then a butterfly over the 64 lanes"""
    t = np.asarray(t, float).reshape(64, 4)
    s = t[:, 0] + t[:, 1]
    s = s + t[:, 2]
    s = s + t[:, 3]
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[idx ^ o]
    return float(s[0])


def _logl(v, pi, mu, var):
    if not pi > 0:
        return np.full(v.shape, -np.inf)
    d = v - mu
    return np.log(pi) - 0.5 * np.log(2.0 * math.pi * var) - d * d / (2.0 * var)


def em_fit(raw, thresh, prob=None):
    """EMClassifier::train on one cell's raw-sample histogram: (prob[256], inside[256], fitted, histCount). Fewer than 10
    discretised samples: the model passed in (0.5 for a fresh classifier) is kept and fitted is False."""
    c = hist_count(raw).astype(float)
    p0 = np.full(256, 0.5) if prob is None else np.asarray(prob, float)
    N = _wsum(c)
    if N < 10:
        return p0, p0 > thresh, False, c.astype(np.int64)
    # 2-means start: least S2 - S1^2 / S0 per side over every split, ties to the lowest
    T0 = T1 = T2 = 0.0
    for v in range(256):
        T0 += c[v]
        T1 += c[v] * v
        T2 += c[v] * v * v
    A0 = A1 = A2 = 0.0
    best, split, bA0, bA1 = math.inf, -1, 0.0, 0.0
    for v in range(255):
        A0 += c[v]
        A1 += c[v] * v
        A2 += c[v] * v * v
        B0, B1, B2 = T0 - A0, T1 - A1, T2 - A2
        if A0 > 0 and B0 > 0:
            sse = (A2 - A1 * A1 / A0) + (B2 - B1 * B1 / B0)
            if sse < best:
                best, split, bA0, bA1 = sse, v, A0, A1
    pi = [bA0 / T0, (T0 - bA0) / T0]
    mu = [bA1 / bA0, (T1 - bA1) / (T0 - bA0)]
    nk = [N - (T0 - bA0), T0 - bA0]
    lv = np.arange(256, dtype=float)
    var = []
    for k in range(2):
        d = lv - mu[k]
        side = (lv <= split) if k == 0 else (lv > split)
        var.append(max(_wsum(np.where(side, c * d * d, 0.0)) / nk[k], DBL_EPS))
    for _ in range(3):
        l0, l1 = _logl(lv, pi[0], mu[0], var[0]), _logl(lv, pi[1], mu[1], var[1])
        m = np.maximum(l0, l1)
        e0, e1 = np.exp(l0 - m), np.exp(l1 - m)
        s = e0 + e1
        rk = [e0 / s, e1 / s]
        for k in range(2):
            w = c * rk[k]
            W, S = _wsum(w), _wsum(w * lv)
            pi[k] = W / N
            if not W > 0:
                continue
            mu[k] = S / W
            d = lv - mu[k]
            var[k] = max(_wsum(w * d * d) / W, DBL_EPS)
    em_fit.params = (pi, mu, var)   # the final mixture, for the tests
    l0, l1 = _logl(lv, pi[0], mu[0], var[0]), _logl(lv, pi[1], mu[1], var[1])
    m = np.maximum(l0, l1)
    p = np.exp(m + np.log(np.exp(l0 - m) + np.exp(l1 - m)))
    return p, p > thresh, True, c.astype(np.int64)


def close3(sparse):
    """3x3 rect MORPH_CLOSE; outside the image nothing dilates or erodes"""
    H, W = sparse.shape
    p = np.zeros((H + 2, W + 2), np.uint8)
    p[1:-1, 1:-1] = sparse
    d = np.zeros((H, W), np.uint8)
    for dy in range(3):
        for dx in range(3):
            d |= p[dy:dy + H, dx:dx + W]
    q = np.ones((H + 2, W + 2), np.uint8)
    q[1:-1, 1:-1] = d
    e = np.ones((H, W), np.uint8)
    for dy in range(3):
        for dx in range(3):
            e &= q[dy:dy + H, dx:dx + W]
    return e


def classify(cellmap, inside, img):
    """classify :317-354 (inside: [ncell][256] bool) with the close"""
    sparse = np.zeros(img.shape, np.uint8)
    sel = cellmap != 0
    sparse[sel] = inside[cellmap[sel].astype(np.int64) - 1, img[sel]].astype(np.uint8)
    return close3(sparse)


def classify2_samples(Hc, rc, prob, img, mc, nc, thresh):
    """classify2 :372-438 before the close: the sparse image, and the per-sample details (x, y, cx, cy, set) for quirk tests"""
    H, W = img.shape
    Hf = np.asarray(Hc, float).reshape(9).astype(F32)
    x0, y0, x1, y1 = rc
    xs, ys = [], []
    ny = 0
    for y in range(y0, y1, 2):
        sx = x0 + ny % 2
        xx = np.arange(sx, x1, 2)
        xs.append(xx)
        ys.append(np.full(xx.shape, y))
        ny += 1
    sparse = np.zeros((H, W), np.uint8)
    if not xs:
        return sparse, None
    x, y = np.concatenate(xs), np.concatenate(ys)
    fx, fy = x.astype(F32), y.astype(F32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        den = fx * Hf[6] + fy * Hf[7] + Hf[8]
        inv = (1.0 / den.astype(float)).astype(F32)
        px = inv * (fx * Hf[0] + fy * Hf[1] + Hf[2])
        py = inv * (fx * Hf[3] + fy * Hf[4] + Hf[5])
        vx, vy = px.astype(float) + 0.5, py.astype(float) + 0.5
        ok = (vx > -1.0) & (vx < mc) & (vy > -1.0) & (vy < nc)
        cx = np.where(ok, np.trunc(np.where(ok, vx, 0)), -1).astype(np.int64)
        cy = np.where(ok, np.trunc(np.where(ok, vy, 0)), -1).astype(np.int64)
        full = ok & (cx > 0) & (cy > 0)
        g = img[y, x].astype(np.int64)
        P = np.asarray(prob, float)
        cxs, cys = np.where(full, cx, 1), np.where(full, cy, 1)
        nb = [(cys - 1) * mc + cxs - 1, (cys - 1) * mc + cxs, cys * mc + cxs - 1, cys * mc + cxs]
        pr = np.zeros(x.shape, F32)
        tw = np.zeros(x.shape, F32)
        for k in range(4):
            ckx, cky = F32(k % mc) + F32(0.5), F32(k // mc) + F32(0.5)
            dist = np.abs(px - ckx) + np.abs(py - cky)
            w = F32(2) - dist
            w = w * w
            tw = tw + w
            pr = (pr.astype(float) + w.astype(float) * P[nb[k], g]).astype(F32)
        pr = pr / tw
        hit = full & (pr.astype(float) > thresh)
    sparse[y[hit], x[hit]] = 1
    return sparse, {"x": x, "y": y, "cx": cx, "cy": cy, "ok": ok, "full": full, "set": hit, "px": px, "py": py}


def classify2(Hc, rc, prob, img, mc, nc, thresh):
    return close3(classify2_samples(Hc, rc, prob, img, mc, nc, thresh)[0])


class ChromaticMask:
    """The reference class over the functions above (one 8-bit plane per call)."""

    def __init__(self, mc, nc, thresh, K, dist, W, H, corners):
        self.mc, self.nc, self.thresh, self.K, self.dist, self.W, self.H = mc, nc, thresh, K, dist, W, H
        self.corners = np.asarray(corners, F32).reshape(4, 3)
        n = mc * nc
        self.prob = np.full((n, 256), 0.5)
        self.trained = np.zeros(n, bool)
        self.cellmap = np.zeros((H, W), np.uint8)
        self.mask = np.zeros((H, W), np.uint8)
        self.valid = False

    def geometry(self, rvec, tvec):
        return geometry(self.corners, rvec, tvec, self.K, self.dist, self.mc, self.nc, self.W, self.H)

    def _fit(self, raw, min_raw=0):
        fitted = np.zeros(len(raw), np.int32)
        counts = np.zeros(raw.shape, np.int64)
        for i in range(len(raw)):
            if min_raw and not raw[i].sum() > min_raw:
                fitted[i] = -1
                continue
            p, _, ok, c = em_fit(raw[i], self.thresh, self.prob[i])
            counts[i] = c
            if ok:
                self.prob[i], self.trained[i], fitted[i] = p, True, 1
        return fitted, counts

    def train(self, img, rvec=None, tvec=None, Ht=None):
        if Ht is None:
            Ht = self.geometry(rvec, tvec)[1]
        self.cellmap = cell_map(Ht, self.mc, self.nc, self.W, self.H)
        raw = raw_hist(self.cellmap, img, self.mc * self.nc)
        self.valid = True
        return raw, self._fit(raw)

    def classify(self, img, rvec=None, tvec=None, Ht=None):
        if Ht is None:
            Ht = self.geometry(rvec, tvec)[1]
        self.cellmap = cell_map(Ht, self.mc, self.nc, self.W, self.H)
        self.mask = classify(self.cellmap, self.prob > self.thresh, img)
        return self.mask

    def classify2(self, img, rvec=None, tvec=None, Hc=None, rc=None):
        if Hc is None:
            _, _, Hc, rc = self.geometry(rvec, tvec)
        self.mask = classify2(Hc, rc, self.prob, img, self.mc, self.nc, self.thresh)
        return self.mask

    def update(self, img):
        raw = raw_hist(self.cellmap, img, self.mc * self.nc, self.mask)
        return raw, self._fit(raw, 50)
