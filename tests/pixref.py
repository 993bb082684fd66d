"""Float64 reference of the pixel-domain corner stages and the families of edge cases they are held to.

SUBPIX restates cv::cornerSubPix as MarkerDetector::detect calls it (src/markerdetector.cpp:402-405: window (p1, p1), no dead zone, 8 iterations
or a step below 0.005), HARRIS restates SubPixelCorner::RefineCorner (src/subpixelcorner.cpp:70-189: one iteration, the bounds test that compares
y with the width, the y update without its C * D term, the 8-bit patch of getRectSubPix), LOCKED restates findCornerMaxima
(src/markerdetector.cpp:157-199). Plain numpy; nothing here calls the oracle or the device. Every stage gives

  exact    the algorithm in float64 throughout (weights, patch, mask, sums, update), same control flow and quirks;
  f32path  the same with the float32 roundings of the published code (bilinear weights, 32f patch, mask, position update, err; for LOCKED the
           float32 response arithmetic in the order of oracle/orc_extra.cpp);
  a record of the path `exact` took: per iteration position, det and err, the exit, for LOCKED the best and the runner-up score.

Fragility is decided from `exact` alone (see fragility()). tests/test_pixref_cpu.py pins the oracle on every family, measures ORACLE_WORST_PX
and proves the caps on the fragile shares; tests/test_gpu_pix_edges.py holds the device to `exact` on the same cases."""
import numpy as np

REL_TOL = 1e-4            # the project's corner tolerance, relative to max(|coordinate|, 1)
NONE, HARRIS, SUBPIX = 0, 1, 2
EPS2 = float(np.finfo(np.float64).eps) ** 2
STOP = 0.005
STOP_MARGIN, DET_MARGIN, MAX_MARGIN = 0.02, 1e-6, 1e-5
FRAGILE_CAP = 0.05

# The oracle's worst deviation from `exact` in pixels over every non-fragile case, per method, as `pytest tests/test_pixref_cpu.py -k measured -s`
# prints it. The device is allowed four times that: it makes roundings of the same size at other places (FMA-contracted samples, expf against
# std::exp, a 64-lane tree sum against an in-order one) and no larger ones. Never measured against the device.
ORACLE_WORST_PX = {"subpix": 3.19e-05, "harris": 3.03e-06}
FINE_BOUND_PX = {m: 4.0 * v for m, v in ORACLE_WORST_PX.items()}


def fine_bound(method, want):
    """The bound for one case in pixels: four times the oracle's worst, at least four float32 spacings of the case's largest coordinate, at
    most the project's relative tolerance."""
    top = max(float(np.max(np.abs(want))), 1.0)
    floor = 4.0 * float(np.spacing(np.float32(top)))
    return min(max(FINE_BOUND_PX[method], floor), REL_TOL * top)


def rel_dev(got, want):
    return float(np.max(np.abs(np.asarray(got, np.float64) - want))) / max(float(np.max(np.abs(want))), 1.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# the three stages
# ---------------------------------------------------------------------------------------------------------------------------------
def _weights(T, cx, cy, pw):
    """getRectSubPix: the patch's origin, split into the integer pixel and the bilinear weights, in arithmetic T."""
    ox, oy = T(cx) - T((pw - 1) * 0.5), T(cy) - T((pw - 1) * 0.5)
    ix, iy = int(np.floor(ox)), int(np.floor(oy))
    fa, fb = T(ox - T(ix)), T(oy - T(iy))
    one = T(1)
    return ix, iy, ((one - fa) * (one - fb), fa * (one - fb), (one - fa) * fb, fa * fb)


def _corners4(img, W, H, ix, iy, pw, xmax=None):
    """The four neighbours of every patch pixel, the border replicated by clamping the index."""
    ys, xs = np.clip(iy + np.arange(pw + 1), 0, H - 1), np.clip(ix + np.arange(pw + 1), 0, W - 1 if xmax is None else xmax)
    P = img[np.ix_(ys, xs)]
    return P[:-1, :-1], P[:-1, 1:], P[1:, :-1], P[1:, 1:]


def subpix(img, pt, win, f32=False, flip=None, wrong=None):
    """cv::cornerSubPix on one corner of img [H][W] uint8. flip = j inverts the decision `err > eps` after iteration j (the neighbouring stopping
    point of a fragile_stop case); wrong = clamp | iter7 | ge is a deliberately wrong reading (test_pixref_cpu.py). Returns {"pt", "iters": [{x, y, det, AC, err}], "exit": det | left | maxiter | eps, "reset"}."""
    T = np.float32 if f32 else np.float64
    H, W = img.shape
    ww = 2 * win + 1
    pw = ww + 2
    k = np.arange(-win, win + 1)
    t = k.astype(T) / T(win)
    e = np.exp(-t * t).astype(T)
    mask = (e[:, None] * e[None, :]).astype(np.float64)
    px, py = k[None, :].astype(np.float64), k[:, None].astype(np.float64)
    cT = (T(pt[0]), T(pt[1]))
    cI, it, iters, exit_ = cT, 0, [], None
    while True:
        ix, iy, (a11, a12, a21, a22) = _weights(T, cI[0], cI[1], pw)
        p00, p01, p10, p11 = (p.astype(T) for p in _corners4(img, W, H, ix, iy, pw, W - 2 if wrong == "clamp" else None))
        buf = (p00 * a11 + p01 * a12 + p10 * a21 + p11 * a22).astype(np.float64)
        gx, gy = buf[1:-1, 2:] - buf[1:-1, :-2], buf[2:, 1:-1] - buf[:-2, 1:-1]
        gxx, gxy, gyy = gx * gx * mask, gx * gy * mask, gy * gy * mask
        A, B, C = float(gxx.sum()), float(gxy.sum()), float(gyy.sum())
        bb1, bb2 = float((gxx * px + gxy * py).sum()), float((gxy * px + gyy * py).sum())
        det = A * C - B * B
        if abs(det) <= EPS2:
            iters.append({"x": float(cI[0]), "y": float(cI[1]), "det": det, "AC": A * C, "err": None})
            exit_ = "det"
            break
        scale = 1.0 / det
        nx, ny = T(float(cI[0]) + C * scale * bb1 - B * scale * bb2), T(float(cI[1]) - B * scale * bb1 + A * scale * bb2)
        dx, dy = T(nx - cI[0]), T(ny - cI[1])
        err = float(T(dx * dx) + T(dy * dy))
        cI = (nx, ny)
        iters.append({"x": float(nx), "y": float(ny), "det": det, "AC": A * C, "err": err})
        if nx < 0 or nx >= W or ny < 0 or ny >= H:
            exit_ = "left"
            break
        it += 1
        if not it < (7 if wrong == "iter7" else 8):
            exit_ = "maxiter"
            break
        go_on = err > STOP * STOP
        if flip is not None and flip == it - 1:
            go_on = not go_on
        if not go_on:
            exit_ = "eps"
            break
    reset = bool(abs(cI[0] - cT[0]) > win or abs(cI[1] - cT[1]) > win)
    if wrong == "ge":
        reset = bool(abs(cI[0] - cT[0]) >= win or abs(cI[1] - cT[1]) >= win)
    if reset:
        cI = cT
    return {"pt": np.array([cI[0], cI[1]], np.float64), "iters": iters, "exit": exit_, "reset": reset}


def harris_skipped(pt, W, H):
    """The reference's bounds test: y is compared with the height and with the width."""
    x, y = float(np.float32(pt[0])), float(np.float32(pt[1]))
    return x < 0 or y < 0 or y > H or y > W


def harris(img, pt, f32=False, wrong=None):
    """SubPixelCorner::RefineCorner on one corner: a 17 x 17 patch of getRectSubPix 8u -> 8u (16.16 fixed-point weights, rounded to 8 bits with
    (s + 2^15) >> 16), the 3 x 3 Sobel on it in integers, rows and columns 1..15 weighted by exp(-l^2 / 225)."""
    T = np.float32 if f32 else np.float64
    H, W = img.shape
    win, ps = 15, 17
    start = np.array([T(pt[0]), T(pt[1])], np.float64)
    if harris_skipped(pt, W, H):
        return {"pt": start, "iters": [], "exit": "skipped", "reset": False}
    ix, iy, wts = _weights(T, pt[0], pt[1], ps)
    a11, a12, a21, a22 = (int(np.rint(np.float64(T(w * T(65536))))) for w in wts)
    p00, p01, p10, p11 = (p.astype(np.int64) for p in _corners4(img, W, H, ix, iy, ps))
    loc = ((p00 * a11 + p01 * a12 + p10 * a21 + p11 * a22 + (0 if wrong == "noround" else 1 << 15)) >> 16) & 0xFF
    gx = (loc[:-2, 2:] + 2 * loc[1:-1, 2:] + loc[2:, 2:]) - (loc[:-2, :-2] + 2 * loc[1:-1, :-2] + loc[2:, :-2])    # rows / columns 1..15
    gy = (loc[2:, :-2] + 2 * loc[2:, 1:-1] + loc[2:, 2:]) - (loc[:-2, :-2] + 2 * loc[:-2, 1:-1] + loc[:-2, 2:])
    gx, gy = gx.astype(np.float64), gy.astype(np.float64)
    l = np.arange(-7, 8)
    m1 = np.exp(-(l * l).astype(np.float64) * (1.0 / (win * win))).astype(T)
    mask = (m1[None, :] * m1[:, None]).astype(np.float64)
    lx, ly = l[None, :].astype(np.float64), l[:, None].astype(np.float64)
    dxx, dyy, dxy = gx * gx * mask, gy * gy * mask, gx * gy * mask
    A, B, E = float(dxx.sum()), float(dxy.sum()), float(dyy.sum())
    C, F = float((dxx * lx + dxy * ly).sum()), float((dxy * lx + dyy * ly).sum())
    D = 0.0
    det = A * E - B * B
    ex, ey = T(pt[0]), T(pt[1])
    exit_ = "det"
    if abs(det) > EPS2:
        inv = 1.0 / det
        ystep = (C * E) - (B * F) if wrong == "fixedy" else (A * F) - (C * D)
        ex, ey = T(float(ex) + ((C * E) - (B * F)) * inv), T(float(ey) + ystep * inv)
        exit_ = "step"
    reset = bool(abs(float(start[0]) - float(ex)) > win or abs(float(start[1]) - float(ey)) > win)
    if reset:
        ex, ey = start
    return {"pt": np.array([ex, ey], np.float64), "iters": [{"x": float(ex), "y": float(ey), "det": det, "AC": A * E, "err": None}], "exit": exit_,
            "reset": reset}


def _reflect101(p, n):
    p = np.asarray(p)
    if n == 1:
        return np.zeros_like(p)
    for _ in range(8):      # offsets of one pixel: one reflection is enough but for windows of one or two pixels
        p = np.where(p < 0, -p, p)
        p = np.where(p >= n, 2 * n - 2 - p, p)
    return p


def locked_window(pt, wsize, W, H):
    cx, cy = np.float32(pt[0]), np.float32(pt[1])
    x0, y0 = max(0, int(cx - np.float32(wsize))), max(0, int(cy - np.float32(wsize)))
    x1, y1 = min(W, int(cx + np.float32(wsize))), min(H, int(cy + np.float32(wsize)))
    return x0, y0, x1, y1


def harris_response(img, x0, y0, x1, y1, f32=False):
    """cv::cornerHarris(block 3, aperture 3, k 0.04) of the window: the Sobel taps read the image around the window (REFLECT_101 at the image's
    border only), the 3 x 3 box sums reflect at the window's rim."""
    T = np.float32 if f32 else np.float64
    H, W = img.shape
    rw, rh = x1 - x0, y1 - y0
    scale = T(1.0 / (4.0 * 3.0 * 255.0))
    g = img.astype(T)

    def G(dx, dy):
        return g[np.ix_(_reflect101(np.arange(y0, y1) + dy, H), _reflect101(np.arange(x0, x1) + dx, W))]

    dxm, dxc, dxp = G(1, -1) - G(-1, -1), G(1, 0) - G(-1, 0), G(1, 1) - G(-1, 1)
    dx = (dxm + dxp) * scale + dxc * (T(2) * scale)
    sm = (G(-1, -1) + G(1, -1)) * scale + G(0, -1) * (T(2) * scale)
    sp = (G(-1, 1) + G(1, 1)) * scale + G(0, 1) * (T(2) * scale)
    dy = sp - sm
    ry, rx = [_reflect101(np.arange(rh) + d, rh) for d in (-1, 0, 1)], [_reflect101(np.arange(rw) + d, rw) for d in (-1, 0, 1)]

    def box(a):
        s = np.zeros_like(a)
        for yy in ry:
            r = np.zeros_like(a)
            for xx in rx:
                r = r + a[np.ix_(yy, xx)]
            s = s + r
        return s

    a, b, c = (box(v).astype(np.float64) for v in (dx * dx, dx * dy, dy * dy))
    return (a * c - b * b - 0.04 * (a + c) * (a + c)).astype(T)


def locked(img, pt, wsize, f32=False, wrong=None):
    """findCornerMaxima on one corner. Returns {"pt", "best", "second": (score, raster index), "window", "exit": peak | nopeak}. `exact` sums
    every 4 x 4 block directly (the same sixteen additions wherever the block lies, so that pixel-identical patches tie exactly); f32path goes
    through the double integral like the reference."""
    T = np.float32 if f32 else np.float64
    H, W = img.shape
    x0, y0, x1, y1 = locked_window(pt, wsize, W, H)
    rw, rh = x1 - x0, y1 - y0
    out = {"window": (x0, y0, rw, rh), "best": (0.0, -1), "second": (0.0, -1), "exit": "nopeak", "pt": np.array([-1.0 + x0, -1.0 + y0])}
    if rw <= 0 or rh <= 0:
        return out
    harr = harris_response(img, x0, y0, x1, y1, f32)
    bls = 4
    if rh > 2 * bls and rw > 2 * bls:
        if f32:
            I = np.zeros((rh + 1, rw + 1), np.float64)
            I[1:, 1:] = np.cumsum(np.cumsum(harr.astype(np.float64), axis=1), axis=0)
            blk = I[bls:, bls:] - I[bls:, :-bls] - I[:-bls, bls:] + I[:-bls, :-bls]      # blk[y][x]: the block that starts at (x, y)
        else:
            blk = np.zeros((rh - bls + 1, rw - bls + 1))
            for j in range(bls):
                for i in range(bls):
                    blk = blk + harr[j:j + rh - bls + 1, i:i + rw - bls + 1]
        harr = harr.copy()
        ylast = rh - bls + (1 if wrong == "rim" else 0)
        harr[bls:ylast, bls:rw - bls] = blk[bls:ylast, bls:rw - bls].astype(T)
    ys, xs = np.mgrid[0:rh, 0:rw]
    with np.errstate(divide="ignore", invalid="ignore"):
        d = (np.abs(T(rw // 2) - xs.astype(T)) + np.abs(T(rh // 2) - ys.astype(T))).astype(T) / T(rw + rh if wrong == "den" else rw // 2 + rh // 2)
        wgt = (1.0 - d.astype(np.float64)).astype(T)
        v = (wgt * harr).astype(np.float64).reshape(-1)
    v = np.where(np.isnan(v), -np.inf, v)
    bi = int(np.argmax(v))             # the first of equal maxima in raster order
    if wrong == "lasttie":
        bi = int(v.size - 1 - np.argmax(v[::-1]))
    if not v[bi] > 0:
        return out
    rest = v.copy()
    rest[bi] = -np.inf
    si = int(np.argmax(rest)) if rest.size > 1 else -1
    out.update(best=(float(v[bi]), bi), second=(float(rest[si]), si) if si >= 0 else (0.0, -1), exit="peak",
               pt=np.array([float(bi % rw + x0), float(bi // rw + y0)]))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# images
# ---------------------------------------------------------------------------------------------------------------------------------
def _aa(h, w, f, aa=6):
    ys, xs = np.mgrid[0:h * aa, 0:w * aa]
    return f((xs + 0.5) / aa - 0.5, (ys + 0.5) / aa - 0.5).astype(np.float64).reshape(h, aa, w, aa).mean(axis=(1, 3))


def _noisy(img, seed):
    return np.clip(np.rint(img + np.random.RandomState(seed).normal(0.0, 1.0, img.shape)), 0, 255).astype(np.uint8)


def xcorner(h, w, cx, cy, deg, seed, lo=40, hi=210, kind="x"):
    """Anti-aliased X-corner (two dark quadrants) or L-corner (one) whose corner point is exactly (cx, cy), with sigma = 1 noise."""
    a = np.radians(deg)

    def f(x, y):
        u, v = (x - cx) * np.cos(a) + (y - cy) * np.sin(a), -(x - cx) * np.sin(a) + (y - cy) * np.cos(a)
        return np.where(u * v > 0 if kind == "x" else (u > 0) & (v > 0), lo, hi)

    return _noisy(_aa(h, w, f), seed)


def checker(h, w, deg, period, seed, lo=40, hi=210, ox=3.3, oy=1.7):
    """An anti-aliased checkerboard turned by `deg`: X-corners every `period` pixels, up to the image's edges."""
    a = np.radians(deg)

    def f(x, y):
        u, v = (x - ox) * np.cos(a) + (y - oy) * np.sin(a), -(x - ox) * np.sin(a) + (y - oy) * np.cos(a)
        return np.where((np.floor(u / period) + np.floor(v / period)) % 2 == 0, lo, hi)

    return _noisy(_aa(h, w, f), seed)


TWIN_PATCH = np.array([[210, 200, 40, 50], [190, 205, 45, 60], [35, 55, 215, 195], [42, 48, 188, 207]], np.uint8)   # a corner without a symmetry


def twin_image(h, w, cx, cy, ax, ay, d, flipx, flipy):
    """A constant frame with two copies of TWIN_PATCH in the 62 x 62 window of (cx, cy): at (ax, ay) and (ax + d, ay - d) from the window's
    centre, mirrored about it by the flips. Both lie in one quadrant, so |x| + |y| is the same for every pixel of one and its twin in the other."""
    img = np.full((h, w), 128, np.uint8)
    for ox, oy in ((ax, ay), (ax + d, ay - d)):
        x, y = (-ox - 3 if flipx else ox), (-oy - 3 if flipy else oy)
        img[cy + y:cy + y + 4, cx + x:cx + x + 4] = TWIN_PATCH
    return img


def rim_image(h, w, variant):
    """A frame on which SUBPIX with win = 1 from (w / 2, h / 2) moves by exactly one pixel and stays: a bright column two pixels to the right whose
    left flank is the only x gradient of the 3 x 3 window, in its column px = +1 (so that bb1 == A, summand for summand, and the step is 1 in any
    arithmetic once it is added to the coordinate), and a y gradient in the row py = 0 of the start's column alone (bb2 == 0). From the new point
    the flank is in column px = 0: the second iteration moves nothing. Variants 1..3 mirror the frame and swap its axes: -1 in x, +1 and -1 in y."""
    a, b, d, e = 100, 180, 60, 150
    P = np.full((5, 7), a, np.int64)            # rows y = -2..2, columns x = -3..3 about the start
    P[:, 3 + 2] = b
    for x in (-2, 0):
        P[2 - 1, 3 + x], P[2 + 1, 3 + x] = d, e
    if variant & 1:
        P = P[:, ::-1]
    img = np.full((max(h, w), max(h, w)), a, np.uint8)
    cy, cx = (w // 2, h // 2) if variant & 2 else (h // 2, w // 2)
    img[cy - 2:cy + 3, cx - 3:cx + 4] = P
    return np.ascontiguousarray((img.T if variant & 2 else img)[:h, :w])


_images = {}


def image(key):
    """Every frame of the families, by key, built once."""
    if key not in _images:
        kind = key[0]
        if kind in ("x", "l"):           # (kind, W, H, deg, index)
            _, w, h, deg, i = key
            cx, cy = w / 2 - 0.7 + 0.37 * (i % 3), h / 2 - 0.4 + 0.29 * (i % 4)
            _images[key] = xcorner(h, w, cx, cy, deg, seed=1000 + 7 * i + deg, kind=kind)
        elif kind == "checker":          # ("checker", W, H, deg, period)
            _, w, h, deg, period = key
            _images[key] = checker(h, w, deg, period, seed=77 + deg + period)
        elif kind == "const":
            _images[key] = np.full((key[2], key[1]), 117, np.uint8)
        elif kind == "vstep":
            _images[key] = np.where(np.arange(key[1])[None, :] < key[1] // 2, 40, 210).astype(np.uint8) * np.ones((key[2], 1), np.uint8)
        elif kind == "hstep":
            _images[key] = np.where(np.arange(key[2])[:, None] < key[2] // 2, 40, 210).astype(np.uint8) * np.ones((1, key[1]), np.uint8)
        elif kind == "xramp":
            _images[key] = (20 + np.arange(key[1])[None, :]).astype(np.uint8) * np.ones((key[2], 1), np.uint8)
        elif kind == "yramp":
            _images[key] = (20 + np.arange(key[2])[:, None]).astype(np.uint8) * np.ones((1, key[1]), np.uint8)
        elif kind == "weak":             # a strong X-corner and a faint one `gap` pixels to its right
            _, w, h, gap, i = key
            base = xcorner(h, w, w / 2 - 8.3, h / 2 + 0.2, 10 + 20 * i, seed=500 + i).astype(np.float64)
            faint = xcorner(h, w, w / 2 - 8.3 + gap, h / 2 + 0.2, 35, seed=600 + i, lo=120, hi=124).astype(np.float64) - 122.0
            _images[key] = np.clip(np.rint(base + faint), 0, 255).astype(np.uint8)
        elif kind == "twin":
            _images[key] = twin_image(120, 160, *key[1:])
        elif kind == "rim":
            _images[key] = rim_image(key[2], key[1], key[3])
        else:
            raise KeyError(key)
        _images[key].setflags(write=False)
    return _images[key]


def center(key):
    """The corner point of an x / l image."""
    _, w, h, deg, i = key
    return w / 2 - 0.7 + 0.37 * (i % 3), h / 2 - 0.4 + 0.29 * (i % 4)


def padded(img, stride):
    """The frame with rows of `stride` bytes, the padding filled with a pattern that is not the image's."""
    h, w = img.shape
    ys, xs = np.mgrid[0:h, 0:stride]
    out = ((7 * xs + 13 * ys) % 251).astype(np.uint8)
    out[:, :w] = img
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
WINS = (1, 2, 3, 7, 9, 15)
WSIZES = (1, 3, 4, 5, 7, 15, 31)
ANGLES = (0, 20, 45, 70, 90)
FRAC = ((0.125, 0.5), (0.5, 0.5), (-0.375, 0.25), (0.5, 0.0), (0.875, -0.625))


def case(family, method, key, pt, win=0, wsize=0, stride=None):
    """method: subpix | harris | locked | locked+subpix | locked+harris."""
    return {"family": family, "method": method, "image": key, "pt": (float(np.float32(pt[0])), float(np.float32(pt[1]))), "win": int(win),
            "wsize": int(wsize), "stride": stride, "name": "%s/%s/%s/w%d/l%d/%s/(%g,%g)" % (family, method, "-".join(map(str, key)), win, wsize, stride, pt[0], pt[1])}


def _starts(key, win):
    """Integer starts up to min(win, 2) px from the corner point, and fractional ones in eighths and at x.5."""
    cx, cy = center(key)
    bx, by = int(round(cx)), int(round(cy))
    r = min(win, 2)
    ints = [(0, 0), (r, 0), (-r, r), (1, -r), (-1, -1)]
    return [(bx + dx, by + dy) for dx, dy in ints] + [(bx + fx, by + fy) for fx, fy in FRAC]


def _interior(method, wins):
    out = []
    for win in wins:
        for i, deg in enumerate(ANGLES):
            for kind in ("x", "l") if deg in (20, 45, 70) else ("x",):
                key = (kind, 64, 48, deg, i)
                out += [case("interior", method, key, p, win=win) for p in _starts(key, win if method == "subpix" else 2)]
    return out


def _edge_starts(W, H, win):
    """Starts 0..win + 1 px from each edge and in each image corner; 0, W - 1 and H - 1 themselves among them."""
    ds = sorted({0, 1, 2, win // 2, win, win + 1})
    pts = []
    for d in ds:
        pts += [(d, H // 2 - 3), (W - 1 - d, H // 2 + 2), (W // 2 - 5, d), (W // 2 + 4, H - 1 - d)]
    for d in sorted({0, 1, win}):
        pts += [(d, d), (W - 1 - d, d), (d, H - 1 - d), (W - 1 - d, H - 1 - d)]
    pts += [(0.5, H // 2 + 0.25), (W - 1.5, 3.125), (W // 2 + 0.5, H - 1.0), (0.0, 0.5)]
    return [(min(max(x, 0), W - 1), min(max(y, 0), H - 1)) for x, y in pts]


def amplification(c):
    """How much `exact` magnifies a displacement of a SUBPIX start by 1e-6 px, in x and in y. A start that wanders for 8 iterations between corners
    can magnify it a thousandfold; every arithmetic's first rounding fares the same, so such a start tests nothing (see _settled)."""
    img, base = image(c["image"]), reference(c)["exact"]
    return max(float(np.max(np.abs(subpix(img, (c["pt"][0] + dx, c["pt"][1] + dy), c["win"])["pt"] - base))) for dx, dy in ((1e-6, 0.0), (0.0, 1e-6))) / 1e-6


MAX_AMPLIFICATION = 100.0
dropped = []


def _settled(cases):
    """The starts of a family that are not aimed at a corner, without those whose result `exact` itself cannot tell to better than a hundred times
    a displacement of the start (kept in `dropped` for the record)."""
    out = []
    for c in cases:
        if c["method"] == "subpix" and not returns_start(c) and amplification(c) > MAX_AMPLIFICATION:
            dropped.append(c["name"])
        else:
            out.append(c)
    return out


_cache = {}


def reference(c):
    """{"exact", "f32path", "record", "fragile": set of kinds, "accept": the results a fragile case may also take} of one case, once per process.
    The stride is no part of the key: a padded frame must give what the packed one gives."""
    k = (c["method"], c["image"], c["pt"], c["win"], c["wsize"])
    if k not in _cache:
        _cache[k] = reference_on(image(c["image"]), c["method"], c["pt"], c["win"], c["wsize"])
    return _cache[k]


def _refine(img, method, pt, win, f32, flip=None):
    return subpix(img, pt, win, f32, flip) if method == "subpix" else harris(img, pt, f32)


def reference_on(img, method, pt, win=0, wsize=0):
    """reference() for a corner of any frame (the detection tests apply it to the oracle's candidates)."""
    c = {"pt": (float(np.float32(pt[0])), float(np.float32(pt[1]))), "win": int(win), "wsize": int(wsize)}
    m, pt = method, c["pt"]
    fragile, accept, rec = set(), [], {}
    pre = None
    if m.startswith("locked"):
        pre = locked(img, pt, c["wsize"])
        pre32 = locked(img, pt, c["wsize"], f32=True)
        rec["locked"] = pre
        (b, bi), (s, si) = pre["best"], pre["second"]
        if pre["exit"] == "peak" and si >= 0 and 0 < b - s < MAX_MARGIN * b:
            fragile.add("fragile_max")
            x0, y0, rw, _ = pre["window"]
            accept.append(np.array([float(si % rw + x0), float(si // rw + y0)]))
        if m == "locked":
            return {"exact": pre["pt"], "f32path": pre32["pt"], "record": rec, "fragile": fragile, "accept": accept}
        pt, m2 = tuple(pre["pt"]), m.split("+")[1]
        starts2 = list(accept)
        accept = []
    else:
        m2, starts2 = m, []
    ex, f3 = _refine(img, m2, pt, c["win"], False), _refine(img, m2, pt, c["win"], True)
    rec["refine"] = ex
    for j, it in enumerate(ex["iters"]):
        if it["det"] != 0 and abs(it["det"]) < DET_MARGIN * abs(it["AC"]):
            fragile.add("fragile_det")
        decided = m2 == "subpix" and it["err"] is not None and j + 1 < 8 and not (j == len(ex["iters"]) - 1 and ex["exit"] == "left")
        if decided and abs(np.sqrt(it["err"]) - STOP) <= STOP_MARGIN * STOP and "fragile_stop" not in fragile:
            fragile.add("fragile_stop")
            accept.append(subpix(img, pt, c["win"], False, flip=j)["pt"])
    for s2 in starts2:       # the runner-up pixel of a fragile pre-pass, refined
        accept.append(_refine(img, m2, tuple(s2), c["win"], False)["pt"])
    return {"exact": ex["pt"], "f32path": f3["pt"], "record": rec, "fragile": fragile, "accept": accept}


def returns_start(c):
    """Cases whose result is the start, bit for bit: a skipped HARRIS corner, det == 0, and a reset."""
    r = reference(c)["record"].get("refine")
    return r is not None and (r["exit"] in ("skipped", "det") or r["reset"]) and not c["method"].startswith("locked")


def _pick(pool, want, n):
    out = []
    for c in pool:
        r = reference(c)
        if not r["fragile"] and want(r["record"]["refine"]):
            out.append(c)
        if len(out) == n:
            break
    return out


_families = None


def families():
    global _families
    if _families is not None:
        return _families
    fam = {}
    # ---- SUBPIX and HARRIS
    fam["interior"] = _interior("subpix", WINS) + _interior("harris", (0,))
    border = []
    for W, H in ((64, 48), (48, 64)):
        key = ("checker", W, H, 10, 11)
        for win in WINS:
            border += [case("border", "subpix", key, p, win=win) for p in _edge_starts(W, H, win)]
        border += [case("border", "harris", key, p) for p in _edge_starts(W, H, 8) if not harris_skipped(p, W, H)]
    small = ("checker", 16, 12, 25, 5)
    for win in (15, 9, 7, 2):
        border += [case("border", "subpix", small, p, win=win) for p in ((0, 0), (15, 11), (7, 5), (8.5, 6.25), (15, 0), (0, 11), (3, 10), (12, 1))]
    border += [case("border", "harris", small, p) for p in ((0, 0), (15, 11), (7, 5), (8.5, 6.25), (15, 0), (0, 11), (3, 10), (12, 1))]
    fam["border"] = _settled(border)
    fam["stride"] = [dict(c, family="stride", stride=c["image"][1] + pad, name=c["name"].replace("interior", "stride").replace("/None/", "/+%d/" % pad))
                     for c in fam["interior"] for pad in (3, 13)]
    deg = []
    for key in (("const", 64, 48), ("vstep", 64, 48), ("hstep", 64, 48), ("vstep", 48, 64)):
        W, H = key[1], key[2]
        pts = [(W // 2, H // 2), (W // 2 - 1, H // 2 - 1), (W // 2 + 0.5, H // 2 - 0.375), (W // 2 - 0.125, H // 2 + 0.5), (1, 2), (W - 2, H - 1), (W // 2, 0), (0, H // 2)]
        for win in WINS:
            deg += [case("degenerate", "subpix", key, p, win=win) for p in pts]
        deg += [case("degenerate", "harris", key, p) for p in pts if not harris_skipped(p, W, H)]
    fam["degenerate"] = deg
    # escape: picked from pools by what `exact` did. Reset: a faint corner with a strong one farther than the window away, and windows on noise alone;
    # left: corners of the checkerboard in the outermost pixels.
    pool = []
    for i in range(4):
        for gap in (9, 12):
            key = ("weak", 64, 48, gap, i)
            for win in (2, 3, 7):
                bx, by = int(round(64 / 2 - 8.3 + gap)), int(round(48 / 2 + 0.2))
                pool += [case("escape", "subpix", key, (bx + dx, by + dy), win=win) for dx, dy in ((0, 0), (1, 0), (0, 1), (-1, 1), (2, -1))]
    for W, H in ((64, 48), (48, 64)):
        for degk, period in ((10, 11), (35, 9)):
            key = ("checker", W, H, degk, period)
            for win in (1, 2, 3):
                pool += [case("escape", "subpix", key, p, win=win) for p in [(0, y) for y in range(1, H - 1, 5)] + [(W - 1, y) for y in range(2, H - 1, 5)] +
                         [(x, 0) for x in range(1, W - 1, 5)] + [(x, H - 1) for x in range(2, W - 1, 5)]]
    rim = [case("escape", "subpix", ("rim", W, H, v), (W // 2, H // 2), win=1) for v in range(4) for W, H in ((64, 48), (48, 64))]
    pool = _settled(pool)
    fam["escape"] = rim + _pick(pool, lambda r: r["reset"] and r["exit"] != "left", 12) + _pick(pool, lambda r: r["exit"] == "left" and r["reset"], 8) + \
        _pick(pool, lambda r: r["exit"] == "left" and not r["reset"], 8)
    mx = []
    for i in range(12):
        key = ("x", 64, 48, (7 * i) % 91, 20 + i)
        cx, cy = center(key)
        bx, by = int(round(cx)), int(round(cy))
        mx += [case("maxiter", "subpix", key, (bx + dx, by + dy), win=1) for dx, dy in ((0, 0), (1, 0), (0, 1), (-1, 1), (1, -1))]
    fam["maxiter"] = mx
    q = []
    tall, wide = ("checker", 48, 64, 10, 11), ("checker", 64, 48, 10, 11)
    q += [case("quirk", "harris", tall, p) for p in ((20, 48), (20.5, 48), (30, 47.875), (20, 48.125), (20, 49), (10, 55.5), (24, 63), (24, 64), (5, 65), (20, 80),
                                                      (-1, 10), (-0.125, 10), (10, -1), (10, -0.5), (0, 0), (47, 48), (60, 20), (47.5, 30))]
    q += [case("quirk", "harris", wide, p) for p in ((20, 48), (20, 48.5), (20, 47), (63, 47), (70, 20), (-0.5, 47), (30, 49))]
    fam["quirk"] = q
    # ---- locked corners
    ck64, ck160 = ("checker", 64, 48, 10, 11), ("checker", 160, 120, 20, 17)
    inter, clipped, thin = [], [], []
    for ws in WSIZES:
        key, W, H = (ck160, 160, 120) if ws == 31 else (ck64, 64, 48)
        pts = [(W // 2, H // 2), (W // 2 - 3, H // 2 + 2), (W // 2 + 0.5, H // 2 - 0.25), (ws, ws), (W - ws, H - ws), (W // 2 + 5.75, H // 2 - 1)]
        full = [case("interior", "locked", key, p, wsize=ws) for p in pts]
        edge = [case("clipped", "locked", key, p, wsize=ws) for p in
                ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (1, 1), (W - 2, H - 2), (2, H // 2), (W - 3, H // 2), (W // 2, 1), (W // 2, H - 2), (0, H // 2),
                 (W // 2, 0), (ws - 1, ws + 2) if ws > 1 else (0, 3), (W - ws + 1, 3), (5, min(H - 1, H - ws + 2)))]
        def side(c):
            x0, y0, x1, y1 = locked_window(c["pt"], ws, W, H)
            return min(x1 - x0, y1 - y0)

        inter += [c for c in full if side(c) == 2 * ws]
        clipped += edge
        thin += [dict(c, family="thin") for c in full + edge if side(c) < 9]
    fam["locked_interior"], fam["clipped"], fam["thin"] = inter, clipped, thin
    fam["stride"] += [dict(c, family="stride", stride=c["image"][1] + pad, name=c["name"].replace("interior", "stride").replace("/None/", "/+%d/" % pad))
                      for c in inter for pad in (3, 13)]
    nop = []
    for key in (("const", 64, 48), ("xramp", 64, 48), ("yramp", 64, 48)):
        for ws in (1, 4, 7, 15, 31):
            nop += [case("nopeak", "locked", key, p, wsize=ws) for p in ((0, 0), (0.5, 0.75), (32, 24), (63, 47), (40, 3), (2, 30))]
    fam["nopeak"] = nop
    tw = []
    for ax, ay in ((5, 16), (6, 17), (7, 16), (8, 19), (5, 19), (8, 16), (7, 18), (6, 19)):
        for fx, fy in ((0, 0), (1, 0), (0, 1), (1, 1)):
            tw.append(case("twin", "locked", ("twin", 80, 60, ax, ay, 11, fx, fy), (80, 60), wsize=31))
    fam["twin"] = tw
    ch = []
    for m2, win in (("subpix", 7), ("subpix", 3), ("harris", 0)):
        for ws in (7, 15) if m2 == "subpix" else (7, 31):
            key, W, H = (ck160, 160, 120) if ws == 31 else (ck64, 64, 48)
            ch += [case("chain", "locked+" + m2, key, p, win=win, wsize=ws) for p in ((W // 2, H // 2), (W // 2 - 7, H // 2 + 4), (ws + 3, ws + 1), (2, 3), (W - 2, H - 4),
                                                                                      (W // 2 + 0.5, 1), (W - ws, H // 2))]
        for key in (("const", 64, 48), ("xramp", 64, 48)):
            ch += [case("chain", "locked+" + m2, key, p, win=win, wsize=7) for p in ((0, 0), (3, 2), (30, 20))]
    fam["chain"] = ch
    _families = fam
    return fam


SUBPIX_FAMILIES = ("interior", "border", "stride", "degenerate", "escape", "maxiter", "quirk")
LOCKED_FAMILIES = ("locked_interior", "clipped", "thin", "nopeak", "twin", "chain")
FAMILIES = SUBPIX_FAMILIES + LOCKED_FAMILIES


def many_points(n):
    """`n` corners for one call: the interior SUBPIX starts of one frame and window, repeated."""
    cs = [c for c in families()["interior"] if c["method"] == "subpix" and c["win"] == 7 and c["image"] == ("x", 64, 48, 45, 2)]
    return [cs[i % len(cs)] for i in range(n)]


def groups(cases):
    """Cases that one call can carry: same frame, stride, method and windows. {(image, stride, method, win, wsize): [cases]}."""
    g = {}
    for c in cases:
        g.setdefault((c["image"], c["stride"], c["method"], c["win"], c["wsize"]), []).append(c)
    return g


def method_codes(method):
    """(method of the refinement, whether the pre-pass runs) for the entry point."""
    m2 = method.split("+")[-1]
    return {"subpix": SUBPIX, "harris": HARRIS, "locked": NONE}[m2], method.startswith("locked")


def bound_key(method):
    return method.split("+")[-1]


def judge(c, got):
    """How one result compares with the reference: (ok, deviation from `exact` in px, the bound). Exact where the reference says exact (integers
    of the pre-pass, returned starts); a fragile case may take its neighbouring result instead; a fragile_det case is not judged."""
    return judge_against(reference(c), c["method"], got, c["method"] == "locked" or returns_start(c))


def judge_against(r, method, got, exactly=False):
    got = np.asarray(got, np.float64)
    if "fragile_det" in r["fragile"]:
        return True, 0.0, 0.0
    wants = [r["exact"]] + list(r["accept"])
    if exactly:
        return any(np.array_equal(got, w) for w in wants), float(np.max(np.abs(got - r["exact"]))), 0.0
    best = None
    for w in wants:
        d, b = float(np.max(np.abs(got - w))), fine_bound(bound_key(method), w)
        if best is None or d / b < best[1] / best[2]:
            best = (bool(np.all(np.isfinite(got))) and d <= b, d, b)
    return best


def run(cases, call, limit=1 << 20):
    """The results of `cases`, in their order, from call(frame [H][stride], width, points n x 2, method, win, locked_wsize) -> n x 2: one call for
    every group of cases that share frame, stride, method and windows (`limit` points a call at most)."""
    out = {}
    for (key, stride, method, win, wsize), cs in groups(cases).items():
        img = image(key)
        frame = img if stride is None else padded(img, stride)
        code, pre = method_codes(method)
        pts = np.array([c["pt"] for c in cs], np.float32)
        got = np.concatenate([np.asarray(call(frame, img.shape[1], pts[i:i + limit], code, win, wsize if pre else 0), np.float32).reshape(-1, 2)
                              for i in range(0, len(pts), limit)])
        for c, g in zip(cs, np.asarray(got, np.float32).reshape(-1, 2)):
            out[c["name"]] = g.copy()
    return [out[c["name"]] for c in cases]
