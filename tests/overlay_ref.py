"""numpy restatement of the overlay rules (DESIGN.md "Overlay"): the primitive list of a marker / a board in painting order, the
projection as tests/planar_ref.py does it, and a painter that stamps one primitive after another (a scatter, where the device
gathers). Written from the rules, not from the kernel; the only thing shared with the library is the font table, which is data.
Shared by test_overlay_cpu.py, test_gpu_overlay.py and test_gpu_overlay_shim.py."""
import os
import re

import numpy as np

from tests import planar_ref

OUTLINE, IDS, AXIS, CUBE, Y_PERP = 1, 2, 4, 8, 16
LIMIT = float(2 ** 20)
RED, GREEN, BLUE = (0, 0, 255), (0, 255, 0), (255, 0, 0)   # B G R

_FONT_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "aruco_amd", "csrc", "overlay_font.h")


def load_font():
    """{character: 7 row bytes} from the library's font header."""
    text = open(_FONT_H).read()
    chars = re.search(r'OVERLAY_FONT_CHARS "([^"]+)"', text).group(1)
    rows = re.findall(r"\{((?:\s*0x[0-9A-Fa-f]{2},?){7})\}", text)
    assert len(rows) == len(chars)
    return {c: [int(v, 16) for v in re.findall(r"0x[0-9A-Fa-f]{2}", r)] for c, r in zip(chars, rows)}


FONT = load_font()


def _valid(x, y):
    return bool(np.isfinite(x) and np.isfinite(y) and abs(x) <= LIMIT and abs(y) <= LIMIT)


def to_pixel(x, y):
    """Point2f -> cv::Point: narrowed to float32, rounded ties-to-even; None for a point that drops its primitive."""
    with np.errstate(all="ignore"):
        x, y = np.float32(x), np.float32(y)
    if not _valid(x, y):
        return None
    return int(np.rint(x)), int(np.rint(y))


def project(points, rvec, tvec, K, dist):
    """float32 object points -> float64 image points (inf / nan where the depth is 0)."""
    P = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    Km = np.asarray(K, np.float32).astype(np.float64).reshape(3, 3)
    d = None if dist is None else np.asarray(dist, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return planar_ref.brown_project(P, planar_ref.rodrigues(rvec), np.asarray(tvec, np.float64), Km, d)


def marker_axis_points(ssize):
    s = np.float32(ssize) * np.float32(3)
    return np.array([[0, 0, 0], [s, 0, 0], [0, s, 0], [0, 0, s]], np.float32)


def marker_cube_points(ssize, y_perp):
    s = np.float32(ssize)
    h = np.float32(s / np.float32(2))
    base = [(-h, -h), (h, -h), (h, h), (-h, h)]
    pts = [(a, b, up) for up in (np.float32(0), s) for a, b in base]
    if y_perp:
        pts = [(a, up, b) for a, b, up in pts]
    return np.array(pts, np.float32)


def board_axis_points(size):
    s = np.float32(2) * np.float32(size)
    return np.array([[0, 0, 0], [s, 0, 0], [0, s, 0], [0, 0, s]], np.float32)


def board_cube_points(size, y_perp):
    c = np.float32(size)
    t0 = np.float32(-c / np.float32(2))
    t1 = np.float32(t0 + c)
    z = np.float32(0)
    if y_perp:
        pts = [(t0, z, t0), (t1, z, t0), (t1, c, t0), (t0, c, t0), (t0, z, t1), (t1, z, t1), (t1, c, t1), (t0, c, t1)]
    else:
        pts = [(t0, t0, z), (t1, t0, z), (t1, t0, -c), (t0, t0, -c), (t0, t1, z), (t1, t1, z), (t1, t1, -c), (t0, t1, -c)]
    return np.array(pts, np.float32)


CUBE_EDGES = [(i, (i + 1) % 4) for i in range(4)] + [(4 + i, 4 + (i + 1) % 4) for i in range(4)] + [(i, i + 4) for i in range(4)]


def centroid(corners):
    """marker.cpp:71-77: Point cent(0, 0); cent.x += corner.x (int = int + float, truncated); cent.x /= 4. (double, truncated)."""
    c = np.asarray(corners, np.float32).reshape(4, 2)
    out = []
    for k in range(2):
        acc = 0
        for i in range(4):
            acc = int(np.float32(acc) + c[i, k])      # int() truncates toward zero
        out.append(int(acc / 4.0))
    return tuple(out)


class Prims:
    """A primitive list. ("line", p0, p1, colour, width) and ("text", anchor, string, colour, scale). `coords` collects every projected
    coordinate that was kept (float32), for the tests' distance-from-a-half-integer condition."""

    def __init__(self):
        self.items = []
        self.coords = []

    def line(self, a, b, color, w):
        if a is not None and b is not None:
            self.items.append(("line", a, b, tuple(color), int(w)))

    def rect(self, a, b, color, w):
        if a is None or b is None:
            return
        for p, q in (((a[0], a[1]), (b[0], a[1])), ((b[0], a[1]), (b[0], b[1])), ((b[0], b[1]), (a[0], b[1])), ((a[0], b[1]), (a[0], a[1]))):
            self.line(p, q, color, w)

    def text(self, anchor, string, color, scale):
        if anchor is not None:
            self.items.append(("text", anchor, string, tuple(color), int(scale)))

    def projected(self, pts, rvec, tvec, K, dist):
        img = project(pts, rvec, tvec, K, dist)
        out = []
        for x, y in img:
            p = to_pixel(x, y)
            out.append(p)
            if p is not None:
                self.coords += [float(np.float32(x)), float(np.float32(y))]
        return out

    def axis(self, pts, rvec, tvec, K, dist, width, labels, scale):
        p = self.projected(pts, rvec, tvec, K, dist)
        for i, col in enumerate((RED, GREEN, BLUE)):
            self.line(p[0], p[1 + i], col, width)
        for i, col in enumerate((RED, GREEN, BLUE)):
            self.text(p[1 + i], labels[i], col, scale)

    def cube(self, pts, rvec, tvec, K, dist):
        p = self.projected(pts, rvec, tvec, K, dist)
        for a, b in CUBE_EDGES:
            self.line(p[a], p[b], RED, 1)


def marker_prims(pr, m, K, dist, flags, line_width, color):
    """Appends the primitives of marker m (an element of capi.MARKER_DTYPE, or a dict with the same fields)."""
    c = np.asarray(m["corners"], np.float32).reshape(4, 2)
    px = [to_pixel(c[i, 0], c[i, 1]) for i in range(4)]
    if flags & OUTLINE:
        for i in range(4):
            pr.line(px[i], px[(i + 1) % 4], color, line_width)
        two = np.float32(2)
        for i, col in enumerate((RED, GREEN, BLUE)):
            pr.rect(to_pixel(c[i, 0] - two, c[i, 1] - two), to_pixel(c[i, 0] + two, c[i, 1] + two), col, line_width)
    if flags & IDS and all(p is not None for p in px):
        pr.text(centroid(c), "id=%d" % int(m["id"]), tuple(255 - int(v) for v in color[:3]), 2)
    if not int(m["has_pose"]):
        return
    if flags & AXIS:
        pr.axis(marker_axis_points(m["ssize"]), m["rvec"], m["tvec"], K, dist, 1, "xyz", 2)
    if flags & CUBE:
        pr.cube(marker_cube_points(m["ssize"], bool(flags & Y_PERP)), m["rvec"], m["tvec"], K, dist)


def board_prims(pr, b, marker_size, K, dist, flags):
    if not int(b["has_pose"]):
        return
    if flags & AXIS:
        pr.axis(board_axis_points(marker_size), b["rvec"], b["tvec"], K, dist, 2, "XYZ", 3)
    if flags & CUBE:
        pr.cube(board_cube_points(marker_size, bool(flags & Y_PERP)), b["rvec"], b["tvec"], K, dist)


def line_pixels(a, b):
    """The n + 1 pixels of a line: the major coordinate advances by one, minor = minor0 + sign * floor((2 i |dminor| + n) / (2n))."""
    (x0, y0), (x1, y1) = a, b
    dx, dy = x1 - x0, y1 - y0
    n = max(abs(dx), abs(dy))
    if n == 0:
        return [(x0, y0)]
    sgn = lambda v: -1 if v < 0 else 1
    out = []
    for i in range(n + 1):
        if abs(dx) >= abs(dy):
            out.append((x0 + sgn(dx) * i, y0 + sgn(dy) * ((2 * i * abs(dy) + n) // (2 * n))))
        else:
            out.append((x0 + sgn(dx) * ((2 * i * abs(dx) + n) // (2 * n)), y0 + sgn(dy) * i))
    return out


def _clip_line_pixels(a, b, W, H, w):
    """line_pixels restricted to those whose stamp can reach the image (lines may run to +-2^20)."""
    (x0, y0), (x1, y1) = a, b
    dx, dy = x1 - x0, y1 - y0
    n = max(abs(dx), abs(dy))
    if n <= 4096:
        return line_pixels(a, b)
    # a long line: only the steps whose major coordinate is within the image (plus the stamp)
    xmajor = abs(dx) >= abs(dy)
    M0, dM, size = (x0, dx, W) if xmajor else (y0, dy, H)
    lo, hi = -w, size + w
    i0, i1 = (lo - M0, hi - M0) if dM > 0 else (M0 - hi, M0 - lo)
    i0, i1 = max(i0, 0), min(i1, n)
    sgn = lambda v: -1 if v < 0 else 1
    out = []
    for i in range(i0, i1 + 1):
        if xmajor:
            out.append((x0 + sgn(dx) * i, y0 + sgn(dy) * ((2 * i * abs(dy) + n) // (2 * n))))
        else:
            out.append((x0 + sgn(dx) * ((2 * i * abs(dx) + n) // (2 * n)), y0 + sgn(dy) * i))
    return out


def paint(img, prims):
    """img: [H][W][C] uint8 view, painted in place, one primitive after another."""
    H, W, C = img.shape
    for it in prims.items if isinstance(prims, Prims) else prims:
        col = np.array(it[3][:C], np.uint8)
        if it[0] == "line":
            w = it[4]
            o = (w - 1) // 2
            for x, y in _clip_line_pixels(it[1], it[2], W, H, w):
                xa, ya, xb, yb = max(x - o, 0), max(y - o, 0), min(x - o + w, W), min(y - o + w, H)
                if xa < xb and ya < yb:
                    img[ya:yb, xa:xb] = col
        else:
            (ax, ay), s = it[1], it[4]
            for k, ch in enumerate(it[2]):
                for r, bits in enumerate(FONT[ch]):
                    for c in range(5):
                        if bits >> (4 - c) & 1:
                            xa, ya = ax + 6 * s * k + c * s, ay - 7 * s + 1 + r * s
                            xb, yb = min(xa + s, W), min(ya + s, H)
                            xa, ya = max(xa, 0), max(ya, 0)
                            if xa < xb and ya < yb:
                                img[ya:yb, xa:xb] = col


def frame_view(buf, f, width, channels):
    """Frame f of a [N][H][row_stride] byte buffer as [H][W][C] (a view)."""
    H = buf.shape[1]
    return buf[f, :, :width * channels].reshape(H, width, channels)


def draw_markers(buf, width, channels, markers, counts, K=None, dist=None, flags=OUTLINE | IDS, line_width=1, color=RED):
    """The restatement of arucohip_draw_markers_batch on a [N][H][row_stride] buffer, in place. Returns the kept projected coordinates."""
    coords = []
    cap = markers.shape[1]
    for f in range(buf.shape[0]):
        pr = Prims()
        for i in range(min(max(int(counts[f]), 0), cap)):
            marker_prims(pr, markers[f, i], K, dist, flags, line_width, color)
        paint(frame_view(buf, f, width, channels), pr)
        coords += pr.coords
    return coords


def draw_boards(buf, width, channels, boards, marker_size, K, dist=None, flags=AXIS | CUBE):
    coords = []
    for f in range(buf.shape[0]):
        pr = Prims()
        board_prims(pr, boards[f], marker_size, K, dist, flags)
        paint(frame_view(buf, f, width, channels), pr)
        coords += pr.coords
    return coords


def half_integer_margin(coords):
    """The smallest distance of any coordinate from a half-integer (1.0 for none)."""
    if not coords:
        return 1.0
    c = np.asarray(coords, np.float64)
    return float(np.min(np.abs((c - 0.5) - np.rint(c - 0.5))))
