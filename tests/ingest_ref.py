"""Camera-native input: a plain numpy restatement of the definitions in include/arucohip.h ("Camera-native input"), written from the
definitions and sharing no code with k_ingest.hip, plus the encoders that make test inputs (mosaic a BGR image, pack Y / U / V, widen grey).

A frame is a tightly packed uint8 array [rows][row bytes] as the producer stores it: GRAY16 little-endian, YUYV / UYVY 2 bytes per pixel,
NV12 with its U,V plane (H / 2 rows) behind the Y plane."""
import numpy as np

FORMATS = ("GRAY8", "BGR8", "RGB8", "BGRA8", "RGBA8", "GRAY16", "YUYV", "UYVY", "NV12", "BAYER_RGGB", "BAYER_BGGR", "BAYER_GRBG", "BAYER_GBRG")
BAYER = ("RGGB", "BGGR", "GRBG", "GBRG")
BYTES_PER_PIXEL = {"GRAY8": 1, "BGR8": 3, "RGB8": 3, "BGRA8": 4, "RGBA8": 4, "GRAY16": 2, "YUYV": 2, "UYVY": 2, "NV12": 1,
                   "BAYER_RGGB": 1, "BAYER_BGGR": 1, "BAYER_GRBG": 1, "BAYER_GBRG": 1}


def gray_of(b, g, r):
    b, g, r = (np.asarray(v).astype(np.int64) for v in (b, g, r))
    return ((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14).astype(np.uint8)


def sat(v):
    return np.clip(v, 0, 255).astype(np.uint8)


def yuv_to_bgr(Y, U, V):
    """BT.601 video range, 20-bit fixed point. Arrays of equal shape -> (B, G, R) uint8. numpy's >> of a negative int64 is the floor shift."""
    Y, U, V = (np.asarray(v).astype(np.int64) for v in (Y, U, V))
    y = np.maximum(0, Y - 16) * 1220542
    R = sat((y + 1673527 * (V - 128) + 524288) >> 20)
    G = sat((y - 852492 * (V - 128) - 409993 * (U - 128) + 524288) >> 20)
    B = sat((y + 2116026 * (U - 128) + 524288) >> 20)
    return B, G, R


def yuv_to_bgr_float(Y, U, V):
    """The float64 formula the fixed-point one approximates (unrounded, unclamped)."""
    Y, U, V = (np.asarray(v).astype(np.float64) for v in (Y, U, V))
    y = 1.164 * np.maximum(0.0, Y - 16)
    return y + 2.018 * (U - 128), y - 0.813 * (V - 128) - 0.391 * (U - 128), y + 1.596 * (V - 128)


def site_letters(pattern, H, W):
    """[H][W] array of 'R' / 'G' / 'B': the pattern names the top-left 2 x 2 block row by row."""
    yy, xx = np.mgrid[:H, :W]
    return np.array(list(pattern))[(yy & 1) * 2 + (xx & 1)]


def demosaic(m, pattern):
    """Bilinear demosaic of a mosaic [H][W] (H, W >= 2) -> [H][W][3] in B,G,R order; neighbours outside by reflect-101."""
    m = np.asarray(m)
    H, W = m.shape
    p = np.pad(m.astype(np.int64), 1, mode="reflect")   # numpy's 'reflect' is reflect-101
    c, N, S, Wn, E = p[1:-1, 1:-1], p[:-2, 1:-1], p[2:, 1:-1], p[1:-1, :-2], p[1:-1, 2:]
    NW, NE, SW, SE = p[:-2, :-2], p[:-2, 2:], p[2:, :-2], p[2:, 2:]
    cross, diag = (N + S + E + Wn + 2) >> 2, (NW + NE + SW + SE + 2) >> 2
    hor, ver = (Wn + E + 1) >> 1, (N + S + 1) >> 1
    yy, xx = np.mgrid[:H, :W]
    letters = site_letters(pattern, H, W)
    row_other = np.array(list(pattern))[(yy & 1) * 2 + (1 - (xx & 1))]   # the colour of the row's other sites
    out = {"G": np.where(letters == "G", c, cross)}
    for ch in "RB":
        out[ch] = np.where(letters == ch, c, np.where(letters == "G", np.where(row_other == ch, hor, ver), diag))
    return np.stack([out["B"], out["G"], out["R"]], axis=-1).astype(np.uint8)


# ---- decoding a raw frame

def _split_yuv422(raw, W, name):
    q = raw[:, :2 * W].reshape(raw.shape[0], W // 2, 4)
    if name == "YUYV":
        y0, u, y1, v = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    else:
        u, y0, v, y1 = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    Y = np.stack([y0, y1], axis=-1).reshape(raw.shape[0], W)
    return Y, np.repeat(u, 2, axis=1), np.repeat(v, 2, axis=1)


def to_bgr(name, raw, W, H, bits=0):
    """A tightly packed raw frame -> [H][W][3] uint8 in B,G,R order."""
    raw = np.asarray(raw, np.uint8)
    if name in ("GRAY8", "GRAY16", ):
        g = to_gray(name, raw, W, H, bits)
        return np.stack([g, g, g], axis=-1)
    if name in ("BGR8", "RGB8", "BGRA8", "RGBA8"):
        px = raw[:H].reshape(H, W, BYTES_PER_PIXEL[name])[..., :3]
        return np.ascontiguousarray(px if name.startswith("BGR") else px[..., ::-1])
    if name in ("YUYV", "UYVY"):
        B, G, R = yuv_to_bgr(*_split_yuv422(raw[:H], W, name))
        return np.stack([B, G, R], axis=-1)
    if name == "NV12":
        Y, uv = raw[:H, :W], raw[H:H + H // 2, :W].reshape(H // 2, W // 2, 2)
        U = np.repeat(np.repeat(uv[..., 0], 2, axis=0), 2, axis=1)
        V = np.repeat(np.repeat(uv[..., 1], 2, axis=0), 2, axis=1)
        B, G, R = yuv_to_bgr(Y, U, V)
        return np.stack([B, G, R], axis=-1)
    assert name.startswith("BAYER_")
    return demosaic(raw[:H, :W], name[6:])


def to_gray(name, raw, W, H, bits=0):
    """A tightly packed raw frame -> [H][W] uint8 grey."""
    raw = np.asarray(raw, np.uint8)
    if name == "GRAY8":
        return raw[:H, :W].copy()
    if name == "GRAY16":
        v = raw[:H, 0:2 * W:2].astype(np.int64) | (raw[:H, 1:2 * W:2].astype(np.int64) << 8)
        return np.minimum(v >> (bits - 8), 255).astype(np.uint8)
    if name in ("YUYV", "UYVY"):
        return np.ascontiguousarray(_split_yuv422(raw[:H], W, name)[0])
    if name == "NV12":
        return raw[:H, :W].copy()
    bgr = to_bgr(name, raw, W, H, bits)
    return gray_of(bgr[..., 0], bgr[..., 1], bgr[..., 2])


def convert(name, raw, W, H, channels, bits=0):
    return to_gray(name, raw, W, H, bits) if channels == 1 else to_bgr(name, raw, W, H, bits)


# ---- encoders: test inputs

def mosaic(bgr, pattern):
    """Sample a [H][W][3] B,G,R image on the pattern's sites -> [H][W]."""
    H, W, _ = bgr.shape
    letters = site_letters(pattern, H, W)
    return np.where(letters == "B", bgr[..., 0], np.where(letters == "G", bgr[..., 1], bgr[..., 2])).astype(np.uint8)


def pack_yuv422(Y, U, V, name):
    """Y [H][W], U and V [H][W / 2] -> [H][2 W] bytes."""
    H, W = Y.shape
    q = np.empty((H, W // 2, 4), np.uint8)
    if name == "YUYV":
        q[..., 0], q[..., 1], q[..., 2], q[..., 3] = Y[:, 0::2], U, Y[:, 1::2], V
    else:
        q[..., 0], q[..., 1], q[..., 2], q[..., 3] = U, Y[:, 0::2], V, Y[:, 1::2]
    return q.reshape(H, 2 * W)


def pack_nv12(Y, U, V):
    """Y [H][W], U and V [H / 2][W / 2] -> [H * 3 / 2][W] bytes."""
    H, W = Y.shape
    uv = np.stack([U, V], axis=-1).reshape(H // 2, W).astype(np.uint8)
    return np.concatenate([np.asarray(Y, np.uint8), uv], axis=0)


def widen(gray, bits, low=None):
    """8-bit grey -> little-endian bytes [H][2 W] of `bits`-bit values: the grey value in the top 8 of the `bits`, `low` (or 0) below."""
    v = np.asarray(gray).astype(np.uint16) << (bits - 8)
    if low is not None and bits > 8:
        v = v | (np.asarray(low).astype(np.uint16) & ((1 << (bits - 8)) - 1))
    H, W = v.shape
    return np.ascontiguousarray(v.astype("<u2")).view(np.uint8).reshape(H, 2 * W)


def encode(name, gray, rng, bits=0):
    """A grey image [H][W] as a raw frame of format `name` whose grey conversion stays close to it: colour formats carry it in all three
    channels (with random alpha), YUV formats as Y with random chroma, GRAY16 in the top bits with random low bits."""
    g = np.asarray(gray, np.uint8)
    H, W = g.shape
    if name == "GRAY8":
        return g.copy()
    if name in ("BGR8", "RGB8"):
        return np.repeat(g[..., None], 3, axis=-1).reshape(H, 3 * W)
    if name in ("BGRA8", "RGBA8"):
        px = np.repeat(g[..., None], 4, axis=-1)
        px[..., 3] = rng.integers(0, 256, (H, W))
        return px.reshape(H, 4 * W)
    if name == "GRAY16":
        return widen(g, bits, rng.integers(0, 1 << 16, (H, W)))
    if name in ("YUYV", "UYVY"):
        return pack_yuv422(g, rng.integers(0, 256, (H, W // 2)), rng.integers(0, 256, (H, W // 2)), name)
    if name == "NV12":
        return pack_nv12(g, rng.integers(0, 256, (H // 2, W // 2)), rng.integers(0, 256, (H // 2, W // 2)))
    return mosaic(np.repeat(g[..., None], 3, axis=-1), name[6:])


def rows_of(name, H):
    return H * 3 // 2 if name == "NV12" else H


def random_raw(name, W, H, rng):
    return rng.integers(0, 256, (rows_of(name, H), W * BYTES_PER_PIXEL[name])).astype(np.uint8)


def lay_out(frames, name, H, row_stride, frame_stride, base=0, chroma_gap=0, fill=0xA5):
    """Tightly packed raw frames [n][rows][row bytes] in a flat buffer with strides: frame f starts at base + f * frame_stride, rows are
    row_stride apart, and the U,V plane of NV12 starts chroma_gap bytes behind the Y plane's last row. Returns (buffer, chroma_offset)."""
    n, rows, rb = frames.shape
    co = row_stride * H + chroma_gap
    buf = np.full(base + n * frame_stride + 8, fill, np.uint8)
    for f in range(n):
        for r in range(rows):
            at = base + f * frame_stride + (r * row_stride if r < H else co + (r - H) * row_stride)
            buf[at:at + rb] = frames[f, r]
    return buf, (co if name == "NV12" else 0)


def frame_bytes(name, W, H, row_stride, chroma_gap=0):
    """The bytes of one frame from its first to its last byte read: the table of arucohip_frame_min_stride."""
    rb = W * BYTES_PER_PIXEL[name]
    if name == "NV12":
        return row_stride * H + chroma_gap + row_stride * (H // 2 - 1) + rb
    return row_stride * (H - 1) + rb


def scene():
    """Two different 320 x 240 grey frames (fixed seed) with four and three markers of 54..64 px, one per quadrant, each turned by up to
    0.4 rad. synth.frame_layout places markers of 86 px and more, of which a frame this small holds one or two: the layouts are made here."""
    from aruco_amd import synth
    rng = np.random.RandomState(20)
    frames = []
    for nm in (4, 3):
        lay = []
        for q, mid in zip(rng.permutation(4)[:nm], rng.choice(1024, nm, replace=False)):
            s, th = rng.uniform(54, 64), rng.uniform(-0.4, 0.4)
            ctr = np.array([80.0 + 160 * (q % 2), 60.0 + 120 * (q // 2)]) + rng.uniform(-3, 3, 2)
            R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
            sq = np.array([[-0.5, -0.5], [0.5, -0.5], [0.5, 0.5], [-0.5, 0.5]]) @ R.T
            lay.append({"id": int(mid), "quad": ctr + sq * s, "quad_q": ctr + sq * s * 9.0 / 7.0})   # one quiet cell around the 7 x 7 marker
        frames.append(synth.render_frame(lay, 320, 240, rng, device="cpu").numpy())
    return np.stack(frames)
