"""Frames out: a plain numpy restatement of the definitions in include/arucohip.h ("Frames out"), written from the header's text and
sharing no code with k_egress.hip. The packing, the strided layout and the frame extents are those of the input side (tests/ingest_ref.py).

An image is uint8 [H][W] (grey) or [H][W][3] (B,G,R). export() returns the destination's planes; pack() lays them out as the tightly packed
raw frame [rows][row bytes] that ingest_ref.lay_out, ingest_ref.to_bgr and ingest_ref.to_gray take."""
import numpy as np

from tests.ingest_ref import BYTES_PER_PIXEL, frame_bytes, gray_of, lay_out, pack_nv12, pack_yuv422, rows_of  # noqa: F401  (re-exported)

DESTINATIONS = ("GRAY8", "BGR8", "RGB8", "BGRA8", "RGBA8", "YUYV", "UYVY", "NV12")
REFUSED = ("GRAY16", "BAYER_RGGB", "BAYER_BGGR", "BAYER_GRBG", "BAYER_GBRG")
YUV = ("YUYV", "UYVY", "NV12")
GREY_IS_LUMA = 1

# round(c * 2^20 / 255) of the BT.601 video-range matrix, rows Y, U, V, columns R, G, B
LUMA = (269262, 528618, 102662)
CHROMA_U = (-155424, -305127, 460551)
CHROMA_V = (460551, -385654, -74897)
MATRIX = ((65.481, 128.553, 24.966), (-37.797, -74.203, 112.0), (112.0, -93.786, -18.214))


def _i64(*v):
    return tuple(np.asarray(a).astype(np.int64) for a in v)


def luma(r, g, b):
    r, g, b = _i64(r, g, b)
    return (LUMA[0] * r + LUMA[1] * g + LUMA[2] * b + (16 << 20) + (1 << 19)) >> 20


def chroma_sums(sr, sg, sb, k):
    """The two sums before the shift, for channel sums over 2^k pixels."""
    sr, sg, sb = _i64(sr, sg, sb)
    bias = (128 << (20 + k)) + (1 << (19 + k))
    return (CHROMA_U[0] * sr + CHROMA_U[1] * sg + CHROMA_U[2] * sb + bias, CHROMA_V[0] * sr + CHROMA_V[1] * sg + CHROMA_V[2] * sb + bias)


def chroma(sr, sg, sb, k):
    u, v = chroma_sums(sr, sg, sb, k)
    return u >> (20 + k), v >> (20 + k)


def yuv_float(r, g, b):
    """The float64 matrix the fixed-point one approximates (unrounded)."""
    r, g, b = (np.asarray(a).astype(np.float64) for a in (r, g, b))
    return tuple(o + (m[0] * r + m[1] * g + m[2] * b) / 255.0 for m, o in zip(MATRIX, (16.0, 128.0, 128.0)))


def _channels(img):
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        return img, img, img, True
    assert img.ndim == 3 and img.shape[2] == 3
    return img[..., 0], img[..., 1], img[..., 2], False


def export(name, img, flags=0):
    """The planes of the destination `name`: (pixels [H][W][bytes per pixel],) for GRAY8 and the packed colour formats, (Y [H][W], U, V) for the
    YUV formats with U and V [H][W / 2] (YUYV / UYVY) or [H / 2][W / 2] (NV12)."""
    b, g, r, grey = _channels(img)
    H, W = b.shape
    if name == "GRAY8":
        return ((b if grey else gray_of(b, g, r))[..., None].astype(np.uint8),)
    if name in ("BGR8", "RGB8", "BGRA8", "RGBA8"):
        ch = [b, g, r] if name.startswith("BGR") else [r, g, b]
        if name.endswith("A8"):
            ch.append(np.full((H, W), 255, np.uint8))
        return (np.stack(ch, axis=-1).astype(np.uint8),)
    assert name in YUV and W % 2 == 0 and (name != "NV12" or H % 2 == 0)
    Y = b.astype(np.int64) if grey and flags & GREY_IS_LUMA else luma(r, g, b)
    bi, gi, ri = _i64(b, g, r)
    if name == "NV12":
        box = lambda c: c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]  # noqa: E731
        U, V = chroma(box(ri), box(gi), box(bi), 2)
    else:
        box = lambda c: c[:, 0::2] + c[:, 1::2]  # noqa: E731
        U, V = chroma(box(ri), box(gi), box(bi), 1)
    if grey:
        U, V = np.full_like(U, 128), np.full_like(V, 128)
    assert min(Y.min(), U.min(), V.min()) >= 0 and max(Y.max(), U.max(), V.max()) <= 255
    return Y.astype(np.uint8), U.astype(np.uint8), V.astype(np.uint8)


def pack(name, planes):
    """The planes of export() as a tightly packed raw frame [rows][row bytes]."""
    if name == "NV12":
        return pack_nv12(*planes)
    if name in ("YUYV", "UYVY"):
        return pack_yuv422(*planes, name)
    px = planes[0]
    return np.ascontiguousarray(px).reshape(px.shape[0], px.shape[1] * px.shape[2])


def export_raw(name, img, flags=0):
    return pack(name, export(name, img, flags))
