"""Camera-native input without a GPU: the numpy restatement of the definitions (tests/ingest_ref.py) is checked against the properties the
definitions imply, and the host-only part of the C ABI (declared symbols, the stride arithmetic) against the built library."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import ingest_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INGEST_SYMBOLS = ["arucohip_frame_min_row_stride", "arucohip_frame_min_stride", "arucohip_convert_batch"]


@pytest.mark.parametrize("pattern", ir.BAYER)
@pytest.mark.parametrize("size", [(2, 2), (3, 2), (5, 7)])
def test_constant_colour_demosaics_to_itself_everywhere(pattern, size):
    W, H = size
    for colour in ((10, 200, 90), (255, 0, 128), (0, 0, 0), (255, 255, 255)):
        img = np.empty((H, W, 3), np.uint8)
        img[:] = colour
        out = ir.demosaic(ir.mosaic(img, pattern), pattern)
        assert (out == img).all(), (pattern, size, colour)


@pytest.mark.parametrize("pattern", ir.BAYER)
def test_demosaic_returns_the_sample_in_the_sites_own_channel(pattern):
    rng = np.random.default_rng(5)
    m = rng.integers(0, 256, (7, 9)).astype(np.uint8)
    out = ir.demosaic(m, pattern)
    letters = ir.site_letters(pattern, 7, 9)
    for ch, k in (("B", 0), ("G", 1), ("R", 2)):
        assert (out[..., k][letters == ch] == m[letters == ch]).all()
    assert "".join(letters[:2, :2].ravel()) == pattern


def test_the_four_patterns_agree_on_a_shifted_image():
    """A mosaic shifted by one column (row) is a mosaic of the pattern with its columns (rows) swapped: away from the reflected border the
    demosaic of the shifted image is the shifted demosaic."""
    rng = np.random.default_rng(6)
    m = rng.integers(0, 256, (12, 14)).astype(np.uint8)
    col = {"RGGB": "GRBG", "GRBG": "RGGB", "BGGR": "GBRG", "GBRG": "BGGR"}   # pattern of m[:, 1:]
    row = {"RGGB": "GBRG", "GBRG": "RGGB", "BGGR": "GRBG", "GRBG": "BGGR"}   # pattern of m[1:, :]
    for p in ir.BAYER:
        full = ir.demosaic(m, p)
        assert (ir.demosaic(m[:, 1:], col[p])[1:-1, 1:-1] == full[1:-1, 2:-1]).all(), p
        assert (ir.demosaic(m[1:, :], row[p])[1:-1, 1:-1] == full[2:-1, 1:-1]).all(), p


def test_yuv_to_bgr_is_within_one_of_the_float_formula_over_all_triples():
    u, v = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    u, v = u.ravel(), v.ravel()
    for y0 in range(0, 256, 16):   # 16 chunks of 2^20 triples
        Y = np.repeat(np.arange(y0, y0 + 16), 65536)
        U, V = np.tile(u, 16), np.tile(v, 16)
        fixed = ir.yuv_to_bgr(Y, U, V)
        exact = ir.yuv_to_bgr_float(Y, U, V)
        for f, e in zip(fixed, exact):
            assert np.abs(f.astype(np.float64) - np.clip(e, 0.0, 255.0)).max() <= 1.0
    Y = np.arange(256)
    B, G, R = ir.yuv_to_bgr(Y, np.full(256, 128), np.full(256, 128))
    assert (B == G).all() and (G == R).all()
    assert B[16] == 0 and B[0] == 0 and B[235] == 255 and B[255] == 255


def test_gray16_saturates_and_eight_bits_is_the_identity():
    g = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert (ir.to_gray("GRAY16", ir.widen(g, 8), 16, 16, 8) == g).all()
    for bits in range(8, 17):
        assert (ir.to_gray("GRAY16", ir.widen(g, bits), 16, 16, bits) == g).all()
        if bits < 16:   # values above 2^bits - 1 saturate
            over = np.array([[1 << bits, (1 << bits) + 5, 0xFFFF, (1 << bits) - 1]], "<u2").view(np.uint8)
            assert ir.to_gray("GRAY16", over, 4, 1, bits).tolist() == [[255, 255, 255, 255]]
    raw = np.array([[0x34, 0x12]], np.uint8)   # little-endian 0x1234
    assert ir.to_gray("GRAY16", raw, 1, 1, 16)[0, 0] == 0x12 and ir.to_gray("GRAY16", raw, 1, 1, 13)[0, 0] == min(0x1234 >> 5, 255)


def test_encoders_and_decoders_are_inverse_where_they_can_be():
    rng = np.random.default_rng(8)
    g = rng.integers(0, 256, (6, 8)).astype(np.uint8)
    for name in ir.FORMATS:
        raw = ir.encode(name, g, rng, bits=12)
        assert raw.shape == (ir.rows_of(name, 6), 8 * ir.BYTES_PER_PIXEL[name]), name
        if not name.startswith("BAYER_"):   # a grey mosaic is smoothed by the demosaic; everything else carries the grey image exactly
            assert (ir.to_gray(name, raw, 8, 6, 12) == g).all(), name
    bgr = rng.integers(0, 256, (6, 8, 3)).astype(np.uint8)
    assert (ir.to_bgr("RGB8", bgr[..., ::-1].reshape(6, 24), 8, 6) == bgr).all()
    assert (ir.to_gray("BGR8", bgr.reshape(6, 24), 8, 6) == ir.gray_of(bgr[..., 0], bgr[..., 1], bgr[..., 2])).all()


def test_header_declares_and_library_exports_the_ingest_calls():
    from aruco_amd import build_library, capi
    txt = open(os.path.join(ROOT, "include", "arucohip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(arucohip_[a-z_0-9]+)\s*\(", txt))
    assert not [s for s in INGEST_SYMBOLS if s not in declared]
    for name in ("arucohip_pixel_format", "arucohip_frame_format_t", "ARUCOHIP_PIX_NV12", "ARUCOHIP_PIX_BAYER_GBRG"):
        assert name in txt
    lib = build_library()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    assert not [s for s in INGEST_SYMBOLS if s not in exported]
    assert not [s for s in INGEST_SYMBOLS if s not in capi.SYMBOLS]
    assert capi.PIX_NAMES == ir.FORMATS and capi.PIX_BAYER_GBRG == 12


def test_min_strides_through_the_built_library():
    from aruco_amd import build_library, capi
    build_library()
    for name in ir.FORMATS:
        fmt = capi.frame_format(name, bits=12 if name == "GRAY16" else 0)
        for W, H in ((2, 2), (6, 4), (640, 480)):
            rb = W * ir.BYTES_PER_PIXEL[name]
            assert fmt.min_row_stride(W) == rb, name
            for rs in (rb, rb + 3):
                assert fmt.min_stride(W, H, rs) == ir.frame_bytes(name, W, H, rs), name
            assert fmt.min_stride(W, H, rb - 1) == 0
        assert fmt.min_row_stride(0) == 0 and fmt.min_stride(4, 0, 64) == 0
    # the constraints of the table
    for name in ("YUYV", "UYVY", "NV12"):
        assert capi.frame_format(name).min_row_stride(5) == 0
    assert capi.nv12().min_stride(4, 3, 4) == 0 and capi.nv12().min_stride(4, 4, 4) == 4 * 4 + 4 * 1 + 4
    assert capi.nv12(chroma_offset=8 * 4 + 16).min_stride(4, 4, 8) == ir.frame_bytes("NV12", 4, 4, 8, chroma_gap=16)
    assert capi.nv12(chroma_offset=8 * 4 - 1).min_stride(4, 4, 8) == 0
    for p in ir.BAYER:
        assert capi.bayer(p).min_row_stride(1) == 0 and capi.bayer(p).min_stride(2, 1, 2) == 0 and capi.bayer(p).min_stride(3, 3, 3) == 9
    for bits in (7, 17, 0):
        assert capi.gray16(bits).min_row_stride(4) == 0
    assert capi.gray16(8).min_row_stride(4) == 8 and capi.gray16(16).min_row_stride(4) == 8
    assert capi.FrameFormat(13, 0, 0).min_row_stride(4) == 0 and capi.FrameFormat(-1, 0, 0).min_row_stride(4) == 0
