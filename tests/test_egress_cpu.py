"""Frames out without a GPU: the numpy restatement of the definitions (tests/egress_ref.py) is checked against the properties the header
states for them, over all 2^24 (R, G, B) triples, and the host-only part of the C ABI (the declared symbol and flag) against the built library."""
import os
import re
import subprocess

import numpy as np

from tests import egress_ref as er
from tests import ingest_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _chunks():
    """All 2^24 triples as 16 chunks of 2^20: (R, G, B) int64 arrays."""
    g, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    g, b = np.tile(g.ravel(), 16), np.tile(b.ravel(), 16)
    for r0 in range(0, 256, 16):
        yield np.repeat(np.arange(r0, r0 + 16), 65536), g, b


def test_constants_are_the_rounded_matrix_and_the_chroma_rows_sum_to_zero():
    for fixed, exact in zip((er.LUMA, er.CHROMA_U, er.CHROMA_V), er.MATRIX):
        assert fixed == tuple(int(np.floor(c * 2 ** 20 / 255 + 0.5)) for c in exact)
    assert sum(er.LUMA) == 900542 and sum(er.CHROMA_U) == 0 and sum(er.CHROMA_V) == 0


def test_fixed_point_matches_the_float_matrix_and_stays_in_range_over_all_triples():
    lo, hi = [], []
    for R, G, B in _chunks():
        Y = er.luma(R, G, B)
        U, V = er.chroma(R, G, B, 0)
        for fixed, exact in zip((Y, U, V), er.yuv_float(R, G, B)):
            assert np.abs(fixed - exact).max() <= 0.5001
        assert Y.min() >= 16 and Y.max() <= 235
        assert min(U.min(), V.min()) >= 16 and max(U.max(), V.max()) <= 240
        # a pair (k = 1) or a 2 x 2 block (k = 2) of identical pixels has the chroma of the single pixel
        for k in (1, 2):
            Uk, Vk = er.chroma(R << k, G << k, B << k, k)
            assert (Uk == U).all() and (Vk == V).all()
        sums = er.chroma_sums(4 * R, 4 * G, 4 * B, 2)
        lo.append(min(s.min() for s in sums)), hi.append(max(s.max() for s in sums))
    # the sums before the shift: never negative (the shift needs no floor), inside int32
    assert min(lo) == 69206044 and max(hi) == 1008730084 and max(hi) < 2 ** 31


def test_grey_has_neutral_chroma_and_the_full_video_range():
    v = np.arange(256)
    for k in (0, 1, 2):
        U, V = er.chroma(v << k, v << k, v << k, k)
        assert (U == 128).all() and (V == 128).all()
    Y = er.luma(v, v, v)
    assert Y[0] == 16 and Y[255] == 235 and (np.diff(Y) >= 0).all()
    assert (Y == (900542 * v + (16 << 20) + (1 << 19)) >> 20).all()   # the header's grey row is the Y of (g, g, g)
    # and the exporter says the same, with and without the flag
    g = v.astype(np.uint8).reshape(16, 16)
    for name in er.YUV:
        Yp, Up, Vp = er.export(name, g, 0)
        assert (Yp == Y.reshape(16, 16)).all() and (Up == 128).all() and (Vp == 128).all()
        Yp, Up, Vp = er.export(name, g, er.GREY_IS_LUMA)
        assert (Yp == g).all() and (Up == 128).all() and (Vp == 128).all()
    # the flag means nothing for a B,G,R source or another destination
    bgr = np.random.default_rng(3).integers(0, 256, (4, 6, 3)).astype(np.uint8)
    for name in er.DESTINATIONS:
        assert er.export_raw(name, bgr, 0).tobytes() == er.export_raw(name, bgr, er.GREY_IS_LUMA).tobytes()
    for name in ("GRAY8", "BGR8", "RGB8", "BGRA8", "RGBA8"):
        assert er.export_raw(name, g, 0).tobytes() == er.export_raw(name, g, er.GREY_IS_LUMA).tobytes()


def test_export_then_ingest_returns_every_channel_within_two():
    for R, G, B in _chunks():
        U, V = er.chroma(R, G, B, 0)
        back = ir.yuv_to_bgr(er.luma(R, G, B), U, V)
        for got, want in zip(back, (B, G, R)):
            assert np.abs(got.astype(np.int64) - want).max() <= 2
    g = np.arange(256)
    for got in ir.yuv_to_bgr(er.luma(g, g, g), np.full(256, 128), np.full(256, 128)):
        assert np.abs(got.astype(np.int64) - g).max() <= 1


def test_packing_is_the_input_sides_and_the_simple_rows_are_what_they_say():
    rng = np.random.default_rng(4)
    bgr = rng.integers(0, 256, (4, 6, 3)).astype(np.uint8)
    g = rng.integers(0, 256, (4, 6)).astype(np.uint8)
    for name in er.DESTINATIONS:
        for img in (bgr, g):
            raw = er.export_raw(name, img)
            assert raw.shape == (ir.rows_of(name, 4), 6 * ir.BYTES_PER_PIXEL[name]) and raw.dtype == np.uint8
    # the packed colour formats and GRAY8 come back exactly through the input side
    for name in ("BGR8", "RGB8", "BGRA8", "RGBA8"):
        assert (ir.to_bgr(name, er.export_raw(name, bgr), 6, 4) == bgr).all()
        assert (ir.to_bgr(name, er.export_raw(name, g), 6, 4) == g[..., None]).all()
    assert (er.export_raw("BGRA8", bgr).reshape(4, 6, 4)[..., 3] == 255).all()
    assert (er.export_raw("GRAY8", g) == g).all()
    assert (er.export_raw("GRAY8", bgr) == ir.gray_of(bgr[..., 0], bgr[..., 1], bgr[..., 2])).all()
    # the Y plane of every YUV destination is the same, and ingest reads it back as the grey frame
    Y = er.export("NV12", bgr)[0]
    for name in er.YUV:
        assert (ir.to_gray(name, er.export_raw(name, bgr), 6, 4) == Y).all()
    # a block whose channel sums are odd: the box filter sums before it multiplies
    blk = np.array([[[1, 2, 4], [2, 5, 7]], [[3, 3, 9], [1, 1, 1]]], np.uint8)   # B,G,R sums 7, 11, 21
    U, V = er.export("NV12", blk)[1:]
    assert (int(U[0, 0]), int(V[0, 0])) == tuple(int(c) for c in er.chroma(21, 11, 7, 2))


def test_header_declares_and_library_exports_the_export_call():
    from aruco_amd import build_library, capi
    raw = open(os.path.join(ROOT, "include", "arucohip.h")).read()
    assert re.search(r"^#define\s+ARUCOHIP_EXPORT_GREY_IS_LUMA\s+1\s*$", raw, flags=re.M)
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert "arucohip_export_batch" in set(re.findall(r"\b(arucohip_[a-z_0-9]+)\s*\(", txt))
    lib = build_library()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "arucohip_export_batch" in set(l.split()[-1] for l in out.splitlines() if l.strip())
    assert "arucohip_export_batch" in capi.SYMBOLS and capi.EXPORT_GREY_IS_LUMA == er.GREY_IS_LUMA
    # no value was added to the pixel-format enum
    assert capi.PIX_NAMES == ir.FORMATS and capi.PIX_BAYER_GBRG == 12 and set(er.DESTINATIONS) | set(er.REFUSED) == set(ir.FORMATS)
