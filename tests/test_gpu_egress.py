"""Frames out on the device: arucohip_export_batch byte for byte against the numpy restatement of the definitions (tests/egress_ref.py;
integer arithmetic, so no tolerance), its refusals, the round trip through arucohip_convert_batch, and its place on the handle's stream:
behind a paint call, and in front of arucohip_detect_batch on the Y plane of the NV12 frames it wrote."""
import ctypes as C

import numpy as np
import pytest

from tests import egress_ref as er
from tests import ingest_ref as ir

pytestmark = pytest.mark.gpu

YUV_SIZES = [(2, 2), (4, 2), (6, 4), (1030, 4)]        # W x H; 1030: 258 quads, a second 256-lane block and a 2-pixel tail
ODD_SIZES = [(5, 3), (1029, 3)]                        # the destinations without chroma subsampling take odd sizes as well
NFRAMES = 3
SRC_FILL, DST_FILL = 0xA5, 0x5A
CAP = 32


@pytest.fixture(scope="module")
def env():
    import torch
    from aruco_amd import capi

    assert torch.cuda.is_available()
    capi.load()
    return {"capi": capi, "torch": torch}


@pytest.fixture(scope="module")
def eh(env):
    h = env["capi"].Handle(1040, 64, max_batch=NFRAMES)
    yield h
    h.close()


def _lay_out_src(imgs, srs, sfs, base):
    """images [n][H][W] or [n][H][W][3] in a flat buffer: frame f at base + f * sfs, rows srs apart, the sentinel between"""
    n, H = imgs.shape[:2]
    rows = imgs.reshape(n, H, -1)
    return ir.lay_out(rows, "GRAY8", H, srs, sfs, base, fill=SRC_FILL)[0]


def _export(env, h, name, imgs, flags, src_dev, dst_dev, srow_pad=0, sframe_gap=0, sbase=0, drow_pad=0, dframe_gap=0, dbase=0, chroma_gap=0):
    """arucohip_export_batch of images [n][H][W] (grey) or [n][H][W][3] (B,G,R) laid out with the given strides; asserts that the whole
    destination buffer equals the expected one: egress_ref's bytes, the sentinel everywhere else."""
    capi, torch = env["capi"], env["torch"]
    n, H, W = imgs.shape[:3]
    Cn = 1 if imgs.ndim == 3 else 3
    rb = W * ir.BYTES_PER_PIXEL[name]
    if name != "NV12":
        chroma_gap = 0
    if drow_pad == "dword":   # every stride a multiple of 4, whatever the width: rows, planes and frames start on dword boundaries
        srow_pad, drow_pad = (-W * Cn) % 4 + 4, (-rb) % 4 + 8
        sframe_gap = (-((W * Cn + srow_pad) * (H - 1) + W * Cn)) % 4 + 12
        chroma_gap = 32 if name == "NV12" else 0
        dframe_gap = (-ir.frame_bytes(name, W, H, rb + drow_pad, chroma_gap)) % 4 + 16
    srs = W * Cn + srow_pad
    sfs = srs * (H - 1) + W * Cn + sframe_gap
    buf = _lay_out_src(imgs, srs, sfs, sbase)
    drs = rb + drow_pad
    dfs = ir.frame_bytes(name, W, H, drs, chroma_gap) + dframe_gap
    raw = np.stack([er.export_raw(name, im, flags) for im in imgs])
    want, co = ir.lay_out(raw, name, H, drs, dfs, dbase, chroma_gap, fill=DST_FILL)
    fmt = capi.frame_format(name, chroma_offset=co if chroma_gap else 0)
    assert fmt.min_row_stride(W) == rb and fmt.min_stride(W, H, drs) == dfs - dframe_gap
    got = np.full_like(want, DST_FILL)
    if src_dev:
        s_t = torch.from_numpy(buf).cuda()
        sptr = s_t.data_ptr() + sbase
    else:
        sptr = buf.ctypes.data + sbase
    if dst_dev:
        d_t = torch.from_numpy(got).cuda()
        dptr = d_t.data_ptr() + dbase
    else:
        dptr = got.ctypes.data + dbase
    torch.cuda.synchronize()
    h.export_batch_ptr(sptr, Cn, n, W, H, fmt, dptr, drs, dfs, srs, sfs, flags=flags, src_on_device=src_dev, dst_on_device=dst_dev)
    if dst_dev:
        h.synchronize()
        got = d_t.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (name, W, H, Cn, flags, src_dev, dst_dev, drow_pad, dbase, "first differing byte", int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))


LAYOUTS = [
    # tight strides, aligned: the dword path (and its byte tail)
    dict(src_dev=True, dst_dev=True),
    dict(src_dev=False, dst_dev=False),
    # padded, still aligned: row, plane and frame gaps on the dword path
    dict(src_dev=True, dst_dev=True, drow_pad="dword"),
    # odd row padding, frame gaps and both bases off by one byte: the byte path on every quad
    dict(src_dev=True, dst_dev=True, srow_pad=3, sframe_gap=5, sbase=1, drow_pad=1, dframe_gap=7, dbase=1, chroma_gap=13),
    dict(src_dev=True, dst_dev=True, sbase=1, dbase=1),
    # host on one side, with padding the copies must keep: a host NV12 destination with an explicit gap before its chroma plane
    dict(src_dev=False, dst_dev=True, srow_pad=3, sframe_gap=5, sbase=1, chroma_gap=7),
    dict(src_dev=True, dst_dev=False, srow_pad=1, drow_pad=5, dframe_gap=3, chroma_gap=64),
    dict(src_dev=False, dst_dev=False, srow_pad=2, drow_pad=3, dframe_gap=9, dbase=1, chroma_gap=5),
]


def _sizes(name):
    return YUV_SIZES + ([] if name in er.YUV else ODD_SIZES)


def _random_images(rng, W, H, Cn, n=NFRAMES):
    return rng.integers(0, 256, (n, H, W) if Cn == 1 else (n, H, W, 3)).astype(np.uint8)


@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("name", er.DESTINATIONS)
def test_export_is_byte_identical_to_the_definition(env, eh, name, Cn):
    rng = np.random.default_rng(2000 + er.DESTINATIONS.index(name) * 2 + Cn)
    for W, H in _sizes(name):
        imgs = _random_images(rng, W, H, Cn)
        for flags in (0, er.GREY_IS_LUMA):
            for lay in LAYOUTS:
                _export(env, eh, name, imgs, flags, **lay)


def _extreme_images():
    """B,G,R frames 12 x 4: all 0, all 255, the six saturated primaries as 2 x 2 blocks and as single columns, and 2 x 2 blocks of four
    different colours whose channel sums are odd (a kernel that averages before it multiplies rounds them differently)."""
    prim = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [255, 0, 255], [0, 255, 255]], np.uint8)
    blocks = np.repeat(np.repeat(prim[None], 2, axis=1), 4, axis=0)             # [4][12][3]: every 2 x 2 block one primary
    columns = np.repeat(np.concatenate([prim, prim[::-1]])[None], 4, axis=0)    # neighbouring pixels of different primaries
    columns[1::2] = columns[1::2, ::-1]
    blk = np.array([[[1, 2, 4], [2, 5, 7]], [[3, 3, 9], [1, 1, 1]]], np.uint8)  # B,G,R sums 7, 11, 21
    odd = np.tile(blk, (2, 6, 1))
    odd[:, 6:] = 255 - odd[:, 6:]                                               # sums 1013, 1009, 999
    zeros, full = np.zeros((4, 12, 3), np.uint8), np.full((4, 12, 3), 255, np.uint8)
    return np.stack([zeros, full, blocks]), np.stack([odd, columns, zeros])


@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("name", er.DESTINATIONS)
def test_export_extremes(env, eh, name, Cn):
    for imgs in _extreme_images():
        if Cn == 1:
            imgs = np.ascontiguousarray(imgs[..., 1])
        for flags in (0, er.GREY_IS_LUMA):
            _export(env, eh, name, imgs, flags, True, True)
            _export(env, eh, name, imgs, flags, True, True, srow_pad=3, sbase=1, drow_pad=1, dbase=1)


@pytest.mark.parametrize("name", ["NV12", "YUYV"])
def test_export_then_convert_is_the_round_trip_of_the_definitions(env, eh, name):
    """arucohip_export_batch to device NV12 / YUYV, then arucohip_convert_batch back to B,G,R on the same stream: exactly ingest_ref's
    reading of egress_ref's frame, every channel within 2 of the image."""
    capi, torch = env["capi"], env["torch"]
    rng = np.random.default_rng(91)
    for W, H in ((6, 4), (1030, 4)):
        imgs = _random_images(rng, W, H, 3)
        fmt = capi.frame_format(name)
        rs = fmt.min_row_stride(W)
        fs = fmt.min_stride(W, H, rs)
        src = torch.from_numpy(imgs).cuda()
        mid = torch.zeros(NFRAMES * fs, dtype=torch.uint8, device="cuda")
        back = torch.zeros((NFRAMES, H, W, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        eh.export_batch_ptr(src.data_ptr(), 3, NFRAMES, W, H, fmt, mid.data_ptr())
        eh.convert_device(mid.data_ptr(), fmt, NFRAMES, W, H, rs, fs, 3, back.data_ptr())
        eh.synchronize()
        got = back.cpu().numpy()
        for f in range(NFRAMES):
            want = ir.to_bgr(name, er.export_raw(name, imgs[f]), W, H)
            assert got[f].tobytes() == want.tobytes()
        # smooth content survives within the bound of the definitions; random pixels share chroma with unlike neighbours and do not
        flat = np.repeat(np.repeat(imgs[:, ::2, ::2], 2, axis=1), 2, axis=2)
        src.copy_(torch.from_numpy(flat).cuda())
        torch.cuda.synchronize()
        eh.export_batch_ptr(src.data_ptr(), 3, NFRAMES, W, H, fmt, mid.data_ptr())
        eh.convert_device(mid.data_ptr(), fmt, NFRAMES, W, H, rs, fs, 3, back.data_ptr())
        eh.synchronize()
        assert np.abs(back.cpu().numpy().astype(int) - flat).max() <= 2


def test_host_wrapper_returns_the_frames_bytes(env, eh):
    capi = env["capi"]
    rng = np.random.default_rng(17)
    bgr, grey = _random_images(rng, 6, 4, 3), _random_images(rng, 6, 4, 1)
    for name in er.DESTINATIONS:
        for imgs in (bgr, grey):
            out = eh.export_frames(imgs, name)
            assert out.shape == (NFRAMES, ir.frame_bytes(name, 6, 4, 6 * ir.BYTES_PER_PIXEL[name]))
            for f in range(NFRAMES):
                assert out[f].tobytes() == er.export_raw(name, imgs[f]).tobytes()
    out = eh.export_frames(grey, capi.nv12(), row_stride=8, chroma_offset=40, flags=capi.EXPORT_GREY_IS_LUMA)
    want, co = ir.lay_out(np.stack([er.export_raw("NV12", g, er.GREY_IS_LUMA) for g in grey]), "NV12", 4, 8, out.shape[1], chroma_gap=8, fill=0)
    assert co == 40 and out.tobytes() == want[:out.size].tobytes()


# ---- refusals

def test_every_refusal_is_invalid_with_a_message_and_writes_nothing(env):
    capi = env["capi"]
    h = capi.Handle(64, 64, max_batch=2)
    try:
        L = h.L
        gray = np.random.default_rng(5).integers(0, 256, (2, 64, 64)).astype(np.uint8)
        exp = h.detect_batch_host(gray, cap=CAP)
        thr = h.thresholded(1, (64, 64)).copy()
        src = np.zeros(64 * 64 * 4 + 64, np.uint8)
        dst = np.full(64 * 64 * 4 + 64, DST_FILL, np.uint8)
        sp, dp = src.ctypes.data, dst.ctypes.data

        def call(fmt, W=8, H=8, Cn=1, srs=None, sfs=None, drs=None, dfs=None, s=sp, d=dp, nf=2, flags=0, fmt_ptr=True):
            srs = W * Cn if srs is None else srs
            sfs = srs * H if sfs is None else sfs
            drs = fmt.min_row_stride(W) if drs is None else drs
            dfs = drs * H * 2 if dfs is None else dfs
            return L.arucohip_export_batch(h.h, C.c_void_p(s), Cn, nf, W, H, srs, sfs, 0, C.byref(fmt) if fmt_ptr else None, flags, C.c_void_p(d), drs, dfs, 0)

        def refused(*a, **kw):
            rc = call(*a, **kw)
            msg = (L.arucohip_last_error_string(h.h) or b"").decode()
            assert rc == capi.E_INVALID and msg, (a, kw, rc, msg)
            assert (dst == DST_FILL).all(), (a, kw)
            return msg

        g8, bgra, yuyv, uyvy, nv12 = (capi.frame_format(n) for n in ("GRAY8", "BGRA8", "YUYV", "UYVY", "NV12"))
        for fmt in (g8, bgra, yuyv, uyvy, nv12, capi.frame_format("BGR8"), capi.frame_format("RGB8"), capi.frame_format("RGBA8")):
            for Cn in (1, 3):
                assert call(fmt, Cn=Cn) == capi.OK   # the helper's defaults are a valid call
                dst[:] = DST_FILL
        refused(g8, s=0), refused(g8, d=0), refused(g8, fmt_ptr=False)                    # NULL pointers
        refused(capi.FrameFormat(13, 0, 0), drs=8), refused(capi.FrameFormat(-1, 0, 0), drs=8)   # unknown format
        own = {refused(capi.gray16(12), drs=16)}                                          # input-only formats, each kind with its own message
        own.add(refused(capi.bayer("RGGB"), drs=8))
        for p in ("BGGR", "GRBG", "GBRG"):
            refused(capi.bayer(p), drs=8)
        assert len(own) == 2 and not own & {refused(capi.FrameFormat(13, 0, 0), drs=8)}
        for Cn in (0, 2, 4):
            refused(g8, Cn=Cn, srs=32)                                                    # src_channels
        refused(yuyv, W=7, drs=16), refused(uyvy, W=7, drs=16), refused(nv12, W=7, drs=8)  # odd width
        refused(nv12, H=7)                                                                # odd height
        for fmt in (g8, bgra, yuyv, nv12):
            refused(fmt, drs=fmt.min_row_stride(8) - 1)                                   # strides below the minimum
            refused(fmt, dfs=fmt.min_stride(8, 8, fmt.min_row_stride(8)) - 1)             # frame_stride does not cover a frame
            assert call(fmt, dfs=fmt.min_stride(8, 8, fmt.min_row_stride(8))) == capi.OK
            dst[:] = DST_FILL
        refused(g8, Cn=3, srs=23), refused(g8, srs=7)
        refused(g8, sfs=63), refused(g8, Cn=3, sfs=24 * 7 + 23)
        refused(capi.nv12(chroma_offset=63))                                              # chroma plane inside the Y plane
        refused(g8, nf=3), refused(g8, nf=0), refused(g8, W=65, drs=65), refused(g8, H=65), refused(g8, W=0)   # the handle's limits
        refused(g8, s=dp, d=dp)                                                           # dst overlaps src
        refused(g8, s=dp + 8 * 8 * 2 + 8 * 7 + 7, d=dp)                                   # ... by its last byte only (frames 128 apart)
        refused(g8, s=dp, d=dp + 8 * 8 + 8 * 7 + 7)
        assert call(g8, s=dp, d=dp + 8 * 8 + 8 * 7 + 8, dfs=64) == capi.OK
        dst[:] = DST_FILL
        refused(g8, flags=2), refused(nv12, flags=3), refused(g8, flags=-1)               # flag bits other than the one defined
        assert call(nv12, flags=1) == capi.OK
        # the last batch is still there
        assert (h.thresholded(1, (64, 64)) == thr).all()
        got = h.detect_batch_host(gray, cap=CAP)
        assert len(got) == len(exp) and all(g.tobytes() == e.tobytes() for g, e in zip(got, exp))
    finally:
        h.close()


# ---- on the handle's stream

@pytest.fixture(scope="module")
def scene(env):
    """one 640 x 480 B,G,R frame with markers (aruco_amd.synth), tinted so that the three channels differ"""
    from aruco_amd import synth
    rng = np.random.RandomState(31)
    lay = synth.frame_layout(rng, 640, 480, n_markers=6, side_range=(60, 110), margin=20)
    g = synth.render_frame(lay, 640, 480, rng, device="cpu").numpy()
    return np.stack([(g.astype(np.uint16) * 3 // 4).astype(np.uint8), g, 255 - (255 - g) // 2], axis=-1)


class _DeviceResults:
    """marker and count arrays of one frame in device memory"""

    def __init__(self, env):
        self.capi, torch = env["capi"], env["torch"]
        self.out = torch.zeros(CAP * self.capi.MARKER_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        self.n = torch.zeros(1, dtype=torch.int32, device="cuda")

    def markers(self):
        return self.out.cpu().numpy().view(self.capi.MARKER_DTYPE)[:int(self.n.cpu()[0])]


def test_export_to_nv12_then_detect_on_its_y_plane_without_synchronising(env, scene):
    capi, torch = env["capi"], env["torch"]
    W, H, rs = 640, 480, 704   # an encoder surface's pitch
    fmt = capi.nv12()
    h = capi.Handle(W, H)
    try:
        Y = er.export("NV12", scene)[0]
        exp = h.detect_batch_host(Y[None], cap=CAP)[0]
        assert len(exp) >= 2
        src = torch.from_numpy(scene).cuda()
        surf = torch.full((fmt.min_stride(W, H, rs),), DST_FILL, dtype=torch.uint8, device="cuda")
        res = _DeviceResults(env)
        torch.cuda.synchronize()
        h.export_batch_ptr(src.data_ptr(), 3, 1, W, H, fmt, surf.data_ptr(), dst_row_stride=rs)
        h.detect_batch_device(surf.data_ptr(), 1, W, H, res.out.data_ptr(), CAP, res.n.data_ptr(), row_stride=rs)
        h.batch_status()
        got = res.markers()
        assert [int(m["id"]) for m in got] == [int(m["id"]) for m in exp]
        assert got.tobytes() == exp.tobytes()
        want, _ = ir.lay_out(er.export_raw("NV12", scene)[None], "NV12", H, rs, surf.numel(), fill=DST_FILL)
        assert surf.cpu().numpy().tobytes() == want[:surf.numel()].tobytes()
    finally:
        h.close()


def test_export_to_bgra_behind_a_paint_call_on_the_same_stream(env, scene):
    capi, torch = env["capi"], env["torch"]
    W, H = 640, 480
    h = capi.Handle(W, H)
    try:
        gray = ir.gray_of(scene[..., 0], scene[..., 1], scene[..., 2])
        markers = h.detect_batch_host(gray[None], cap=CAP)[0]
        assert len(markers) >= 2
        mk = np.zeros((1, CAP), capi.MARKER_DTYPE)
        mk[0, :len(markers)] = markers
        d_mk = torch.from_numpy(mk.view(np.uint8).reshape(-1)).cuda()
        d_n = torch.tensor([len(markers)], dtype=torch.int32, device="cuda")
        frames = torch.from_numpy(scene[None].copy()).cuda()
        fmt = capi.frame_format("BGRA8")
        out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        h.draw_markers(frames, d_mk, d_n, line_width=2, color=(0, 255, 0))
        h.export_batch_ptr(frames.data_ptr(), 3, 1, W, H, fmt, out.data_ptr())
        h.synchronize()
        painted = frames[0].cpu().numpy()
        assert (painted != scene).any()
        assert out.cpu().numpy().tobytes() == er.export_raw("BGRA8", painted).tobytes()
    finally:
        h.close()
