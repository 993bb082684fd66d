"""Camera-native input on the device: arucohip_convert_batch byte for byte against the numpy restatement of the definitions
(tests/ingest_ref.py; integer arithmetic, so no tolerance), its refusals, and the route from it to the detector: frames converted to grey
in device memory and read there by arucohip_detect_batch, against a host call on ingest_ref's grey conversion of the same encoded bytes."""
import ctypes as C

import numpy as np
import pytest

from tests import ingest_ref as ir

pytestmark = pytest.mark.gpu

SIZES = [(2, 2), (4, 2), (6, 4), (10, 6), (1030, 4)]        # W x H; 1030 crosses a 256-lane block at 4 pixels per lane
BAYER_SIZES = [(3, 3), (5, 2), (1029, 3)]
NFRAMES = 3
BITS = 12
SRC_FILL, DST_FILL = 0xA5, 0x5A
K = np.array([[300.0, 0, 160.0], [0, 300.0, 120.0], [0, 0, 1]], np.float32)
MARKER_SIZE = 0.05
CAP = 32


@pytest.fixture(scope="module")
def env():
    import torch
    from aruco_amd import capi

    assert torch.cuda.is_available()
    capi.load()
    return {"capi": capi, "torch": torch}


@pytest.fixture(scope="module")
def ch(env):
    h = env["capi"].Handle(1040, 64, max_batch=NFRAMES)
    yield h
    h.close()


def _fmt(capi, name, chroma_offset=0):
    return capi.frame_format(name, bits=BITS if name == "GRAY16" else 0, chroma_offset=chroma_offset)


def _convert(env, h, name, frames, W, H, Cn, src_dev, dst_dev, row_pad=0, frame_gap=0, base=0, chroma_gap=0, drow_pad=0, dframe_gap=0, dbase=0):
    """arucohip_convert_batch of tightly packed raw frames [n][rows][row bytes] laid out with the given strides; returns nothing, asserts
    that the whole destination buffer equals the expected one: ingest_ref's pixels, the sentinel everywhere else."""
    capi, torch = env["capi"], env["torch"]
    n, rb = frames.shape[0], frames.shape[2]
    if row_pad == "dword":   # every stride a multiple of 4, whatever the width: rows and frames start on dword boundaries
        row_pad, drow_pad = (-rb) % 4 + 8, (-W * Cn) % 4 + 4
        frame_gap = (-ir.frame_bytes(name, W, H, rb + row_pad, chroma_gap)) % 4 + 16
        dframe_gap = 12
    rs = rb + row_pad
    fs = ir.frame_bytes(name, W, H, rs, chroma_gap) + frame_gap
    buf, co = ir.lay_out(frames, name, H, rs, fs, base, chroma_gap, fill=SRC_FILL)
    fmt = _fmt(capi, name, co if chroma_gap else 0)
    assert fmt.min_stride(W, H, rs) == fs - frame_gap
    drs = W * Cn + drow_pad
    dfs = drs * H + dframe_gap
    want = np.full(dbase + n * dfs + 8, DST_FILL, np.uint8)
    for f in range(n):
        ref = ir.convert(name, frames[f], W, H, Cn, BITS).reshape(H, W * Cn)
        for y in range(H):
            at = dbase + f * dfs + y * drs
            want[at:at + W * Cn] = ref[y]
    got = np.full_like(want, DST_FILL)
    if src_dev:
        s_t = torch.from_numpy(buf).cuda()
        sptr = s_t.data_ptr() + base
    else:
        sptr = buf.ctypes.data + base
    if dst_dev:
        d_t = torch.from_numpy(got).cuda()
        dptr = d_t.data_ptr() + dbase
    else:
        dptr = got.ctypes.data + dbase
    torch.cuda.synchronize()
    h.convert_device(sptr, fmt, n, W, H, rs, fs, Cn, dptr, drs, dfs, src_on_device=src_dev, dst_on_device=dst_dev)
    if dst_dev:
        h.synchronize()
        got = d_t.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (name, W, H, Cn, src_dev, dst_dev, row_pad, base, "first differing byte", int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))


LAYOUTS = [
    # tight strides, aligned: the dword path (and its byte tail)
    dict(src_dev=True, dst_dev=True),
    dict(src_dev=False, dst_dev=False),
    # padded, still aligned: row and frame gaps on the dword path
    dict(src_dev=True, dst_dev=True, row_pad="dword", chroma_gap=32),
    # odd row padding, a frame gap and a source base off by one byte: the byte-wise path
    dict(src_dev=True, dst_dev=True, row_pad=3, frame_gap=5, base=1, drow_pad=1, dframe_gap=7, dbase=1),
    dict(src_dev=False, dst_dev=True, row_pad=3, frame_gap=5, base=1, chroma_gap=7),
    dict(src_dev=True, dst_dev=False, row_pad=1, drow_pad=5, dframe_gap=3),
]


def _sizes(name):
    return SIZES + (BAYER_SIZES if name.startswith("BAYER_") else [])


@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("name", ir.FORMATS)
def test_convert_is_byte_identical_to_the_definition(env, ch, name, Cn):
    rng = np.random.default_rng(1000 + ir.FORMATS.index(name) * 2 + Cn)
    for W, H in _sizes(name):
        frames = np.stack([ir.random_raw(name, W, H, rng) for _ in range(NFRAMES)])
        for lay in LAYOUTS:
            kw = dict(lay)
            if name != "NV12":
                kw.pop("chroma_gap", None)
            _convert(env, ch, name, frames, W, H, Cn, **kw)


@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("name", ir.FORMATS)
def test_convert_extremes(env, ch, name, Cn):
    """All 0, all 255, and for the YUV formats every combination of Y, U, V in 0, 16, 128, 235, 255."""
    W, H = 10, 6
    rows, rb = ir.rows_of(name, H), W * ir.BYTES_PER_PIXEL[name]
    frames = np.stack([np.zeros((rows, rb), np.uint8), np.full((rows, rb), 255, np.uint8), np.full((rows, rb), 128, np.uint8)])
    _convert(env, ch, name, frames, W, H, Cn, True, True)
    _convert(env, ch, name, frames, W, H, Cn, True, True, row_pad=3, base=1)
    if name in ("YUYV", "UYVY", "NV12"):
        lv = np.array([0, 16, 128, 235, 255], np.uint8)
        y, u, v = (a.ravel() for a in np.meshgrid(lv, lv, lv, indexing="ij"))   # 125 combinations, one per pixel pair
        W, H = 250, 2
        Y = np.repeat(y, 2)[None].repeat(H, axis=0)
        if name == "NV12":
            raw = ir.pack_nv12(Y, u[None], v[None])
        else:
            raw = ir.pack_yuv422(Y, u[None].repeat(H, axis=0), v[None].repeat(H, axis=0), name)
        frames = np.stack([raw] * NFRAMES)
        _convert(env, ch, name, frames, W, H, Cn, True, True)
        _convert(env, ch, name, frames, W, H, Cn, True, True, row_pad=1)


def test_nv12_with_an_explicit_chroma_offset(env, ch):
    rng = np.random.default_rng(77)
    for W, H in ((6, 4), (1030, 4)):
        frames = np.stack([ir.random_raw("NV12", W, H, rng) for _ in range(NFRAMES)])
        for gap in (64, 13):   # an aligned surface height, and one that forces the byte-wise path
            for Cn in (1, 3):
                _convert(env, ch, "NV12", frames, W, H, Cn, True, True, row_pad=2, chroma_gap=gap, frame_gap=gap)
                _convert(env, ch, "NV12", frames, W, H, Cn, False, False, row_pad=2, chroma_gap=gap, frame_gap=gap)


# ---- beside the detector

@pytest.fixture(scope="module")
def scene(env):
    return ir.scene()


@pytest.fixture
def make_handle(env):
    """handles of one test (320 x 240, two frames), closed after it; subpix: SUBPIX corner refinement, which reads the grey pixels"""
    capi = env["capi"]
    made = []

    def make(subpix=False):
        p = capi.default_params()
        if subpix:
            p.corner_method = capi.CORNER_SUBPIX
        made.append(capi.Handle(320, 240, max_batch=2, params=p))
        return made[-1]

    yield make
    for h in made:
        h.close()


@pytest.fixture
def dh(make_handle):
    return make_handle()


def _same(got, exp):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert g.tobytes() == e.tobytes()


class _DeviceResults:
    """marker and count arrays of `n` frames in device memory"""

    def __init__(self, env, n):
        self.capi, torch = env["capi"], env["torch"]
        self.frames = n
        self.out = torch.zeros(n * CAP * self.capi.MARKER_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        self.n = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

    def lists(self):
        n_h = self.n.cpu().numpy()
        out_h = self.out.cpu().numpy().view(self.capi.MARKER_DTYPE).reshape(self.frames, CAP)
        return [out_h[f, :n_h[f]] for f in range(self.frames)]


def _to_device_grey(env, h, name, raw):
    """the raw host frames go up and are converted to grey in device memory, asynchronously on h's stream"""
    d_gray = env["torch"].zeros((raw.shape[0], 240, 320), dtype=env["torch"].uint8, device="cuda")
    env["torch"].cuda.synchronize()
    rs = raw.shape[2]
    h.convert_device(raw.ctypes.data, _fmt(env["capi"], name), raw.shape[0], 320, 240, rs, raw.shape[1] * rs, 1, d_gray.data_ptr(), src_on_device=False)
    return d_gray


@pytest.mark.parametrize("name", ir.FORMATS)
def test_convert_on_the_device_then_detect(env, make_handle, scene, name):
    """The route of a camera-native frame to the detector: arucohip_convert_batch into device grey, then the existing calls with
    frames_on_device = 1. The markers are, byte for byte, those of arucohip_detect_batch on ingest_ref's grey conversion of the same encoded
    bytes: with poses, with LINES and with SUBPIX refinement, one frame per call twice in a row, through submit / wait at pipeline depth 2 and
    with arucohip_set_pyr_down(1). Lanes and pyrDown run on handles of their own."""
    rng = np.random.default_rng(300 + ir.FORMATS.index(name))
    raw = np.stack([ir.encode(name, g, rng, bits=BITS) for g in scene])
    gray = np.stack([ir.to_gray(name, r, 320, 240, BITS) for r in raw])
    kw = dict(K=K, marker_size=MARKER_SIZE)
    for subpix in (False, True):
        h = make_handle(subpix)
        exp = h.detect_batch_host(gray, cap=CAP, **kw)
        if not name.startswith("BAYER_"):   # these carry the scene's grey values exactly; the demosaic of a grey mosaic smooths them
            assert (gray == scene).all() and all(len(e) >= 2 for e in exp)
        d_gray = _to_device_grey(env, h, name, raw)
        res = _DeviceResults(env, 2)
        h.detect_batch_device(d_gray.data_ptr(), 2, 320, 240, res.out.data_ptr(), CAP, res.n.data_ptr(), **kw)
        h.batch_status()
        assert (d_gray.cpu().numpy() == gray).all()
        _same(res.lists(), exp)
        one = _DeviceResults(env, 1)
        for f in (0, 1, 1, 0):   # one frame per call; each frame twice in a row
            h.detect_batch_device(d_gray.data_ptr() + f * 320 * 240, 1, 320, 240, one.out.data_ptr(), CAP, one.n.data_ptr(), **kw)
            h.batch_status()
            _same(one.lists(), [exp[f]])
    # batches in flight at depth 2: the conversion is queued on the handle's stream, the lanes start behind it
    h = make_handle(True)
    exp = h.detect_batch_host(gray, cap=CAP, **kw)
    h.set_pipeline_depth(2)
    d_gray = _to_device_grey(env, h, name, raw)
    res = [_DeviceResults(env, 2) for _ in range(2)]
    tickets = [h.submit_device(d_gray.data_ptr(), 2, 320, 240, r.out.data_ptr(), CAP, r.n.data_ptr(), **kw) for r in res]
    for t, r in zip(tickets, res):
        h.wait(t)
        _same(r.lists(), exp)
    # detection on the reduced image: threshold and contours on the pyramid of the converted frames, decoding and SUBPIX on the frames
    h = make_handle(True)
    h.set_pyr_down(1)
    exp = h.detect_batch_host(gray, cap=CAP, **kw)
    d_gray = _to_device_grey(env, h, name, raw)
    r = _DeviceResults(env, 2)
    h.detect_batch_device(d_gray.data_ptr(), 2, 320, 240, r.out.data_ptr(), CAP, r.n.data_ptr(), **kw)
    h.batch_status()
    _same(r.lists(), exp)


def test_nv12_device_surface_is_a_grey_frame_as_it_lies(env, dh, scene):
    """The Y plane of an NV12 device surface goes to arucohip_detect_batch where it is, with the surface's pitch as row_stride and the
    distance between surfaces as frame_stride (the U,V plane lies behind the Y plane, inside that distance): the thresholded images and
    the markers are those of a grey call on the Y planes alone."""
    capi, torch = env["capi"], env["torch"]
    rng = np.random.default_rng(55)
    raw = np.stack([ir.encode("NV12", g, rng) for g in scene])
    rs = 320 + 64
    fs = ir.frame_bytes("NV12", 320, 240, rs) + 128
    buf, _ = ir.lay_out(raw, "NV12", 240, rs, fs, fill=SRC_FILL)
    exp = dh.detect_batch_host(scene, cap=CAP)
    thr = [dh.thresholded(f, (240, 320)).copy() for f in range(2)]
    assert all(len(e) >= 2 for e in exp)
    d = torch.from_numpy(buf).cuda()
    res = _DeviceResults(env, 2)
    dh.detect_batch_device(d.data_ptr(), 2, 320, 240, res.out.data_ptr(), CAP, res.n.data_ptr(), row_stride=rs, frame_stride=fs)
    dh.batch_status()
    for f in range(2):
        assert (dh.thresholded(f, (240, 320)) == thr[f]).all()
    _same(res.lists(), exp)
    # and the colour of the same surfaces, for the consumers that want it
    bgr = torch.zeros((2, 240, 320, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    dh.convert_device(d.data_ptr(), capi.nv12(), 2, 320, 240, rs, fs, 3, bgr.data_ptr())
    dh.synchronize()
    assert all((bgr[f].cpu().numpy() == ir.to_bgr("NV12", raw[f], 320, 240)).all() for f in range(2))


def test_existing_calls_are_unchanged_by_a_conversion(env, dh, scene):
    capi = env["capi"]
    h = dh
    bgr = np.repeat(scene[..., None], 3, axis=-1)
    bgr[..., 0] = scene // 2   # a real colour image: the three channels differ
    before = (h.detect_batch_host(scene, cap=CAP), h.detect_batch_bgr_host(bgr, cap=CAP), h.detect(scene[0], cap=CAP), h.detect_bgr(bgr[0], cap=CAP))
    raw = np.stack([ir.mosaic(f, "GRBG") for f in bgr])
    got = h.convert(raw, capi.bayer("GRBG"), 3, 320, 240)
    assert all((got[f] == ir.to_bgr("BAYER_GRBG", raw[f], 320, 240)).all() for f in range(2))
    # BGR8 to grey is arucohip_bgr_to_gray's conversion
    assert (h.convert(bgr.reshape(2, 240, 960), capi.frame_format("BGR8"), 1, 320, 240)[1] == h.bgr_to_gray(bgr[1])).all()
    after = (h.detect_batch_host(scene, cap=CAP), h.detect_batch_bgr_host(bgr, cap=CAP), h.detect(scene[0], cap=CAP), h.detect_bgr(bgr[0], cap=CAP))
    _same(before[0], after[0])
    _same(before[1], after[1])
    _same([before[2], before[3]], [after[2], after[3]])


def test_every_refusal_is_invalid_and_keeps_the_last_batch(env, dh, scene):
    capi = env["capi"]
    h = dh
    L = h.L
    exp = h.detect_batch_host(scene, cap=CAP)
    thr = h.thresholded(1, (240, 320)).copy()
    src = np.zeros(64 * 64 * 4 + 64, np.uint8)
    dst = np.zeros(64 * 64 * 4 + 64, np.uint8)
    sp, dp = src.ctypes.data, dst.ctypes.data

    def call(fmt, W=8, H=8, rs=None, fs=None, Cn=1, drs=None, dfs=None, s=sp, d=dp, nf=2):
        rs = fmt.min_row_stride(W) if rs is None else rs
        fs = rs * H * 2 if fs is None else fs
        drs = W * Cn if drs is None else drs
        dfs = drs * H if dfs is None else dfs
        return L.arucohip_convert_batch(h.h, C.c_void_p(s), C.byref(fmt), nf, W, H, rs, fs, 0, Cn, C.c_void_p(d), drs, dfs, 0)

    g8, yuyv, nv12, rggb = capi.frame_format("GRAY8"), capi.frame_format("YUYV"), capi.nv12(), capi.bayer("RGGB")
    assert call(g8) == capi.OK   # the helper's defaults are a valid call
    assert call(capi.FrameFormat(13, 0, 0), rs=8) == capi.E_INVALID                    # unknown format
    assert call(capi.FrameFormat(-1, 0, 0), rs=8) == capi.E_INVALID
    assert call(capi.gray16(7), rs=16) == capi.E_INVALID                               # bits outside 8..16
    assert call(capi.gray16(17), rs=16) == capi.E_INVALID
    assert call(yuyv, W=7, rs=16) == capi.E_INVALID                                    # odd width
    assert call(capi.frame_format("UYVY"), W=7, rs=16) == capi.E_INVALID
    assert call(nv12, W=7, rs=8) == capi.E_INVALID
    assert call(nv12, H=7, rs=8) == capi.E_INVALID                                     # odd height
    assert call(rggb, W=1, rs=8) == capi.E_INVALID                                     # a Bayer frame below 2 x 2
    assert call(rggb, H=1, rs=8) == capi.E_INVALID
    for fmt in (g8, yuyv, nv12, rggb, capi.frame_format("RGB8"), capi.frame_format("BGRA8"), capi.gray16(12)):
        assert call(fmt, rs=fmt.min_row_stride(8) - 1) == capi.E_INVALID                # row_stride below the minimum
        assert call(fmt, fs=fmt.min_stride(8, 8, fmt.min_row_stride(8)) - 1) == capi.E_INVALID   # frame_stride below one frame
        assert call(fmt, fs=fmt.min_stride(8, 8, fmt.min_row_stride(8))) == capi.OK
    assert call(capi.nv12(chroma_offset=63), rs=8) == capi.E_INVALID                   # chroma plane inside the Y plane
    assert call(g8, Cn=2) == capi.E_INVALID and call(g8, Cn=0) == capi.E_INVALID and call(g8, Cn=4) == capi.E_INVALID
    assert call(g8, Cn=3, drs=23) == capi.E_INVALID                                    # dst strides below the minimum
    assert call(g8, dfs=63) == capi.E_INVALID
    assert call(g8, d=sp) == capi.E_INVALID                                            # dst overlaps src
    assert call(g8, d=sp + 8 * 8 * 2 + 8 * 7 + 7) == capi.E_INVALID                    # ... by its first byte only
    assert call(g8, d=sp + 8 * 8 * 2 + 8 * 7 + 8) == capi.OK
    assert call(g8, s=dp + 8 * 8 + 8 * 7 + 7, d=dp) == capi.E_INVALID
    assert call(g8, nf=3) == capi.E_INVALID and call(g8, W=321, rs=321) == capi.E_INVALID   # the handle's limits
    # the last batch is still there
    assert (h.thresholded(1, (240, 320)) == thr).all()
    _same(h.detect_batch_host(scene, cap=CAP), exp)
