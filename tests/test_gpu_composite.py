"""Plane compositing on the device against tests/composite_ref.py. Caller maps: bytes, no tolerance (the projection is the same IEEE
double arithmetic on both sides). Board call: the maps differ from numpy's in sin and cos only, so they are compared within 1e-12 and the
images byte for byte with the reference run on the maps the call returned. Small shapes: 96 x 64 frames, 40 x 30 textures, 5 frames."""
import ctypes

import numpy as np
import pytest

from tests import composite_ref as cr
from tests import rectify_ref as rr
from tests.test_gpu_rectify import DIST8, K_SMALL, POSE_LIKE, SENT, board_case, mismatch

pytestmark = pytest.mark.gpu

W, H, TW, TH, N = 96, 64, 40, 30, 5


def eye(ds=0.0, dt=0.0):
    return np.array([[1, 0, ds], [0, 1, dt], [0, 0, 1]], np.float64)


MAGNIFY = np.array([[0.3, 0, 0.25], [0, 0.45, 0.5], [0, 0, 1.0]])       # a texel covers about 3 x 2 frame pixels
MINIFY = np.array([[2.5, 0, -10.0], [0, 2.2, -7.0], [0, 0, 1.0]])       # the texture fits into 16 x 14 frame pixels
# Q = 1 - u / 40 - v / 90 changes sign inside the frame
PERSPECTIVE = np.array([[0.9, 0.1, 4.0], [-0.05, 1.1, 1.5], [-1 / 40.0, -1 / 90.0, 1.0]])
BASIC = [eye(), eye(-3, 2), eye(-0.5, 0), eye(1 / 64, 3 / 64), PERSPECTIVE]
nan_map, inf_map = eye(), eye()
nan_map[1, 1], inf_map[0, 2] = np.nan, np.inf
DEGENERATE = [np.array([[1e12, 0, 1e12], [0, 1e12, 1e12], [0, 0, 1.0]]), nan_map, inf_map, MAGNIFY, MINIFY]
# ray -> texel: test_gpu_rectify's window -> camera maps inverted, the 70 x 50 window scaled onto the 40 x 30 texture
RAY_TO_TEXEL = [np.diag([39 / 69.0, 29 / 49.0, 1.0]) @ cr.inverse_map(M)[0].reshape(3, 3) for M in POSE_LIKE]
# ... and composed with the pixel -> ray step, for a call without a camera
PIXEL_TO_TEXEL = [R @ np.linalg.inv(K_SMALL.astype(np.float64)) for R in RAY_TO_TEXEL]


@pytest.fixture(scope="module")
def handle():
    from aruco_amd import capi

    h = capi.Handle(640, 480, max_batch=4)
    yield h
    h.close()


_CACHE = {}


def source(cn, w=W, h=H):
    """the frames before the call, uint8 [N][h][w] (x 3)"""
    key = ("src", cn, w, h)
    if key not in _CACHE:
        _CACHE[key] = np.random.RandomState(21 + cn).randint(0, 256, (N, h, w) if cn == 1 else (N, h, w, 3)).astype(np.uint8)
    return _CACHE[key]


def textures(cn, alpha=None, tw=TW, th=TH):
    """N textures uint8 [N][th][tw][cn or cn + 1]; alpha: None (no channel), 0, 255 or "ramp" (0 .. 255 along the columns)"""
    key = ("tex", cn, alpha, tw, th)
    if key not in _CACHE:
        t = np.random.RandomState(31 + cn).randint(0, 256, (N, th, tw, cn + (alpha is not None))).astype(np.uint8)
        if alpha is not None:
            t[..., cn] = np.linspace(0, 255, tw).astype(np.uint8)[None, None, :] if alpha == "ramp" else alpha
        _CACHE[key] = t
    return _CACHE[key]


def checkerboard():
    y, x = np.mgrid[0:H, 0:W]
    return np.broadcast_to((((x // 3) + (y // 2)) & 1).astype(np.uint8), (N, H, W)).copy()


class Frames:
    """The frames of a call: rows of (w + 3) * cn bytes, frames a row and 11 bytes apart, starting at an odd address, 0xA5 in every byte
    that is not an image's (test_gpu_rectify's Dst, filled with the source)."""

    def __init__(self, images, device):
        self.n, self.h, self.w = images.shape[:3]
        self.cn = 1 if images.ndim == 3 else 3
        self.device = device
        self.row, self.frame = (self.w + 3) * self.cn, (self.w + 3) * self.cn * (self.h + 1) + 11
        buf = np.full(1 + self.n * self.frame + 16, SENT, np.uint8)
        flat = images.reshape(self.n, self.h, self.w * self.cn)
        for f in range(self.n):
            for y in range(self.h):
                at = 1 + f * self.frame + y * self.row
                buf[at:at + self.w * self.cn] = flat[f, y]
        if device:
            import torch

            self.buf = torch.from_numpy(buf).cuda()
            self.ptr = self.buf.data_ptr() + 1
        else:
            self.buf = buf
            self.ptr = self.buf.ctypes.data + 1
        assert self.ptr % 2 == 1

    def split(self):
        """(the images [n][h][w](x 3), whether every other byte still holds the sentinel)"""
        if self.device:
            import torch

            torch.cuda.synchronize()
            b = self.buf.cpu().numpy().copy()
        else:
            b = self.buf.copy()
        out = np.zeros((self.n, self.h, self.w * self.cn), np.uint8)
        for f in range(self.n):
            for y in range(self.h):
                at = 1 + f * self.frame + y * self.row
                out[f, y] = b[at:at + self.w * self.cn]
                b[at:at + self.w * self.cn] = SENT
        return (out if self.cn == 1 else out.reshape(self.n, self.h, self.w, 3)), bool((b == SENT).all())


def reference(src, tex, maps, K=None, dist=None, valid=None, opacity=255, masks=None, per_frame=False):
    """(the painted frames, the painted pixels of each)"""
    out = [cr.composite(src[f], tex[f if per_frame else 0], maps[f], K, dist, True if valid is None else bool(valid[f]), opacity,
                        None if masks is None else masks[f]) for f in range(len(maps))]
    return np.stack([o[0] for o in out]), np.array([o[1].sum() for o in out])


def run(handle, src, tex, maps, K=None, dist=None, valid=None, opacity=255, masks=None, per_frame=False, device=False):
    """arucohip_composite_plane_batch with everything on the host or everything on the device"""
    from aruco_amd import capi

    n, cn = len(maps), 1 if src.ndim == 3 else 3
    fr = Frames(src[:n], device)
    m = np.ascontiguousarray(np.asarray(maps, np.float64).reshape(n, 9))
    v = None if valid is None else np.ascontiguousarray(valid, np.int32)
    t = np.ascontiguousarray(tex if per_frame else tex[0])
    if device:
        import torch

        keep = [torch.from_numpy(a).cuda() if a is not None else None for a in (t, m, v, masks)]
        dt, dm, dv, dk = keep
        handle.composite_plane_device(fr.ptr, n, fr.w, fr.h, cn, capi.texture(dt, opacity, per_frame), dm.data_ptr(), K, dist,
                                      None if dv is None else dv.data_ptr(), None if dk is None else dk.data_ptr(), fr.row, fr.frame)
        handle.synchronize()
    else:
        handle.composite_plane_device(fr.ptr, n, fr.w, fr.h, cn, capi.texture(t, opacity, per_frame), m.ctypes.data, K, dist,
                                      None if v is None else v.ctypes.data, None if masks is None else masks.ctypes.data, fr.row, fr.frame,
                                      frames_on_device=0, maps_on_device=0, masks_on_device=0)
    return fr.split()


def check(handle, src, tex, maps, want=None, devices=(False, True), **kw):
    """both residences equal the reference byte for byte and write nothing else; returns the reference's (frames, painted counts)"""
    want = reference(src, tex, maps, **kw) if want is None else want
    for device in devices:
        got, clean = run(handle, src, tex, maps, device=device, **kw)
        assert not mismatch(got, want[0]), (device, mismatch(got, want[0]))
        assert clean, "bytes outside the images were written"
    return want


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("name,maps", [("basic", BASIC), ("degenerate", DEGENERATE)])
def test_caller_maps_equal_the_reference(handle, cn, name, maps):
    src, tex = source(cn), textures(cn)
    want, painted = reference(src, tex, maps)
    if name == "basic":
        assert painted[0] == TW * TH and np.array_equal(want[0][:TH, :TW].reshape(TH, TW, cn), tex[0])    # identity
        assert painted[1] == TW * (TH - 2) and np.array_equal(want[1][:, :3], src[1][:, :3])                # s = u - 3, t = v + 2: 3 columns keep
        assert painted[2] == (TW - 1) * TH and painted[3] == TW * (TH - 1)                                  # half a texel in x; ay = 2 in y
        assert 0 < painted[4] < 900 and np.array_equal(want[4][:, 45:], src[4][:, 45:])                     # behind the line where Q changes sign
    else:
        assert painted[:3].tolist() == [0, 0, 0] and np.array_equal(want[:3], src[:3])                     # saturated, NaN, Inf: untouched
        assert painted[3] == W * H and 150 < painted[4] < 16 * 14 + 1                                       # magnified all over; minified
    check(handle, src, tex, maps, (want, painted))


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("camera", ["none", "K", 4, 5, 8])
def test_camera_and_distortion(handle, cn, camera):
    src, tex = source(cn), textures(cn)
    if camera == "none":
        maps, K, dist = PIXEL_TO_TEXEL, None, None
    else:
        maps, K, dist = RAY_TO_TEXEL, K_SMALL, (None if camera == "K" else DIST8[:camera])
    want = reference(src, tex, maps, K, dist)
    assert want[1].min() > 1500
    if camera == 8:
        assert mismatch(want[0], reference(src, tex, maps, K, DIST8[:5])[0])    # the rational terms change the frames
    check(handle, src, tex, maps, want, devices=(camera != 4,), K=K, dist=dist)


@pytest.mark.parametrize("cn", [1, 3])
def test_valid_flags_opacity_and_masks(handle, cn):
    src, tex = source(cn), textures(cn)
    valid = [1, 0, 1, 1, 0]
    want = check(handle, src, tex, BASIC, valid=valid)
    assert want[1][1] == want[1][4] == 0 and np.array_equal(want[0][1], src[1]) and want[1][0] == TW * TH
    want = check(handle, src, tex, BASIC, opacity=0)
    assert np.array_equal(want[0], src) and not want[1].any()                      # opacity 0: byte-identical to before
    solid = check(handle, src, tex, BASIC)
    half = check(handle, src, tex, BASIC, opacity=128)
    assert np.array_equal(half[1], solid[1]) and mismatch(half[0], solid[0]) and mismatch(half[0], src)
    masked = check(handle, src, tex, BASIC, masks=checkerboard())
    assert 0 < masked[1][0] < solid[1][0]
    none = check(handle, src, tex, BASIC, masks=np.zeros((N, H, W), np.uint8))
    assert np.array_equal(none[0], src)


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("alpha", [0, 255, "ramp"])
def test_alpha_textures(handle, cn, alpha):
    src, tex = source(cn), textures(cn, alpha)
    for opacity in (255, 128):
        want = check(handle, src, tex, [eye(), MAGNIFY, eye(-0.5, -0.25)], opacity=opacity)
        if alpha == 0:
            assert np.array_equal(want[0], src[:3]) and not want[1].any()
        elif alpha == 255 and opacity == 255:
            assert np.array_equal(want[0][0][:TH, :TW].reshape(TH, TW, cn), tex[0][..., :cn])
        else:
            assert 0 < want[1][0] <= TW * TH and mismatch(want[0], src[:3])


@pytest.mark.parametrize("cn", [1, 3])
def test_one_texture_against_one_per_frame(handle, cn):
    src, tex = source(cn), textures(cn, "ramp")
    shared = check(handle, src, tex, BASIC)
    each = check(handle, src, tex, BASIC, per_frame=True)
    assert np.array_equal(shared[0][0], each[0][0]) and mismatch(shared[0][1:], each[0][1:])


@pytest.mark.parametrize("cn", [1, 3])
def test_sizes(handle, cn):
    """a 1 x 1 texture; a 1 x 1 frame; a frame 70 wide (a row crosses a tile edge and has a tail of 2) and 19 high (a second tile row)"""
    maps = [eye(), eye(-3, -2), MAGNIFY, eye(-0.4, 0.3), PERSPECTIVE]
    want = check(handle, source(cn), textures(cn, tw=1, th=1), maps)
    assert want[1].tolist() == [1, 1, 0, 0, 0]            # only a position that rounds to the texel's centre is painted
    want = check(handle, source(cn, 1, 1), textures(cn), maps)
    assert want[1].tolist() == [1, 0, 1, 0, 1]
    want = check(handle, source(cn, 70, 19), textures(cn, "ramp"), [MAGNIFY, eye(-33, 0), eye(-62.5, -1), PERSPECTIVE, eye()], opacity=200)
    assert want[1][0] == 70 * 19 and want[1][1] == 36 * 19 and want[1][2] > 0      # columns 34 .. 69: texel column 0 has alpha 0


def test_mixed_residence_gives_the_same_bytes(handle):
    """the texture and the masks on the host with frames and maps on the device, and the reverse, equal the all-host result; so does
    the numpy-level call"""
    import torch

    from aruco_amd import capi

    cn = 3
    src, tex, masks = source(cn), np.ascontiguousarray(textures(cn, "ramp")[0]), checkerboard()
    m = np.ascontiguousarray(np.asarray(BASIC, np.float64).reshape(N, 9))
    want, _ = reference(src, [tex], BASIC, opacity=200, masks=masks)
    dm, dt, dk = torch.from_numpy(m).cuda(), torch.from_numpy(tex).cuda(), torch.from_numpy(masks).cuda()
    a = Frames(src, True)
    handle.composite_plane_device(a.ptr, N, W, H, cn, capi.texture(tex, 200), dm.data_ptr(), masks_ptr=masks.ctypes.data, row_stride=a.row, frame_stride=a.frame,
                                  masks_on_device=0)
    b = Frames(src, False)
    handle.composite_plane_device(b.ptr, N, W, H, cn, capi.texture(dt, 200), m.ctypes.data, masks_ptr=dk.data_ptr(), row_stride=b.row, frame_stride=b.frame,
                                  frames_on_device=0, maps_on_device=0)
    for d in (a, b):
        got, clean = d.split()
        assert not mismatch(got, want) and clean
    before = src.copy()
    assert np.array_equal(handle.composite_plane(src, tex, BASIC, opacity=200, masks=masks), want) and np.array_equal(src, before)


# ---- the board call
def windows():
    from aruco_amd import capi

    # 40 x 30 texels of 2 mm around the board's origin, slightly turned so that all six window entries matter; and one whose rows run
    # along -y (a y-up board): its map has a negative determinant
    return {"turned": capi.Rectify(TW, TH, -0.0412, -0.0287, 0.002, 0.0001, -0.00015, 0.002), "flip_y": capi.Rectify(TW, TH, -0.04, 0.03, 0.002, 0.0, 0.0, -0.002)}


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("which", ["turned", "flip_y"])
def test_board_call(handle, cn, which):
    """status equal to the reference's validity (frame 2 has no pose); maps_out within 1e-12 of the reference's, relative to the map's
    largest entry (an entry of N is a difference of products of two entries of M, each accurate to 1e-12 of M's largest as
    test_gpu_rectify asserts; only sin and cos differ from numpy, by an ulp); the frames byte for byte those of the reference run on the
    returned maps_out."""
    import torch

    from aruco_amd import capi

    win, (_, boards) = windows()[which], board_case()
    dist = DIST8[:5]
    src, tex = source(cn), np.ascontiguousarray(textures(cn, "ramp")[0])
    ref = [cr.board_map(boards[f]["rvec"], boards[f]["tvec"], boards[f]["has_pose"], win) for f in range(N)]
    assert [r[1] for r in ref] == [1, 1, 0, 1, 1]
    assert all((np.linalg.det(r[2].reshape(3, 3)) < 0) == (which == "flip_y") for r in ref if r[1])
    results = []
    for device in (False, True):
        fr = Frames(src, device)
        if device:
            db, dt = torch.from_numpy(boards.view(np.uint8).copy()).cuda(), torch.from_numpy(tex).cuda()
            got_s, got_m = handle.board_composite_device(fr.ptr, N, W, H, cn, db, K_SMALL, win, capi.texture(dt, 230), dist, None, fr.row, fr.frame, report=True)
        else:
            got_s, got_m = handle.board_composite_device(fr.ptr, N, W, H, cn, boards, K_SMALL, win, capi.texture(tex, 230), dist, None, fr.row, fr.frame,
                                                         frames_on_device=0, report=True)
        got, clean = fr.split()
        assert clean
        assert got_s.tolist() == [r[1] for r in ref]
        for f in range(N):
            assert np.max(np.abs(got_m[f] - ref[f][0])) <= 1e-12 * max(np.max(np.abs(ref[f][0])), 1e-300), f
        want, painted = reference(src, [tex], got_m, K_SMALL, dist, valid=got_s, opacity=230)
        assert painted[2] == 0 and all(painted[f] > 200 for f in (0, 1, 3, 4)), painted
        assert not mismatch(got, want), (device, mismatch(got, want))
        results.append((got.tobytes(), got_s.tobytes(), got_m.tobytes()))
    assert results[0] == results[1]            # everything on the host and on the device
    # without the reports: asynchronous, the same frames; and the numpy-level call
    fr = Frames(src, True)
    db, dt = torch.from_numpy(boards.view(np.uint8).copy()).cuda(), torch.from_numpy(tex).cuda()
    assert handle.board_composite_device(fr.ptr, N, W, H, cn, db, K_SMALL, win, capi.texture(dt, 230), dist, None, fr.row, fr.frame) is None
    handle.synchronize()
    assert fr.split()[0].tobytes() == results[1][0]
    out, status, maps = handle.board_composite(src, boards, K_SMALL, win, tex, dist, opacity=230)
    assert (out.tobytes(), status.tobytes(), maps.tobytes()) == results[0]


# ---- the chains
NEW_IDS = [7, 300, 641, 88, 1001, 412]


def boards_of(poses):
    from aruco_amd import capi

    b = np.zeros(len(poses), capi.BOARD_DTYPE)
    for k, p in enumerate(poses):
        b[k] = (p["n_markers"], p["has_pose"], p["rvec"], p["tvec"])
    return b


def test_replace_the_board_all_on_the_device(handle):
    """paint -> render -> detect_batch -> board_detect_batch -> board_composite_device -> detect_batch: the second detection gives the new
    ids, and only those, on all three frames; then detect(frame) after the chain equals a fresh handle's (the frame graph and its
    buffers survive the compositing calls)."""
    import torch

    from aruco_amd import capi

    _, ids, obj = handle.fiducial_board_image(capi.FIDUCIAL_PANEL, rr.RT_GRID, rr.RT_SIDE, rr.RT_DIST, rr.RT_IDS)
    texture, _, new_obj = handle.fiducial_board_image(capi.FIDUCIAL_PANEL, rr.RT_GRID, rr.RT_SIDE, rr.RT_DIST, NEW_IDS)
    assert np.array_equal(obj, new_obj)
    frames = rr.round_trip_frames(obj)
    n = len(frames)
    win = capi.rectify_board_window(obj, capi.BOARD_PIX, rr.RT_MARKER_M, rr.RT_SIDE / rr.RT_MARKER_M, 0.0)
    assert (win.out_width, win.out_height) == texture.shape[::-1] == (238, 154)
    single = [handle.detect(frames[0], K=rr.RT_K, marker_size=rr.RT_MARKER_M) for _ in range(2)]
    dfr, dtex = torch.from_numpy(frames).cuda(), torch.from_numpy(texture).cuda()
    dm = torch.zeros(n * 32 * capi.MARKER_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    dn = torch.zeros(n, dtype=torch.int32, device="cuda")

    def detect_ids():
        handle.detect_batch_device(dfr.data_ptr(), n, rr.RT_W, rr.RT_H, dm.data_ptr(), 32, dn.data_ptr(), K=rr.RT_K, marker_size=rr.RT_MARKER_M)
        handle.synchronize()
        counts, markers = dn.cpu().numpy(), np.frombuffer(dm.cpu().numpy().tobytes(), capi.MARKER_DTYPE).reshape(n, 32)
        return [sorted(markers[f, :counts[f]]["id"].tolist()) for f in range(n)]

    assert detect_ids() == [sorted(rr.RT_IDS)] * n
    poses = handle.board_detect_batch(n, ids, obj, capi.BOARD_PIX, rr.RT_K, None, rr.RT_MARKER_M)
    db = torch.from_numpy(boards_of(poses).view(np.uint8).copy()).cuda()
    assert handle.board_composite_device(dfr.data_ptr(), n, rr.RT_W, rr.RT_H, 1, db, rr.RT_K, win, capi.texture(dtex)) is None
    assert detect_ids() == [sorted(NEW_IDS)] * n
    changed = (dfr.cpu().numpy() != frames).reshape(n, -1).sum(axis=1)
    assert (changed > 10000).all() and (changed < 73725).all()
    # the frame graph: two calls before the chain, one after it, a fresh handle
    after = handle.detect(frames[0], K=rr.RT_K, marker_size=rr.RT_MARKER_M)
    fresh = capi.Handle(640, 480, max_batch=4)
    try:
        first = fresh.detect(frames[0], K=rr.RT_K, marker_size=rr.RT_MARKER_M)
    finally:
        fresh.close()
    assert len(after) == 6 and single[0].tobytes() == single[1].tobytes() == after.tobytes() == first.tobytes()


def test_occlusion_chain_takes_the_masks_from_the_device(handle):
    """detect -> board pose -> ChromaticMask classify -> composite with the masks as the device pointer classify wrote to: the frames equal
    the reference run with those masks read back, and what the occluder covers keeps its pixels."""
    import torch

    from aruco_amd import capi
    from tests.test_chromatic_cpu import scene
    from tests.test_gpu_chromatic import make

    Wc, Hc = 640, 480
    sc = scene(Wc, Hc)
    bc, K = sc["board"], sc["K"]
    frames = np.stack([sc["img"], sc["occ"], sc["occ"]])
    n = len(frames)
    handle.detect_batch_host(frames)
    poses = handle.board_detect_batch(n, bc["ids"], bc["obj"], bc["info_type"], K=K, marker_size=0.039)
    assert all(p["has_pose"] for p in poses)
    dev = make(handle, sc, Wc, Hc)
    try:
        dev.train(sc["img"], poses[0]["rvec"], poses[0]["tvec"])
        dfr = torch.from_numpy(frames).cuda()
        dmask = torch.zeros((n, Hc, Wc), dtype=torch.uint8, device="cuda")
        dev.classify_batch_device(handle, dfr.data_ptr(), n, Wc, Wc * Hc, dmask.data_ptr(), method=2)
        win = capi.rectify_board_window(bc["obj"], bc["info_type"], 0.039, 641.0, 0.0)
        tex = np.random.RandomState(8).randint(0, 256, (win.out_height, win.out_width)).astype(np.uint8)
        dtex = torch.from_numpy(tex).cuda()
        status, maps = handle.board_composite_device(dfr.data_ptr(), n, Wc, Hc, 1, boards_of(poses), K, win, capi.texture(dtex, 255), None, dmask.data_ptr(),
                                                     report=True)
    finally:
        dev.close()
    masks = dmask.cpu().numpy()
    assert status.tolist() == [1] * n and masks[0].sum() > 20000
    want, painted = reference(frames, [tex], maps, K, None, masks=masks)
    got = dfr.cpu().numpy()
    assert not mismatch(got, want)
    free, _ = reference(frames, [tex], maps, K, None)
    hidden = sc["occ_in"]        # ChromaticMask's own tests ask for 99 % of these pixels to be classified as covered
    assert painted[1] < painted[0] and (got[1][hidden] == frames[1][hidden]).mean() >= 0.99 and (free[1][hidden] != frames[1][hidden]).mean() > 0.9


def test_invalid_arguments_are_named_and_touch_nothing(handle):
    from aruco_amd import capi

    L = handle.L
    frames = np.full((2, H, W * 3), SENT, np.uint8)
    maps = np.tile(np.eye(3).reshape(9), (2, 1))
    tex = np.zeros((2, TH, TW * 4), np.uint8)
    masks = np.ones((2, H, W), np.uint8)
    _, boards = board_case()
    boards = boards[:2].copy()
    fp, mp, tp, bp, kp = frames.ctypes.data, maps.ctypes.data, tex.ctypes.data, boards.ctypes.data, masks.ctypes.data
    Kp = K_SMALL.ctypes.data
    d5 = DIST8[:5].copy()

    def texture(**kw):
        a = dict(data=tp, width=TW, height=TH, channels=3, on_device=0, row_stride=TW * 4, frame_stride=0, opacity=255)
        a.update(kw)
        return capi.Texture(a["data"], a["width"], a["height"], a["channels"], a["on_device"], a["row_stride"], a["frame_stride"], a["opacity"], 0)

    def plane(**kw):
        a = dict(frames=fp, n=2, w=W, h=H, ch=3, rs=W * 3, fs=W * 3 * H, tex=texture(), maps=mp, K=None, dist=None, nd=0, masks=None)
        a.update(kw)
        t = a["tex"]
        return L.arucohip_composite_plane_batch(handle.h, a["frames"], a["n"], a["w"], a["h"], a["ch"], a["rs"], a["fs"], 0, None if t is None else ctypes.byref(t),
                                                a["maps"], None, 0, a["K"], a["dist"], a["nd"], a["masks"], 0)

    def window(**kw):
        w = capi.Rectify(TW, TH, 0.0, 0.0, 0.002, 0.0, 0.0, 0.002)
        for k, v in kw.items():
            setattr(w, k, v)
        return w

    def board(**kw):
        a = dict(frames=fp, n=2, ch=3, rs=W * 3, boards=bp, K=Kp, dist=None, nd=0, win=window(), tex=texture(), masks=None)
        a.update(kw)
        w, t = a["win"], a["tex"]
        return L.arucohip_board_composite_batch(handle.h, a["frames"], a["n"], W, H, a["ch"], a["rs"], W * 3 * H, 0, a["boards"], 0, a["K"], a["dist"], a["nd"],
                                                None if w is None else ctypes.byref(w), None if t is None else ctypes.byref(t), a["masks"], 0, None, None)

    cases = [(plane, dict(frames=None), "frames"), (plane, dict(tex=None), "tex"), (plane, dict(tex=texture(data=None)), "tex->data"),
             (plane, dict(maps=None), "maps"), (plane, dict(ch=2), "channels"), (plane, dict(ch=4), "channels"),
             (plane, dict(tex=texture(channels=2)), "tex->channels"), (plane, dict(tex=texture(channels=5)), "tex->channels"),
             (plane, dict(tex=texture(opacity=-1)), "opacity"), (plane, dict(tex=texture(opacity=256)), "opacity"),
             (plane, dict(w=0), "width"), (plane, dict(h=0), "height"), (plane, dict(w=16384, rs=16384 * 3, fs=16384 * 3 * H), "16383"),
             (plane, dict(tex=texture(width=0)), "tex->width"), (plane, dict(tex=texture(height=0)), "tex->height"),
             (plane, dict(tex=texture(width=16384, row_stride=16384 * 4)), "16383"),
             (plane, dict(rs=W * 3 - 1), "row_stride"), (plane, dict(fs=W * 3 * H - 1), "frame_stride"),
             (plane, dict(tex=texture(row_stride=TW * 3 - 1)), "tex->row_stride"), (plane, dict(tex=texture(frame_stride=TW * 4 * (TH - 1))), "tex->frame_stride"),
             (plane, dict(K=Kp, dist=d5.ctypes.data, nd=3), "ndist"), (plane, dict(K=Kp, nd=5), "dist"), (plane, dict(dist=d5.ctypes.data, nd=5), "K"),
             (plane, dict(n=0), "nframes"), (plane, dict(tex=texture(data=fp + 100)), "overlaps"), (plane, dict(masks=fp + W * 3 * H), "overlaps"),
             (board, dict(frames=None), "frames"), (board, dict(boards=None), "boards"), (board, dict(win=None), "win"), (board, dict(tex=None), "tex"),
             (board, dict(K=None), "K"), (board, dict(ch=2), "channels"), (board, dict(nd=6, dist=d5.ctypes.data), "ndist"), (board, dict(rs=10), "row_stride"),
             (board, dict(n=0), "nframes"), (board, dict(tex=texture(opacity=300)), "opacity"), (board, dict(win=window(out_width=TW + 1)), "differ"),
             (board, dict(win=window(out_height=TH - 1)), "differ"), (board, dict(win=window(ux=0.0)), "parallel"),
             (board, dict(win=window(vx=0.002, vy=0.0)), "parallel"), (board, dict(win=window(uy=0.001, vx=0.004, vy=0.002)), "parallel"),
             (board, dict(win=window(x0=float("nan"))), "finite"), (board, dict(masks=fp + 7), "overlaps")]
    assert L.arucohip_composite_plane_batch(None, fp, 2, W, H, 3, W * 3, W * 3 * H, 0, ctypes.byref(texture()), mp, None, 0, None, None, 0, None, 0) == capi.E_INVALID
    for fn, kw, word in cases:
        assert fn(**kw) == capi.E_INVALID, kw
        msg = (L.arucohip_last_error_string(handle.h) or b"").decode()
        assert word in msg, (kw, msg)
        assert (frames == SENT).all(), kw
    assert plane(masks=kp) == capi.OK and (frames[:, :TH, :TW * 3] == 0).all()
    frames[:] = SENT
    assert board(tex=texture(channels=4, frame_stride=TW * 4 * TH)) == capi.OK and (frames == SENT).all()      # alpha 0: valid, and nothing painted
