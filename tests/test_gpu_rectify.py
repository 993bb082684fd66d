"""Plane rectification on the device against tests/rectify_ref.py. Caller maps: bytes, no tolerance (the projection is the same IEEE
double arithmetic on both sides). Board call: the maps differ from numpy's in sin and cos only, so the images are compared except where
the reference's position lies within 1e-6 of a rounding tie. Small shapes: 96 x 64 sources, 70 x 50 outputs, 5 frames with 5 maps."""
import ctypes

import numpy as np
import pytest

from tests import rectify_ref as rr

pytestmark = pytest.mark.gpu

W, H, OW, OH, N = 96, 64, 70, 50, 5
SENT = 0xA5
K_SMALL = np.array([[85.5, 0, 47.25], [0, 84.25, 31.5], [0, 0, 1]], np.float32)
DIST8 = np.array([0.08, -0.12, 0.0011, -0.0017, 0.03, 0.02, -0.015, 0.004], np.float32)


def eye(tx=0.0, ty=0.0):
    return np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], np.float64)


# W changes sign inside the 70 x 50 output: 1 - u / 40 - v / 90 is 0 along a line from (40, 0) to (17.8, 50)
PERSPECTIVE = np.array([[0.9, 0.1, 4.0], [-0.05, 1.1, 1.5], [-1 / 40.0, -1 / 90.0, 1.0]])
BASIC = [eye(), eye(-3, 2), eye(-0.5, 0), eye(1 / 64, 3 / 64), PERSPECTIVE]
ROTATED = np.array([[0.8, -0.6, 20.25], [0.6, 0.8, -11.5], [0.0003, 0.0002, 1.0]])
nan_map, inf_map = eye(), eye()
nan_map[1, 1], inf_map[0, 2] = np.nan, np.inf
DEGENERATE = [np.array([[1e12, 0, 1e12], [0, 1e12, 1e12], [0, 0, 1.0]]), nan_map, inf_map, ROTATED, eye(30.5, 40.25)]
# for a camera: output pixel -> a point in front of it, about +-0.4 across
POSE_LIKE = [np.array([[1 / 90.0, 0.0007 * k, -0.41 + 0.02 * k], [-0.0004, 1 / 88.0, -0.27 - 0.01 * k], [0.0006 * k, -0.0009, 1.0 + 0.05 * k]]) for k in range(N)]


@pytest.fixture(scope="module")
def handle():
    from aruco_amd import capi

    h = capi.Handle(640, 480, max_batch=4)
    yield h
    h.close()


_SOURCES = {}


def source(cn):
    """[N][H][row_stride] with a padded row_stride; the image part is a fixed texture"""
    if cn not in _SOURCES:
        rng = np.random.RandomState(11 + cn)
        buf = np.full((N, H, W * cn + 5), 0x5A, np.uint8)
        buf[:, :, :W * cn] = rng.randint(0, 256, (N, H, W * cn))
        _SOURCES[cn] = buf
    return _SOURCES[cn]


def images(buf, cn):
    v = buf[:, :, :W * cn]
    return v if cn == 1 else v.reshape(N, H, W, 3)


def reference(cn, maps, K=None, dist=None, valid=None, ow=OW, oh=OH):
    src = images(source(cn), cn)
    return np.stack([rr.warp_plane(src[f], maps[f], ow, oh, K, dist, True if valid is None else bool(valid[f])) for f in range(len(maps))])


class Dst:
    """The destination of a call: rows of (ow + 3) * cn bytes, images a row and 11 bytes apart, starting at an odd address, 0xA5 all over."""

    def __init__(self, n, ow, oh, cn, device):
        self.n, self.ow, self.oh, self.cn, self.device = n, ow, oh, cn, device
        self.row, self.frame = (ow + 3) * cn, (ow + 3) * cn * (oh + 1) + 11
        size = 1 + n * self.frame + 16
        if device:
            import torch

            self.buf = torch.full((size,), SENT, dtype=torch.uint8, device="cuda")
            self.ptr = self.buf.data_ptr() + 1
        else:
            self.buf = np.full(size, SENT, np.uint8)
            self.ptr = self.buf.ctypes.data + 1
        assert self.ptr % 2 == 1

    def host(self):
        if self.device:
            import torch

            torch.cuda.synchronize()
            return self.buf.cpu().numpy()
        return self.buf

    def split(self):
        """(the images [n][oh][ow](x cn), whether every other byte still holds the sentinel)"""
        b = self.host().copy()
        out = np.zeros((self.n, self.oh, self.ow * self.cn), np.uint8)
        for f in range(self.n):
            for y in range(self.oh):
                at = 1 + f * self.frame + y * self.row
                out[f, y] = b[at:at + self.ow * self.cn]
                b[at:at + self.ow * self.cn] = SENT
        return (out if self.cn == 1 else out.reshape(self.n, self.oh, self.ow, 3)), bool((b == SENT).all())


def run(handle, cn, maps, K=None, dist=None, valid=None, ow=OW, oh=OH, device=False):
    """arucohip_warp_plane_batch with everything on the host or everything on the device"""
    src = source(cn)
    m = np.ascontiguousarray(np.asarray(maps, np.float64).reshape(len(maps), 9))
    v = None if valid is None else np.ascontiguousarray(valid, np.int32)
    dst = Dst(len(maps), ow, oh, cn, device)
    if device:
        import torch

        ds, dm = torch.from_numpy(src).cuda(), torch.from_numpy(m).cuda()
        dv = None if v is None else torch.from_numpy(v).cuda()
        handle.warp_plane_device(ds.data_ptr(), len(maps), W, H, cn, dm.data_ptr(), dst.ptr, ow, oh, K, dist, None if dv is None else dv.data_ptr(),
                                 src.shape[2], src.shape[2] * H, dst.row, dst.frame)
        handle.synchronize()
    else:
        handle.warp_plane_device(src.ctypes.data, len(maps), W, H, cn, m.ctypes.data, dst.ptr, ow, oh, K, dist, None if v is None else v.ctypes.data,
                                 src.shape[2], src.shape[2] * H, dst.row, dst.frame, src_on_device=0, maps_on_device=0, dst_on_device=0)
    return dst.split()


def mismatch(got, want):
    bad = np.argwhere(got != want)
    return "%d bytes differ, first at %s: %s != %s" % (len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]) if len(bad) else ""


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("name,maps", [("basic", BASIC), ("degenerate", DEGENERATE)])
def test_caller_maps_equal_the_reference(handle, cn, name, maps):
    want = reference(cn, maps)
    if name == "basic":
        assert np.array_equal(want[0], images(source(cn), cn)[0, :OH, :OW])   # identity
        assert not want[1][:, :3].any() and want[1][:, 3:].any()             # the shift reads 3 columns left of the source: 0
        assert not want[4][:, 45:].any() and want[4][:, :10].any()           # behind the line where W changes sign: 0
    else:
        assert not want[0].any() and not want[1].any() and not want[2].any() and want[3].any()   # saturated, NaN, Inf: all 0
    for device in (False, True):
        got, clean = run(handle, cn, maps, device=device)
        assert not mismatch(got, want), (device, mismatch(got, want))
        assert clean, "bytes outside the images were written"


@pytest.mark.parametrize("cn", [1, 3])
def test_valid_flags(handle, cn):
    valid = [1, 0, 1, 1, 0]
    want = reference(cn, BASIC, valid=valid)
    assert not want[1].any() and not want[4].any() and want[0].any()
    for device in (False, True):
        got, clean = run(handle, cn, BASIC, valid=valid, device=device)
        assert not mismatch(got, want) and clean, (device, mismatch(got, want))


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("ndist", [0, 4, 5, 8])
def test_camera_and_distortion(handle, cn, ndist):
    dist = DIST8[:ndist] if ndist else None
    want = reference(cn, POSE_LIKE, K_SMALL, dist)
    assert (want != 0).mean() > 0.5
    if ndist == 8:
        assert mismatch(want, reference(cn, POSE_LIKE, K_SMALL, DIST8[:5]))   # the rational terms change the image
    got, clean = run(handle, cn, POSE_LIKE, K_SMALL, dist, device=ndist != 4)
    assert not mismatch(got, want) and clean, mismatch(got, want)


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("ow,oh", [(7, 3), (1, 1), (260, 9)])
def test_output_sizes(handle, cn, ow, oh):
    """a tail of less than one lane's four pixels, one pixel, and an output wider than a workgroup's 64-pixel tile (with a tail of 4)"""
    maps = [eye(), eye(-3, 2), PERSPECTIVE, ROTATED, np.array([[0.3, 0, 0.25], [0, 2.0, 0.5], [0, 0, 1.0]])]
    want = reference(cn, maps, ow=ow, oh=oh)
    assert want.any()
    for device in (False, True):
        got, clean = run(handle, cn, maps, ow=ow, oh=oh, device=device)
        assert not mismatch(got, want) and clean, (device, mismatch(got, want))


def test_mixed_residence_gives_the_same_bytes(handle):
    """maps on the host with frames and dst on the device, and the reverse, equal the all-host result"""
    import torch

    cn = 3
    src = source(cn)
    m = np.ascontiguousarray(np.asarray(BASIC, np.float64).reshape(N, 9))
    want = reference(cn, BASIC)
    ds, dm = torch.from_numpy(src).cuda(), torch.from_numpy(m).cuda()
    a = Dst(N, OW, OH, cn, True)
    handle.warp_plane_device(ds.data_ptr(), N, W, H, cn, m.ctypes.data, a.ptr, OW, OH, None, None, None, src.shape[2], src.shape[2] * H, a.row, a.frame,
                             maps_on_device=0)
    b = Dst(N, OW, OH, cn, False)
    handle.warp_plane_device(src.ctypes.data, N, W, H, cn, dm.data_ptr(), b.ptr, OW, OH, None, None, None, src.shape[2], src.shape[2] * H, b.row, b.frame,
                             src_on_device=0, dst_on_device=0)
    for d in (a, b):
        got, clean = d.split()
        assert not mismatch(got, want) and clean
    # the numpy-level call
    assert np.array_equal(handle.warp_plane(images(src, cn).copy(), BASIC, (OW, OH)), want)


# ---- the board call
def board_case():
    from aruco_amd import capi

    # the window: 70 x 50 pixels of 2 mm around the board's origin, slightly turned so that all six window entries matter
    win = capi.Rectify(OW, OH, -0.0712, -0.0487, 0.002, 0.0001, -0.00015, 0.002)
    boards = np.zeros(N, capi.BOARD_DTYPE)
    poses = [((0.0, 0.0, 0.0), (0.003, -0.002, 0.2)),                       # frontal
             ((np.pi / 3, 0.0, 0.0), (0.0, 0.004, 0.25)),                   # tilted by 60 degrees about x
             ((0.3, -0.2, 0.1), (0.01, 0.0, 0.22)),                         # no pose: has_pose = 0
             ((0.1, 0.5, -1.2), (0.12, -0.05, 0.24)),                       # part of the window leaves the frame
             ((-0.4, 0.35, 2.0), (-0.01, 0.01, 0.3))]
    for f, (r, t) in enumerate(poses):
        boards[f] = (4, 0 if f == 2 else 1, r, t)
    return win, boards


def board_reference(cn, win, boards, K, dist):
    src = images(source(cn), cn)
    out, status, maps, near = [], [], [], []
    for f in range(N):
        M, ok = rr.plane_map(boards[f]["rvec"], boards[f]["tvec"], boards[f]["has_pose"], win)
        maps.append(M), status.append(ok)
        out.append(rr.warp_plane(src[f], M, OW, OH, K, dist, ok))
        qx, qy, _ = rr.positions(M, OW, OH, K, dist)
        with np.errstate(all="ignore"):
            tie = (np.abs(qx - np.floor(qx) - 0.5) < 1e-6) | (np.abs(qy - np.floor(qy) - 0.5) < 1e-6)
        near.append(tie & bool(ok))
    return np.stack(out), np.array(status, np.int32), np.stack(maps), np.stack(near)


@pytest.mark.parametrize("cn", [1, 3])
def test_board_call(handle, cn):
    """status equal; maps_out within 1e-12 of the reference's, relative to the map's largest entry (an entry is a sum of products of R
    and the window, accurate to the size of its terms; only sin and cos differ from numpy, by an ulp); images equal except where the
    reference's px * 32 or py * 32 lies within 1e-6 of a half-integer, at most 0.1 % of an image's pixels (expected: 0.01 of a pixel)."""
    import torch

    win, boards = board_case()
    dist = DIST8[:5]
    want, status, maps, near = board_reference(cn, win, boards, K_SMALL, dist)
    assert status.tolist() == [1, 1, 0, 1, 1]
    assert near.reshape(N, -1).sum(axis=1).max() <= 0.001 * OW * OH
    assert not want[2].any() and all(want[f].any() for f in (0, 1, 3, 4))
    assert not want[3][:, -8:].any()           # the part outside the frame
    src = source(cn)
    results = []
    for device in (False, True):
        dst = Dst(N, OW, OH, cn, device)
        if device:
            ds = torch.from_numpy(src).cuda()
            db = torch.from_numpy(boards.view(np.uint8).copy()).cuda()
            got_s, got_m = handle.board_rectify_device(ds.data_ptr(), N, W, H, cn, db, K_SMALL, win, dst.ptr, dist, src.shape[2], src.shape[2] * H,
                                                       dst.row, dst.frame, report=True)
        else:
            got_s, got_m = handle.board_rectify_device(src.ctypes.data, N, W, H, cn, boards, K_SMALL, win, dst.ptr, dist, src.shape[2], src.shape[2] * H,
                                                       dst.row, dst.frame, frames_on_device=0, dst_on_device=0, report=True)
        got, clean = dst.split()
        assert clean
        assert got_s.tolist() == status.tolist()
        for f in range(N):
            assert np.max(np.abs(got_m[f] - maps[f])) <= 1e-12 * max(np.max(np.abs(maps[f])), 1e-300), f
        diff = (got != want) if cn == 1 else (got != want).any(axis=3)
        assert not (diff & ~near).any(), mismatch(got, want)
        results.append((got.tobytes(), got_s.tobytes(), got_m.tobytes()))
    assert results[0] == results[1]            # boards on the host and on the device
    # without the reports: asynchronous, the same image
    dst = Dst(N, OW, OH, cn, True)
    ds = torch.from_numpy(src).cuda()
    db = torch.from_numpy(boards.view(np.uint8).copy()).cuda()
    assert handle.board_rectify_device(ds.data_ptr(), N, W, H, cn, db, K_SMALL, win, dst.ptr, dist, src.shape[2], src.shape[2] * H, dst.row, dst.frame) is None
    handle.synchronize()
    assert dst.split()[0].tobytes() == results[1][0]


# ---- the round trip, and what must still hold after it
@pytest.fixture(scope="module")
def chain(handle):
    """paint -> render -> detect_batch -> board_detect_batch -> board_rectify, with the frames and dst on the device and through host buffers"""
    import torch

    from aruco_amd import capi

    board, ids, obj = handle.fiducial_board_image(capi.FIDUCIAL_PANEL, rr.RT_GRID, rr.RT_SIDE, rr.RT_DIST, rr.RT_IDS)
    frames = rr.round_trip_frames(obj)
    n = len(frames)
    win = capi.rectify_board_window(obj, capi.BOARD_PIX, rr.RT_MARKER_M, rr.RT_SIDE / rr.RT_MARKER_M, 0.0)
    single = [handle.detect(frames[0], K=rr.RT_K, marker_size=rr.RT_MARKER_M) for _ in range(3)]   # the third call replays the frame graph

    def boards_of(poses):
        b = np.zeros(n, capi.BOARD_DTYPE)
        for k, p in enumerate(poses):
            b[k] = (p["n_markers"], p["has_pose"], p["rvec"], p["tvec"])
        return b

    # on the device
    dfr = torch.from_numpy(frames).cuda()
    dm = torch.zeros(n * 32 * capi.MARKER_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    dn = torch.zeros(n, dtype=torch.int32, device="cuda")
    handle.detect_batch_device(dfr.data_ptr(), n, rr.RT_W, rr.RT_H, dm.data_ptr(), 32, dn.data_ptr(), K=rr.RT_K, marker_size=rr.RT_MARKER_M)
    poses_dev = handle.board_detect_batch(n, ids, obj, capi.BOARD_PIX, rr.RT_K, None, rr.RT_MARKER_M)
    ddst = torch.full((n, win.out_height, win.out_width), SENT, dtype=torch.uint8, device="cuda")
    status_dev, _ = handle.board_rectify_device(dfr.data_ptr(), n, rr.RT_W, rr.RT_H, 1, boards_of(poses_dev), rr.RT_K, win, ddst.data_ptr(), report=True)
    on_device = ddst.cpu().numpy()
    # through host buffers
    handle.detect_batch_host(frames, K=rr.RT_K, marker_size=rr.RT_MARKER_M, cap=32)
    poses_host = handle.board_detect_batch(n, ids, obj, capi.BOARD_PIX, rr.RT_K, None, rr.RT_MARKER_M)
    on_host, status_host, _ = handle.board_rectify(frames, poses_host, rr.RT_K, win)
    after = handle.detect(frames[0], K=rr.RT_K, marker_size=rr.RT_MARKER_M)
    return dict(board=board, win=win, on_device=on_device, on_host=on_host, status=(status_dev, status_host), single=single, after=after, n=n)


def test_round_trip_reads_the_painted_board(chain):
    assert (chain["win"].out_width, chain["win"].out_height) == (238, 154) and chain["board"].shape == (154, 238)
    assert chain["status"][0].tolist() == [1] * chain["n"] and chain["status"][1].tolist() == [1] * chain["n"]
    for f in range(chain["n"]):
        assert rr.round_trip_mismatches(chain["board"], chain["on_device"][f]) == [], f
    assert chain["on_device"].tobytes() == chain["on_host"].tobytes()


def test_frame_graph_survives_the_chain(chain):
    assert len(chain["single"][0]) == 6
    assert chain["single"][0].tobytes() == chain["single"][2].tobytes() == chain["after"].tobytes()


def test_invalid_arguments_are_named_and_touch_nothing(handle):
    from aruco_amd import capi

    L = handle.L
    src = np.zeros((2, H, W * 3), np.uint8)
    maps = np.tile(np.eye(3).reshape(9), (2, 1))
    dst = np.full((2, OH, OW * 3), SENT, np.uint8)
    win, boards = board_case()
    boards = boards[:2].copy()
    sp, mp, dp, bp = src.ctypes.data, maps.ctypes.data, dst.ctypes.data, boards.ctypes.data
    Kp = K_SMALL.ctypes.data
    d5 = DIST8[:5].copy()

    def warp(**kw):
        a = dict(src=sp, n=2, w=W, h=H, ch=3, rs=W * 3, fs=W * 3 * H, maps=mp, K=None, dist=None, nd=0, dst=dp, ow=OW, oh=OH, drs=OW * 3, dfs=OW * 3 * OH)
        a.update(kw)
        return L.arucohip_warp_plane_batch(handle.h, a["src"], a["n"], a["w"], a["h"], a["ch"], a["rs"], a["fs"], 0, a["maps"], None, 0, a["K"], a["dist"],
                                           a["nd"], a["dst"], a["ow"], a["oh"], a["drs"], a["dfs"], 0)

    def rect(**kw):
        a = dict(src=sp, n=2, ch=3, rs=W * 3, boards=bp, K=Kp, dist=None, nd=0, win=win, dst=dp, drs=OW * 3)
        a.update(kw)
        w = a["win"]
        return L.arucohip_board_rectify_batch(handle.h, a["src"], a["n"], W, H, a["ch"], a["rs"], W * 3 * H, 0, a["boards"], 0, a["K"], a["dist"], a["nd"],
                                              None if w is None else ctypes.byref(w), a["dst"], a["drs"], a["drs"] * OH, 0, None, None)

    def window(**kw):
        w = capi.Rectify(OW, OH, 0.0, 0.0, 0.002, 0.0, 0.0, 0.002)
        for k, v in kw.items():
            setattr(w, k, v)
        return w

    cases = [(warp, dict(src=None), "src"), (warp, dict(maps=None), "maps"), (warp, dict(dst=None), "dst"), (warp, dict(ch=2), "channels"),
             (warp, dict(ch=4), "channels"), (warp, dict(K=Kp, dist=d5.ctypes.data, nd=3), "ndist"), (warp, dict(K=Kp, nd=5), "dist"),
             (warp, dict(dist=d5.ctypes.data, nd=5), "K"), (warp, dict(rs=W * 3 - 1), "row_stride"), (warp, dict(fs=W * 3 * H - 1), "frame_stride"),
             (warp, dict(drs=OW * 3 - 1), "dst_row_stride"), (warp, dict(dfs=OW * 3 * OH - 1), "dst_frame_stride"), (warp, dict(ow=0), "out_width"),
             (warp, dict(oh=0), "out_height"), (warp, dict(ow=16384, drs=16384 * 3, dfs=16384 * 3 * OH), "16383"), (warp, dict(n=0), "nframes"),
             (warp, dict(w=0), "width"), (warp, dict(dst=sp + 100), "overlaps"),
             (rect, dict(src=None), "src"), (rect, dict(boards=None), "boards"), (rect, dict(win=None), "win"), (rect, dict(K=None), "K"),
             (rect, dict(dst=None), "dst"), (rect, dict(ch=2), "channels"), (rect, dict(nd=6, dist=d5.ctypes.data), "ndist"),
             (rect, dict(rs=10), "row_stride"), (rect, dict(drs=10), "dst_row_stride"), (rect, dict(n=0), "nframes"),
             (rect, dict(win=window(out_width=0)), "out_width"), (rect, dict(win=window(out_height=20000)), "16383"),
             (rect, dict(win=window(ux=0.0)), "parallel"), (rect, dict(win=window(vx=0.002, vy=0.0)), "parallel"),
             (rect, dict(win=window(ux=0.0, vy=0.0)), "parallel"), (rect, dict(win=window(uy=0.001, vx=0.004, vy=0.002)), "parallel")]
    for fn, kw, word in cases:
        assert fn(**kw) == capi.E_INVALID, kw
        msg = (L.arucohip_last_error_string(handle.h) or b"").decode()
        assert word in msg, (kw, msg)
        assert (dst == SENT).all(), kw
    assert warp() == capi.OK and rect() == capi.OK and (dst != SENT).any()
