"""Chessboard-corner (ChArUco) boards on the device: the painter against charuco_ref's image, the interpolated corners of rendered frames
against charuco_ref (start, markers, window) and pixref (the SUBPIX refinement, at the bound test_gpu_pix_edges.py holds refine_pixels_kernel
to), the edge cases of the interpolation, the argument errors, and the two consumers of the resident corners: calibration (bit for bit
arucohip_calibrate_camera on the same corners, and calib_ref's scipy solve) and pose (pose_ref's polished minimum)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import calib_ref
from tests import charuco_ref as cr
from tests import pixref
from tests import pose_ref

pytestmark = pytest.mark.gpu
KF = cr.K.astype(np.float32)
SQUARE_M = cr.UNIT * cr.LAYOUT[2]    # the side of a square in metres, as the renderer draws it


@pytest.fixture(scope="module")
def capi():
    import torch  # noqa: F401  (torch's HIP runtime first, see aruco_amd/capi.py)
    from aruco_amd import capi as c

    return c


def chunked_handle(capi, max_batch, workers):
    """a handle whose batches of max_batch frames run as `workers` chunks, each on its own worker (ARUCOHIP_STREAMS is read at creation)"""
    old = os.environ.get("ARUCOHIP_STREAMS")
    os.environ["ARUCOHIP_STREAMS"] = str(workers)
    try:
        return capi.Handle(cr.W, cr.H, max_batch=max_batch)
    finally:
        if old is None:
            del os.environ["ARUCOHIP_STREAMS"]
        else:
            os.environ["ARUCOHIP_STREAMS"] = old


def lay(capi, L):
    return capi.charuco_layout(L[:2], L[2], L[3])


def marker_list(m):
    """a frame's detections as charuco_ref.interpolate takes them; None for a frame the batch gave up"""
    return None if m is None else [(int(x["id"]), np.asarray(x["corners"], np.float32).reshape(4, 2)) for x in m]


def check_frame(frame, rec, markers, L=cr.LAYOUT, ids=cr.IDS, min_markers=2, max_win=5):
    """One frame's records against the reference computed from the marker list the detect call returned. Returns the reference records."""
    H, W = frame.shape
    ref = cr.interpolate(L, ids, markers, W, H, min_markers, max_win)
    assert len(rec) == len(ref)
    worst = 0.0
    for c, (g, r) in enumerate(zip(rec, ref)):
        assert g["markers"] == r["markers"] and g["pad_"] == 0, (c, g, r)
        if r["markers"]:
            for got, want in ((g["start_x"], r["start"][0]), (g["start_y"], r["start"][1])):
                assert abs(float(got) - want) <= 4.0 * float(np.spacing(np.float32(max(abs(want), 1.0)))), (c, got, want)
        else:
            assert g["start_x"] == 0 and g["start_y"] == 0
        if r["fragile"]:   # a decision within 1e-4 of its threshold: the neighbouring window, and what follows from it, is as good
            assert abs(int(g["win"]) - r["win"]) <= 1, (c, g, r)
        else:
            assert (bool(g["found"]), int(g["win"])) == (r["found"], r["win"]), (c, g, r)
        start = np.array([g["start_x"], g["start_y"]], np.float32)
        got = np.array([g["x"], g["y"]], np.float32)
        if not g["found"]:
            assert np.array_equal(got, start), (c, g)
            continue
        # the refinement, judged from the device's own start and window: the arithmetic is refine_pixels_kernel's, and so is the bound
        pr = pixref.reference_on(frame, "subpix", start, int(g["win"]))
        rr = pr["record"]["refine"]
        ok, dev, bound = pixref.judge_against(pr, "subpix", got, exactly=rr["exit"] == "det" or rr["reset"])
        worst = max(worst, dev)
        assert ok, (c, g, pr["exact"], dev, bound, pr["fragile"])
    print("worst refined deviation from pixref %.3g px" % worst)
    return ref


@pytest.fixture(scope="module")
def batch(capi):
    """The batch of six frames on a handle with two chunk workers, three frames each. The handle stays open with the corners resident."""
    frames = np.stack([cr.frame(n)[0] for n in cr.BATCH])
    h = chunked_handle(capi, 6, 2)
    markers = h.detect_batch_host(frames, K=KF, marker_size=SQUARE_M * 0.7)
    assert h.batch_chunks()[0] == 2
    rec, nf = h.charuco_corners_batch(lay(capi, cr.LAYOUT), cr.IDS, frames)
    yield {"h": h, "frames": frames, "markers": [marker_list(m) for m in markers], "rec": rec, "nf": nf}
    h.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# painter
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [cr.LAYOUT, (3, 2, 23, 9), (4, 5, 37, 30), (2, 2, 9, 7)])
def test_painter_is_byte_identical_to_the_reference(capi, L):
    import torch

    ids = list(range(11, 11 + cr.board_size(L)[2]))
    want = cr.board_image(L, ids)
    h = capi.Handle(64, 64)
    try:
        for centered in (False, True):
            img, obj, cobj = h.charuco_board_image(lay(capi, L), ids, centered=centered)
            wobj, wcobj = cr.objects(L, centered)
            assert np.array_equal(img, want) and np.array_equal(obj, wobj) and np.array_equal(cobj, wcobj)
        # a device destination whose rows are 13 bytes longer than the image and start at an odd address
        Hh, Ww = want.shape
        stride = Ww + 13
        dev = torch.full((Hh * stride + 3,), 77, dtype=torch.uint8, device="cuda")
        a = np.ascontiguousarray(ids, np.int32)
        h._chk(h.L.arucohip_charuco_board_image(h.h, C.byref(lay(capi, L)), 0, a.ctypes.data_as(C.c_void_p), a.size, C.c_void_p(dev.data_ptr() + 3),
                                                stride, 1, None, None))
        got = dev.cpu().numpy()
        rows = got[3:].reshape(Hh, stride)
        assert np.array_equal(rows[:, :Ww], want) and np.all(rows[:, Ww:] == 77) and np.all(got[:3] == 77)
        # a host destination with padded rows
        host = np.full((Hh, stride), 55, np.uint8)
        h._chk(h.L.arucohip_charuco_board_image(h.h, C.byref(lay(capi, L)), 0, a.ctypes.data_as(C.c_void_p), a.size, host.ctypes.data_as(C.c_void_p),
                                                stride, 0, None, None))
        assert np.array_equal(host[:, :Ww], want) and np.all(host[:, Ww:] == 55)
    finally:
        h.close()


def test_painted_board_is_detected_and_is_a_board(capi):
    h = capi.Handle(cr.W, cr.H)
    try:
        img, obj, _ = h.charuco_board_image(lay(capi, cr.LAYOUT), cr.IDS, centered=True)
        frame = np.full((cr.H, cr.W), 255, np.uint8)
        frame[40:440, 70:570] = img
        m = h.detect(frame, K=KF, marker_size=0.07)
        assert [int(x["id"]) for x in m] == cr.IDS
        # obj with ids is a board for the existing board calls
        b = h.board_detect(m, cr.IDS, obj, capi.BOARD_PIX, K=KF, marker_size=0.07)
        assert b["has_pose"] == 1 and len(b["markers"]) == 10
    finally:
        h.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# corners
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", range(len(cr.BATCH)))
def test_corners_of_the_batch(batch, f):
    name = cr.BATCH[f]
    ref = check_frame(batch["frames"][f], batch["rec"][f], batch["markers"][f])
    assert batch["nf"][f] == int(batch["rec"][f]["found"].sum())
    found = sum(r["found"] for r in ref)
    if name in ("frontal", "tilted", "turned"):
        assert found == 12 and batch["nf"][f] == 12
        truth = cr.frame(name)[1]
        got = np.stack([batch["rec"][f]["x"], batch["rec"][f]["y"]], axis=1).astype(np.float64)
        assert np.max(np.linalg.norm(got - truth, axis=1)) < 0.5      # the right corners, each at its number
    if name == "covered":
        near = [c for c in range(12) if cr.COVERED in [k for k, _ in cr.neighbours(cr.LAYOUT, c)]]
        assert len(near) == 4 and all(batch["rec"][f][c]["markers"] == 1 and not batch["rec"][f][c]["found"] for c in near) and batch["nf"][f] == 8
    if name == "outside":
        assert 0 < batch["nf"][f] < 12
    if name == "empty":
        assert batch["markers"][f] == [] and batch["nf"][f] == 0 and not batch["rec"][f]["found"].any() and not batch["rec"][f]["markers"].any()


def test_min_markers_one_takes_a_single_neighbour_and_the_frame_border_rejects(batch, capi):
    h, frames = batch["h"], batch["frames"]
    opt = capi.default_charuco()
    assert (opt.min_markers, opt.max_win) == (2, 5)
    opt.min_markers = 1
    rec, nf = h.charuco_corners_batch(lay(capi, cr.LAYOUT), cr.IDS, frames, opt=opt)
    try:
        f = cr.BATCH.index("covered")
        check_frame(frames[f], rec[f], batch["markers"][f], min_markers=1)
        near = [c for c in range(12) if cr.COVERED in [k for k, _ in cr.neighbours(cr.LAYOUT, c)]]
        assert all(rec[f][c]["markers"] == 1 and rec[f][c]["found"] for c in near) and nf[f] == 12
        f = cr.BATCH.index("outside")
        ref = check_frame(frames[f], rec[f], batch["markers"][f], min_markers=1)
        cut = [c for c, r in enumerate(ref) if r["markers"] >= 1 and r["win"] >= 2 and not r["found"]]
        assert cut and all(not rec[f][c]["found"] and rec[f][c]["win"] >= 2 for c in cut)      # step 4 alone rejected them
    finally:   # the module's resident corners are those of the default options again
        rec2, _ = h.charuco_corners_batch(lay(capi, cr.LAYOUT), cr.IDS, frames)
        assert rec2.tobytes() == batch["rec"].tobytes()


def test_padded_host_frames_and_device_frames_give_the_same_bytes(batch, capi):
    import torch

    h, frames = batch["h"], batch["frames"]
    padded = np.full((len(frames), cr.H, cr.W + 32), 9, np.uint8)
    padded[:, :, :cr.W] = frames
    rec, nf = h.charuco_corners_batch(lay(capi, cr.LAYOUT), cr.IDS, padded, width=cr.W)
    assert rec.tobytes() == batch["rec"].tobytes() and np.array_equal(nf, batch["nf"])
    dev = torch.from_numpy(frames).cuda()
    rec, nf = h.charuco_corners_batch(lay(capi, cr.LAYOUT), cr.IDS, dev)
    assert rec.tobytes() == batch["rec"].tobytes() and np.array_equal(nf, batch["nf"])
    out = torch.zeros((len(frames), 12, 32), dtype=torch.uint8, device="cuda")
    nf = h.charuco_corners_batch_device(lay(capi, cr.LAYOUT), cr.IDS, dev.data_ptr(), len(frames), cr.W, cr.H, out.data_ptr())
    assert out.cpu().numpy().tobytes() == batch["rec"].tobytes() and np.array_equal(nf, batch["nf"])
    # fewer frames than the batch holds: the first ones
    rec, nf = h.charuco_corners_batch(lay(capi, cr.LAYOUT), cr.IDS, frames[:5])
    assert rec.tobytes() == batch["rec"][:5].tobytes()
    rec, _ = h.charuco_corners_batch(lay(capi, cr.LAYOUT), cr.IDS, frames)
    assert rec.tobytes() == batch["rec"].tobytes()


@pytest.mark.parametrize("square_px,marker_px,win", cr.WINDOW_LAYOUTS)
def test_margins_set_the_window(capi, square_px, marker_px, win):
    """a one-frame arucohip_detect, then the corners: the margin between marker and square decides the window, and a window of 1 is no corner"""
    L, (frame, _, _) = cr.window_frame(square_px, marker_px)
    h = capi.Handle(cr.W, cr.H)
    try:
        m = h.detect(frame)
        rec, nf = h.charuco_corners_batch(lay(capi, L), cr.IDS, frame[None])
        ref = check_frame(frame, rec[0], marker_list(m), L=L)
    finally:
        h.close()
    hit = [c for c, r in enumerate(ref) if r["markers"] == 2 and r["win"] == win and not r["fragile"]]
    assert hit, [r["win"] for r in ref]
    assert all(bool(rec[0][c]["found"]) == (win >= 2) and rec[0][c]["win"] == win for c in hit)


def test_a_frame_the_batch_gave_up_has_no_corners(capi):
    lim = capi.Limits()
    capi.load().arucohip_default_limits(C.byref(lim), cr.W, cr.H, 1)
    lim.contours_per_frame = 4
    h = capi.Handle(cr.W, cr.H, max_batch=1, limits=lim)
    try:
        frame = cr.frame("frontal")[0]
        markers, _, first = h.detect_batch_host_tolerant(frame[None], retry=False)
        assert markers[0] is None and first[0] == -1
        rec, nf = h.charuco_corners_batch(lay(capi, cr.LAYOUT), cr.IDS, frame[None])
        assert nf[0] == 0 and not rec["found"].any() and not rec["markers"].any() and not rec["x"].any()
        boards = h.charuco_pose_batch(1, KF, square_size=SQUARE_M)
        assert boards[0]["n_markers"] == 0 and boards[0]["has_pose"] == 0
    finally:
        h.close()


def _two_frames(capi, prepare):
    frames = np.stack([cr.frame("frontal")[0], cr.frame("turned")[0]])
    h = capi.Handle(cr.W, cr.H, max_batch=2)
    try:
        prepare(h)
        markers = h.detect_batch_host(frames)
        rec, nf = h.charuco_corners_batch(lay(capi, cr.LAYOUT), cr.IDS, frames)
        for f in range(2):
            ref = check_frame(frames[f], rec[f], marker_list(markers[f]))
            assert nf[f] == sum(r["found"] for r in ref) and nf[f] >= 8
    finally:
        h.close()


def test_pyr_down_level_one(capi):
    _two_frames(capi, lambda h: h.set_pyr_down(1))


def test_harris_marker_corners(capi):
    def harris(h):
        p = h.get_params()
        p.corner_method = capi.CORNER_HARRIS
        h.set_params(p)

    _two_frames(capi, harris)


def test_argument_errors(batch, capi):
    h, frames = batch["h"], batch["frames"]
    good = lay(capi, cr.LAYOUT)
    before = h.charuco_pose_batch(6, KF, square_size=SQUARE_M)

    def invalid(fn, *a, **k):
        with pytest.raises(capi.ArucoHipError) as e:
            fn(*a, **k)
        assert e.value.code == capi.E_INVALID

    for L in ((1, 4, 100, 70), (65, 4, 9, 7), (5, 1, 100, 70), (5, 65, 9, 7), (5, 4, 100, 6), (5, 4, 71, 70), (28, 20, 9, 7), (2, 2, 8192, 7)):
        nm = L[0] * L[1] // 2
        invalid(h.charuco_corners_batch, lay(capi, L), list(range(nm)), frames)
        invalid(h.charuco_board_image, lay(capi, L), list(range(nm)))
    invalid(h.charuco_corners_batch, good, cr.IDS[:9], frames)
    invalid(h.charuco_corners_batch, good, cr.IDS + [5], frames)
    invalid(h.charuco_board_image, good, cr.IDS[:9])
    invalid(h.charuco_board_image, good, cr.IDS[:9] + [1024])
    invalid(h.charuco_corners_batch, good, cr.IDS, np.concatenate([frames, frames[:1]]))      # nframes beyond the last batch
    invalid(h.charuco_corners_batch, good, cr.IDS, np.ascontiguousarray(frames[:, :-1]))   # not that batch's frame size
    for mw, mm in ((1, 2), (16, 2), (5, 0), (5, 3)):
        opt = capi.default_charuco()
        opt.max_win, opt.min_markers = mw, mm
        invalid(h.charuco_corners_batch, good, cr.IDS, frames, opt=opt)
    # a refused call leaves the resident corners alone
    assert h.charuco_pose_batch(6, KF, square_size=SQUARE_M).tobytes() == before.tobytes()
    invalid(h.charuco_pose_batch, 7, KF, square_size=SQUARE_M)
    invalid(h.charuco_pose_batch, 6, KF, square_size=SQUARE_M, min_corners=3)
    invalid(h.charuco_pose_batch, 6, KF, dist=np.zeros(3, np.float32), square_size=SQUARE_M)
    invalid(h.charuco_calibrate_batch, (cr.W, cr.H), min_corners=3)
    invalid(h.charuco_calibrate_batch, (cr.W, cr.H), min_corners=13)                          # no frame has that many
    fresh = capi.Handle(cr.W, cr.H)
    try:
        invalid(fresh.charuco_corners_batch, good, cr.IDS, frames[:1])                         # no batch at all
        invalid(fresh.charuco_calibrate_batch, (cr.W, cr.H))
    finally:
        fresh.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# the consumers
# ---------------------------------------------------------------------------------------------------------------------------------
def corner_objects(L, square_size):
    """the object points as the library forms them: the corner's board pixel times square_size / square_px in double, rounded to float"""
    _, cobj = cr.objects(L)
    scale = np.float64(np.float32(square_size)) / np.float64(L[2]) if square_size > 0 else 1.0
    return (cobj.astype(np.float64) * scale).astype(np.float32)


def test_calibration_from_the_resident_corners(capi):
    L, ids = cr.CALIB_LAYOUT, cr.CALIB_IDS
    views = cr.calib_frames()
    frames = np.stack([v[0] for v in views])
    size = 0.08
    h = chunked_handle(capi, 9, 3)
    try:
        h.detect_batch_host(frames)
        assert h.batch_chunks()[0] == 3
        rec, nf = h.charuco_corners_batch(lay(capi, L), ids, frames)
        print("found corners per view", nf.tolist())
        assert np.all(nf[:8] >= 16) and 4 <= nf[8] < 10
        got = h.charuco_calibrate_batch((cr.W, cr.H), square_size=size, min_corners=10)
        assert got["used"].tolist() == [True] * 8 + [False]
        cobj = corner_objects(L, size)
        objs = [cobj[rec[f]["found"] != 0] for f in range(8)]
        imgs = [np.stack([rec[f]["x"], rec[f]["y"]], axis=1)[rec[f]["found"] != 0] for f in range(8)]
        same = h.calibrate_camera(objs, imgs, (cr.W, cr.H))
        for k in ("K", "dist", "rvecs", "tvecs"):
            assert got[k].tobytes() == same[k].tobytes(), k
        assert got["rms"] == same["rms"]
        # every frame a view, and the solver's other start
        all9 = h.charuco_calibrate_batch((cr.W, cr.H), square_size=size, min_corners=4)
        assert all9["used"].all() and all9["rvecs"].shape == (9, 3)
    finally:
        h.close()
    ref = calib_ref.scipy_calibrate(objs, imgs, (cr.W, cr.H))
    gi = calib_ref.intr_of_result(got)
    print("intrinsics", gi, "scipy", ref["intr"], "rms", got["rms"], ref["rms"])
    # the tolerance of test_gpu_calib.py: intrinsics 1e-6 relative, distortion 1e-6 absolute (scale 1), rms 1e-7 relative
    scale = np.concatenate([np.abs(ref["intr"][:4]), np.maximum(np.abs(ref["intr"][4:]), 1.0)])
    assert np.all(np.abs(gi - ref["intr"]) <= 1e-6 * scale), (gi, ref["intr"])
    assert abs(got["rms"] - ref["rms"]) <= 1e-7 * ref["rms"], (got["rms"], ref["rms"])
    assert abs(got["K"][0, 0] / cr.K[0, 0] - 1) < 0.05 and abs(got["K"][1, 1] / cr.K[1, 1] - 1) < 0.05 and got["rms"] < 0.3


def _pose_reference(name, rec, y_perp=False):
    """pose_ref's polished minimum over the found corners, started at the pose the frame was rendered with (the device's object points are
    not centred: the renderer's translation, moved to the board's corner)"""
    from oracle import orc

    rv, tv, _, _ = cr.scenes()[name]
    Wb, Hb, _, _ = cr.board_size(cr.LAYOUT)
    R = pose_ref.rodrigues(np.array(rv, np.float64))
    t0 = np.array(tv, np.float64) - R @ (np.array([Wb / 2.0, Hb / 2.0, 0.0]) * cr.UNIT)
    keep = rec["found"] != 0
    obj = corner_objects(cr.LAYOUT, SQUARE_M)[keep]
    img = np.stack([rec["x"], rec["y"]], axis=1)[keep]
    r, t = pose_ref.polished_minimum(obj, img, cr.K, np.zeros(5), (np.array(rv, np.float64), t0))
    return (orc.rotate_x_axis(r) if y_perp else r), t, int(keep.sum())


def test_pose_from_the_resident_corners(batch, capi):
    h = batch["h"]
    boards = h.charuco_pose_batch(6, KF, square_size=SQUARE_M)
    turned = h.charuco_pose_batch(6, KF, dist=np.zeros(5, np.float32), square_size=SQUARE_M, y_perp=True)
    for f, name in enumerate(cr.BATCH):
        b, n = boards[f], int(batch["nf"][f])
        assert b["n_markers"] == n == turned[f]["n_markers"]
        if name == "empty":
            assert b["has_pose"] == 0 and not b["rvec"].any() and not b["tvec"].any()
            continue
        assert b["has_pose"] == 1 and turned[f]["has_pose"] == 1
        for got, y in ((b, False), (turned[f], True)):
            r, t, cnt = _pose_reference(name, batch["rec"][f], y)
            assert cnt == n
            d = pose_ref.pose_dev(got["rvec"], got["tvec"], r, t)
            print("%-8s y_perp %d: R / t against the polished minimum %.3g %.3g" % (name, y, d[0], d[1]))
            assert max(d) < pose_ref.POSE_TOL
    # a frame below min_corners, the first frames only, and no K
    few = h.charuco_pose_batch(4, KF, square_size=SQUARE_M, min_corners=7)
    f = cr.BATCH.index("outside")
    assert len(few) == 4 and batch["nf"][f] == 6 and few[f]["has_pose"] == 0 and few[f]["n_markers"] == 6 and not few[f]["tvec"].any()
    assert few[:3].tobytes() == boards[:3].tobytes()
    nok = h.charuco_pose_batch(6, None, square_size=SQUARE_M)
    assert not nok["has_pose"].any() and np.array_equal(nok["n_markers"], batch["nf"])
