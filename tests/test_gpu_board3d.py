"""Board pose of boards out of a plane on the device (aruco_amd/csrc/pnp3d_device.h): arucohip_board_detect, arucohip_board_detect_batch
and arucohip_board_recover_batch against tests/board3d_ref.py, the float64 restatement of solvePnP's general start followed by a polished
reprojection minimum. Every comparison is at the project's pose tolerance (1e-4) in both measures of pose_ref.pose_dev. Corners are handed
in unless a test says that it detects."""
import numpy as np
import pytest

from tests import board3d_ref as b3
from tests import pose_ref
from tests.planar_ref import rodrigues, rotate_x_axis

pytestmark = pytest.mark.gpu
TOL = pose_ref.POSE_TOL
SIZE = b3.MARKER_SIZE
METERS = 1


@pytest.fixture(scope="module")
def handle():
    import torch  # noqa: F401  (torch's HIP runtime first, see aruco_amd/capi.py)
    from aruco_amd import capi

    h = capi.Handle(b3.W, b3.H, max_batch=8)
    yield h
    h.close()


def _markers(ids, corners):
    from aruco_amd import capi

    c = np.asarray(corners, np.float32).reshape(-1, 8)
    m = np.zeros(len(c), capi.MARKER_DTYPE)
    m["id"] = np.asarray(ids)
    m["corners"] = c
    m["ssize"] = -1
    return m


def _detect(handle, v, markers=None, **kw):
    m = _markers(v["ids"], v["corners"]) if markers is None else markers
    return handle.board_detect(m, v["ids"], v["obj"], METERS, K=v["K"], dist=v["dist"], marker_size=SIZE, **kw)


def _ref_of(v, keep=None):
    obj, img = np.asarray(v["obj"], np.float64).reshape(-1, 3), v["corners"].reshape(-1, 2)
    if keep is not None:
        obj, img = obj[keep], img[keep]
    return b3.solve(obj, img, v["K"], v["dist"])


@pytest.mark.parametrize("nm", b3.FOLD_SIZES)
@pytest.mark.parametrize("angle", b3.FOLD_ANGLES)
def test_fold_pose_is_the_references_polished_minimum(handle, angle, nm):
    """1. Every judged fold case through arucohip_board_detect: 8 points (the smallest DLT), 12, 60, 64 (one point per lane), 68 (a second
    trip), 256 and 512 (the batched kernel's capacity). Without pnp3d_device.h the call returns has_pose = 0 on all of them."""
    cases = [c for c in b3.judged_cases() if c["angle"] == angle and c["nm"] == nm and c["gate"]["judged"]]
    assert len([c for c in cases if c["noise"] == 0]) == len(b3.FOLD_POSES)
    worst = 0.0
    for c in cases:
        got = _detect(handle, c["view"])
        ref = c["gate"]["ref"]
        assert got["has_pose"] == 1 and got["prob"] == 1.0 and ref["branch"] == "d"
        d = pose_ref.pose_dev(got["rvec"], got["tvec"], ref["rvec"], ref["tvec"])
        worst = max(worst, max(d))
        assert max(d) < TOL, (c["pose"], c["noise"], d)
    print("fold %2g deg, %3d markers: %d judged cases, worst R/t against the reference %.3g" % (angle, nm, len(cases), worst))


def test_cube_faces(handle):
    for pose in b3.FOLD_POSES:
        v = b3.view(b3.cube_faces(), pose, 0.0, pose_ref.K_MAIN, seed=4103)
        got, ref = _detect(handle, v), _ref_of(v)
        assert got["has_pose"] == 1 and max(pose_ref.pose_dev(got["rvec"], got["tvec"], ref["rvec"], ref["tvec"])) < TOL


def _tilted_boards():
    out = [("lifted %d" % nm, pose_ref.board(nm), b3.LIFT) for nm in (1, 16, 17)]
    ids, obj = pose_ref.board(16)
    out.append(("z = 0.25", (ids, obj), (np.zeros(3), np.array([0.0, 0.0, 0.25]))))
    return out


@pytest.mark.parametrize("which", range(4))
def test_tilted_plane_equals_the_flat_board_composed_with_its_transform(handle, which):
    """2. Planar boards whose plane is not z = 0: within 1e-4 of the reference, and of the device pose of the same corners on the z = 0
    board composed with the transform."""
    name, flat, lift = _tilted_boards()[which]
    moved = b3.lifted(flat, lift)
    for pose in b3.FOLD_POSES:
        v = b3.view(moved, pose, pose_ref.NOISE, pose_ref.K_MAIN, seed=5200 + which)
        got, ref = _detect(handle, v), _ref_of(v)
        assert ref["branch"] == "c" and got["has_pose"] == 1
        d_ref = pose_ref.pose_dev(got["rvec"], got["tvec"], ref["rvec"], ref["tvec"])
        v0 = dict(v, obj=flat[1])
        got0 = _detect(handle, v0)
        assert got0["has_pose"] == 1
        Rc, tc = b3.compose(got0["rvec"], got0["tvec"], lift)
        d_flat = pose_ref.pose_dev(got["rvec"], got["tvec"], Rc, tc)
        print("%-10s %-5s against the reference %.3g, against the composed flat pose %.3g" % (name, pose, max(d_ref), max(d_flat)))
        assert max(d_ref) < TOL and max(d_flat) < TOL


def test_one_panel_of_a_fold_is_a_tilted_plane(handle):
    ids, obj, panel = b3.fold(16, 90.0)
    for pose in b3.FOLD_POSES:
        v = b3.view((ids, obj), pose, pose_ref.NOISE, pose_ref.K_MAIN, seed=5300)
        keep = panel == 1
        got = _detect(handle, v, _markers(ids[keep], v["corners"][keep]))
        ref = _ref_of(v, np.repeat(keep, 4))
        assert ref["branch"] == "c" and got["has_pose"] == 1 and len(got["markers"]) == 8
        assert max(pose_ref.pose_dev(got["rvec"], got["tvec"], ref["rvec"], ref["tvec"])) < TOL


@pytest.mark.parametrize("n_out", (1, 3, 6))
def test_reprojection_filter_on_a_fold(handle, n_out):
    """3. Corners moved by 25 px, threshold 5: the second solve runs without them and gives the pose of the board without those corners.
    arucohip_board_detect takes whole markers, so the pose without single corners is the reference's on the kept points."""
    v = b3.view(b3.fold(16, 90.0), "mild", pose_ref.NOISE, pose_ref.K_MAIN, seed=5400 + n_out)
    rng = np.random.default_rng(5500 + n_out)
    moved = rng.choice(64, n_out, replace=False)
    c = v["corners"].reshape(-1, 2).copy()
    a = rng.uniform(0.0, 2 * np.pi, n_out)
    c[moved] += np.float32(25.0) * np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32)
    got = _detect(handle, v, _markers(v["ids"], c), repj_err_thres=5.0)
    plain = _detect(handle, v, _markers(v["ids"], c))
    keep = np.ones(64, bool)
    keep[moved] = False
    ref = _ref_of(dict(v, corners=c), keep)
    assert got["has_pose"] == 1 and plain["has_pose"] == 1
    d = pose_ref.pose_dev(got["rvec"], got["tvec"], ref["rvec"], ref["tvec"])
    shift = max(pose_ref.pose_dev(plain["rvec"], plain["tvec"], ref["rvec"], ref["tvec"]))
    print("%d corners moved: unfiltered pose off by %.3g, filtered against the board without them %.3g" % (n_out, shift, max(d)))
    assert shift > TOL and max(d) < TOL


def test_y_perpendicular_is_rotate_x_axis_of_the_plain_pose(handle):
    """4."""
    v = b3.fold_case(90.0, 16, "mild", pose_ref.NOISE)
    plain, turned = _detect(handle, v), _detect(handle, v, y_perp=True)
    assert plain["has_pose"] == turned["has_pose"] == 1
    assert np.array_equal(turned["tvec"], plain["tvec"])
    exp = rotate_x_axis(plain["rvec"])
    assert np.max(np.abs(rodrigues(turned["rvec"]) - rodrigues(exp))) < 1e-6   # float arithmetic of rotateXAxis on both sides


def test_hostile_input_gives_no_pose_and_no_error(handle):
    """5. Ordinary numbers that the solver must reject; the handle answers the next call as before.
    - non-planar with n = 4, a fold with a NaN corner: has_pose = 0, return code OK (board_detect raises on any other).
    - 8 points of which seven are coplanar and one is 1e-4 m off: w2 / w1 is about 1e-6, far below the 1e-3 switch, so rule c applies
      and solvePnP poses these points through the homography; the reference restatement does, and so must the device, with the same
      pose. (A solver that sent them to the DLT would meet a normal matrix of rank 11 and must not return a pose from it.)"""
    from aruco_amd import capi

    ids, obj, _ = b3.fold(2, 90.0)
    v = b3.view((ids, obj), "mild", 0.0, pose_ref.K_MAIN, seed=5600)
    # n = 4 out of a plane: one marker whose fourth corner is bent out
    o1 = obj[:1].copy()
    o1[0, 3, 2] += 0.02
    px = pose_ref.brown_project(o1.reshape(-1, 3).astype(np.float64), v["R"], v["t"], v["K"], None).astype(np.float32)
    got = handle.board_detect(_markers(ids[:1], px), ids[:1], o1, METERS, K=v["K"], marker_size=SIZE)
    assert got["has_pose"] == 0 and len(got["markers"]) == 1 and got["prob"] == 1.0
    assert b3.start_pose(o1.reshape(-1, 3), px, v["K"], None) is None
    # NaN corner
    c = v["corners"].copy()
    c[1, 2, 0] = np.nan
    got = _detect(handle, v, _markers(ids, c))
    assert got["has_pose"] == 0 and len(got["markers"]) == 2
    # seven coplanar points and one 1e-4 m off
    ids2, flat = pose_ref.board(2)
    o2 = flat.copy()
    o2[1, 2, 2] = 1e-4
    v2 = b3.view((ids2, o2), "mild", 0.0, pose_ref.K_MAIN, seed=5601)
    r = b3.spread_ratio(o2)
    got, ref = _detect(handle, v2), _ref_of(v2)
    print("seven coplanar points and one 1e-4 m off: w2/w1 = %.3g, reference branch %s, device has_pose %d" % (r, ref["branch"], got["has_pose"]))
    assert r < 1e-5 and ref["branch"] == "c"
    assert got["has_pose"] == 1 and max(pose_ref.pose_dev(got["rvec"], got["tvec"], ref["rvec"], ref["tvec"])) < TOL
    assert np.all(np.isfinite(got["rvec"])) and np.all(np.isfinite(got["tvec"]))
    # no error state: a planar board is answered as ever
    pv = pose_ref.board_view(16, "mild", 0.0, pose_ref.K_MAIN, seed=5602)
    ok = _detect(handle, pv)
    assert ok["has_pose"] == 1 and max(pose_ref.pose_dev(ok["rvec"], ok["tvec"], pv["R"], pv["t"])) < TOL
    assert capi.OK == 0


def _check_batch(h, frames, markers, board, shown):
    ids, obj = board[0], board[1]
    KF = b3.K_FRAME.astype(np.float32)
    boards = h.board_detect_batch(len(frames), ids, obj, METERS, K=KF, marker_size=SIZE)
    again = h.board_detect_batch(len(frames), ids, obj, METERS, K=KF, marker_size=SIZE)
    bitwise = True
    for f in range(len(frames)):
        m = markers[f]
        assert len(m) == shown[f] == boards[f]["n_markers"], (f, len(m))
        if shown[f] == 0:
            assert boards[f]["has_pose"] == 0 and boards[f]["prob"] == 0
            continue
        one = h.board_detect(m, ids, obj, METERS, K=KF, marker_size=SIZE)
        assert boards[f]["has_pose"] == one["has_pose"] == 1
        assert max(pose_ref.pose_dev(boards[f]["rvec"], boards[f]["tvec"], one["rvec"], one["tvec"])) < TOL
        bitwise = bitwise and np.array_equal(boards[f]["rvec"], one["rvec"]) and np.array_equal(boards[f]["tvec"], one["tvec"])
        slot = [list(ids).index(int(i)) for i in m["id"]]
        ref = b3.solve(np.asarray(obj, np.float64)[slot].reshape(-1, 3), np.asarray(m["corners"], np.float64).reshape(-1, 2), b3.K_FRAME, None)
        assert ref["branch"] == ("c" if shown[f] == 6 else "d")
        d = pose_ref.pose_dev(boards[f]["rvec"], boards[f]["tvec"], ref["rvec"], ref["tvec"])
        Rt = b3.frame_pose(f)
        print("frame %d: %2d markers, batch against the reference %.3g, against the painted pose %.3g" % (
            f, shown[f], max(d), max(pose_ref.pose_dev(boards[f]["rvec"], boards[f]["tvec"], Rt[2], Rt[1]))))
        assert max(d) < TOL
        # the same input gives the same bits on every run
        assert np.array_equal(boards[f]["rvec"], again[f]["rvec"]) and np.array_equal(boards[f]["tvec"], again[f]["tvec"])
    print("batch and single call equal to the bit: %s" % bitwise)


def test_batch_path_on_rendered_frames(monkeypatch):
    """6. 640 x 480, the 12-marker 90 degree fold detected at five poses over two chunk workers (one frame shows one panel: the tilted
    branch; one is empty), and the same batch as a pipeline ticket."""
    import torch  # noqa: F401
    from aruco_amd import capi

    board, frames, shown = b3.batch_frames()
    KF = b3.K_FRAME.astype(np.float32)
    monkeypatch.setenv("ARUCOHIP_STREAMS", "2")
    h = capi.Handle(b3.W, b3.H, max_batch=5)
    monkeypatch.delenv("ARUCOHIP_STREAMS")
    try:
        markers = h.detect_batch_host(frames, K=KF, marker_size=SIZE)
        assert len(h.batch_chunks()) == 2
        _check_batch(h, frames, markers, board, shown)
    finally:
        h.close()
    h = capi.Handle(b3.W, b3.H, max_batch=5)
    try:
        h.set_pipeline_depth(2)
        out, n = np.zeros((5, 64), capi.MARKER_DTYPE), np.zeros(5, np.int32)
        out2, n2 = out.copy(), n.copy()
        t = h.submit_host(frames, out, n, K=KF, marker_size=SIZE)
        t2 = h.submit_host(frames[::-1].copy(), out2, n2, K=KF, marker_size=SIZE)
        h.wait(t2)
        h.wait(t)   # the last batch is the first ticket's
        _check_batch(h, frames, [out[f, :n[f]].copy() for f in range(5)], board, shown)
    finally:
        h.close()


def test_recovery_on_a_fold_frame():
    """7. Two cells of marker 6 repainted: the decoder rejects it, the recovery projects it with all three coordinates and takes it back
    with its id; the board pose after the recovery is arucohip_board_detect's on the returned markers."""
    import torch  # noqa: F401
    from aruco_amd import capi

    board = b3.fold(12, 90.0)
    ids, obj = board[0], board[1]
    rvec, tvec, _ = b3.frame_pose(1)
    gray = b3.render(board, rvec, tvec, seed=21, damage={6: [(2, 2), (4, 3)]})
    KF = b3.K_FRAME.astype(np.float32)
    h = capi.Handle(b3.W, b3.H, max_batch=1)
    try:
        m = h.detect(gray, K=KF, marker_size=SIZE)
        assert sorted(int(i) for i in m["id"]) == [int(i) for i in ids if i != ids[6]]
        out, n, rec, boards = h.board_recover_batch(1, ids, obj, METERS, KF, marker_size=SIZE)
        assert rec[0] == 1 and n[0] == 12 and sorted(int(i) for i in out[0]["id"]) == [int(i) for i in ids]
        one = h.board_detect(out[0], ids, obj, METERS, K=KF, marker_size=SIZE)
        assert boards[0]["has_pose"] == one["has_pose"] == 1 and boards[0]["n_markers"] == 12
        d = pose_ref.pose_dev(boards[0]["rvec"], boards[0]["tvec"], one["rvec"], one["tvec"])
        print("pose after the recovery against board_detect on the returned markers: %.3g" % max(d))
        assert max(d) < TOL
    finally:
        h.close()
