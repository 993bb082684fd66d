"""The fisheye calls on the device against the float64 restatement (tests/fisheye_ref.py): points, frames and the resident markers of
a batch. 640 x 480 frames of the golden board through a lens of roughly 200 degrees (tests/test_fisheye_cpu.py checks the restatement
and the inputs' margins on the CPU)."""
import numpy as np
import pytest

from tests import fisheye_ref as fr

pytestmark = pytest.mark.gpu

REL_TOL = 1e-4   # the project's standing device-versus-oracle bound, for corners (relative to the coordinate) and poses
MODEL, MODEL2 = (fr.K, fr.D), (fr.K2, fr.D2)
KNEW32 = fr.KNEW.astype(np.float32)


@pytest.fixture(scope="module")
def env():
    import torch  # noqa: F401  (torch's HIP runtime first, see aruco_amd/capi.py)
    from aruco_amd import capi
    from oracle import orc

    assert torch.cuda.is_available()
    frames = np.stack([fr.fisheye_frame(0), fr.fisheye_frame(1)])
    ids, obj = fr.board()
    return {"capi": capi, "orc": orc, "torch": torch, "frames": frames, "ids": ids, "obj": obj,
            "oracle": [orc.Oracle().detect(g) for g in frames]}


def make_handle(env, max_batch=1):
    return env["capi"].Handle(fr.W, fr.H, max_batch=max_batch)


def as_dicts(ms):
    return [{"id": int(m["id"]), "corners": np.array(m["corners"], np.float32).reshape(4, 2)} for m in ms]


def assert_one_ulp(got, want64):
    """A float result against the float-rounded float64 value: the double error is orders below a float ulp, so they can differ only
    where the double value sits at a rounding boundary, by one ulp."""
    want = np.asarray(want64, np.float64).astype(np.float32)
    got = np.asarray(got, np.float32).reshape(want.shape)
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))
    assert np.array_equal(got[want == 0], want[want == 0])


def assert_ref_markers(got, before, model, Knew, max_angle=0.0):
    """got (a frame's list after the call) against the restatement on the list before it; returns the dropped count"""
    want, dropped, margin = fr.undistort_markers(as_dicts(before), model[0], model[1], Knew, max_angle)
    assert margin > 1e-9
    assert [int(m["id"]) for m in got] == [m["id"] for m in want]
    for a, b in zip(got, want):
        assert_one_ulp(a["corners"], b["corners"].astype(np.float64).reshape(8))   # the restated corners are float-rounded already
        assert int(a["has_pose"]) == 0 and float(a["ssize"]) == -1.0
    return dropped


# ---- points
def test_points_against_the_restatement(env):
    capi, torch = env["capi"], env["torch"]
    h = make_handle(env)
    try:
        pts, edge_from = fr.point_cases()
        want, wvalid, margin = fr.undistort_points(pts, fr.K, fr.D, fr.KNEW, fr.POINTS_MAX_ANGLE)
        assert (margin > 1e-9).all() and list(wvalid[edge_from:]) == [True, False, True, False]
        got, valid = h.fisheye_undistort_points(pts, MODEL, KNEW32, fr.POINTS_MAX_ANGLE)
        assert np.array_equal(valid, wvalid)
        assert_one_ulp(got, want)
        # Knew = NULL is K, max_angle <= 0 is 1.4
        got0, valid0 = h.fisheye_undistort_points(pts, MODEL)
        want0, wvalid0, margin0 = fr.undistort_points(pts, fr.K, fr.D)
        assert (margin0 > 1e-9).all() and np.array_equal(valid0, wvalid0)
        assert_one_ulp(got0, want0)
        # a theta_d that turns back: no root, invalid
        nm = fr.not_monotone_cases()
        gotn, validn = h.fisheye_undistort_points(nm, (fr.K, fr.D_NOT_MONOTONE), KNEW32, fr.POINTS_MAX_ANGLE)
        wantn, wvalidn, _ = fr.undistort_points(nm, fr.K, fr.D_NOT_MONOTONE, fr.KNEW, fr.POINTS_MAX_ANGLE)
        assert list(validn) == [True, False, False] == list(wvalidn)
        assert_one_ulp(gotn, wantn)
        # the other direction, over the ideal frame and beyond it
        ys, xs = np.mgrid[-40:fr.H + 40:31, -40:fr.W + 40:29]
        ideal = np.stack([xs.ravel() + 0.5, ys.ravel() + 0.25], axis=1).astype(np.float32)
        assert_one_ulp(h.fisheye_distort_points(ideal, MODEL, KNEW32), fr.distort_points(ideal, fr.K, fr.D, fr.KNEW))
        assert_one_ulp(h.fisheye_distort_points(ideal, MODEL), fr.distort_points(ideal, fr.K, fr.D))
        # device arrays give the host path's bits
        d_src = torch.from_numpy(pts).cuda()
        d_dst = torch.full_like(d_src, 7.0)
        d_valid = torch.full((len(pts),), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        h.fisheye_points_device(d_src.data_ptr(), len(pts), d_dst.data_ptr(), MODEL, KNEW32, fr.POINTS_MAX_ANGLE, valid_ptr=d_valid.data_ptr())
        h.synchronize()
        assert d_dst.cpu().numpy().tobytes() == got.tobytes() and np.array_equal(d_valid.cpu().numpy().astype(bool), valid)
        d_ideal = torch.from_numpy(ideal).cuda()
        d_back = torch.empty_like(d_ideal)
        torch.cuda.synchronize()
        h.fisheye_points_device(d_ideal.data_ptr(), len(ideal), d_back.data_ptr(), MODEL, KNEW32)
        h.synchronize()
        assert d_back.cpu().numpy().tobytes() == h.fisheye_distort_points(ideal, MODEL, KNEW32).tobytes()
    finally:
        h.close()


def test_points_errors(env):
    capi = env["capi"]
    h = make_handle(env)
    try:
        pts = np.zeros((4, 2), np.float32)
        for bad in (dict(max_angle=1.5708), dict(max_angle=2.0)):
            with pytest.raises(capi.ArucoHipError) as e:
                h.fisheye_undistort_points(pts, MODEL, KNEW32, **bad)
            assert e.value.code == capi.E_INVALID
        skew = fr.K.copy()
        skew[0, 1] = 0.5
        for model, Knew in (((skew, fr.D), KNEW32), ((np.zeros((3, 3)), fr.D), KNEW32), (MODEL, np.zeros((3, 3), np.float32))):
            with pytest.raises(capi.ArucoHipError) as e:
                h.fisheye_undistort_points(pts, model, Knew)
            assert e.value.code == capi.E_INVALID
        out, valid = h.fisheye_undistort_points(np.zeros((0, 2), np.float32), MODEL)   # no points: nothing to do
        assert len(out) == 0 and len(valid) == 0
    finally:
        h.close()


# ---- frames
def assert_remap(got, img, table, cn):
    u32, v32, beyond = table
    want = fr.remap(img, u32, v32, beyond)
    diff = (got != want).reshape(fr.H, fr.W, cn).any(axis=2)
    # 1e-8: about the double evaluation error of 32 u and 32 v
    assert not (diff & ~fr.near_rounding_boundary(u32, v32, 1e-8)).any()
    return int(diff.sum())


@pytest.mark.parametrize("cn", [1, 3])
def test_frames_against_the_restated_remap(env, cn):
    torch = env["torch"]
    h = make_handle(env, 2)
    try:
        gray = env["frames"]
        imgs = gray if cn == 1 else np.stack([gray, 255 - gray, gray // 2 + 40], axis=3)
        table = fr.build_map(fr.W, fr.H, fr.K, fr.D, fr.KNEW, 1.0)   # at 1.0 rad the ideal frame's left and right edges lie beyond the lens
        assert table[2].any() and not table[2].all()
        # host source, one frame and two
        first = h.fisheye_undistort(imgs[0], MODEL, KNEW32, 1.0)
        assert_remap(first, imgs[0], table, cn)
        if cn == 1:
            both = h.fisheye_undistort(imgs, MODEL, KNEW32, 1.0)   # the kept map
            assert both[0].tobytes() == first.tobytes()
            assert_remap(both[1], imgs[1], table, cn)
        # device source with padded rows, device destination
        rs = fr.W * cn + 64
        padded = np.zeros((2, fr.H, rs), np.uint8)
        padded[:, :, :fr.W * cn] = imgs.reshape(2, fr.H, fr.W * cn)
        d_src = torch.from_numpy(padded).cuda()
        d_dst = torch.full((2, fr.H, fr.W * cn), 3, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        h.fisheye_undistort_device(d_src.data_ptr(), 2, fr.W, fr.H, cn, d_dst.data_ptr(), MODEL, KNEW32, 1.0, row_stride=rs)
        h.synchronize()
        dev = d_dst.cpu().numpy().reshape(imgs.shape)
        assert dev[0].tobytes() == first.tobytes()
        assert_remap(dev[1], imgs[1], table, cn)
        # another max_angle is another map
        wide = h.fisheye_undistort(imgs[0], MODEL, KNEW32)
        assert_remap(wide, imgs[0], fr.build_map(fr.W, fr.H, fr.K, fr.D, fr.KNEW), cn)
        assert wide.tobytes() != first.tobytes()
    finally:
        h.close()


def test_fisheye_and_pinhole_maps_do_not_collide(env):
    """arucohip_undistort with a pinhole model returns the same bytes before and after a fisheye call, and the other way round."""
    h = make_handle(env)
    try:
        g = env["frames"][0]
        Kp = np.array([[400.0, 0, 320], [0, 400.0, 240], [0, 0, 1]], np.float32)
        dist = [-0.2, 0.05, 1e-3, -5e-4, 0]
        pin = h.undistort(g, Kp, dist)
        fish = h.fisheye_undistort(g, MODEL, KNEW32)
        assert fish.tobytes() != pin.tobytes()
        assert h.undistort(g, Kp, dist).tobytes() == pin.tobytes()
        assert h.fisheye_undistort(g, MODEL, KNEW32).tobytes() == fish.tobytes()
        assert h.undistort(g, Kp, dist).tobytes() == pin.tobytes()
    finally:
        h.close()


# ---- markers in place
def test_markers_in_place_and_board_pose(env):
    capi, orc, ids, obj = env["capi"], env["orc"], env["ids"], env["obj"]
    h = make_handle(env, 2)
    try:
        before = h.detect_batch_host(env["frames"], K=fr.K.astype(np.float32), marker_size=fr.MARKER_SIZE)
        assert all(int(m["has_pose"]) == 1 for ms in before for m in ms)
        out, n, dropped = h.fisheye_undistort_markers_batch(2, MODEL, KNEW32)
        boards = h.board_detect_batch(2, ids, obj, capi.BOARD_PIX, K=KNEW32, marker_size=fr.MARKER_SIZE)
        for f in range(2):
            assert assert_ref_markers(out[f], before[f], MODEL, fr.KNEW) == 0 == dropped[f] and n[f] == 24
            # the CPU chain: oracle detection, restated undistortion, oracle board pose
            chain, _, _ = fr.undistort_markers(env["oracle"][f], fr.K, fr.D, fr.KNEW)
            assert [int(m["id"]) for m in out[f]] == [m["id"] for m in chain]
            for a, b in zip(out[f], chain):
                ca, cb = np.asarray(a["corners"], np.float64).reshape(4, 2), b["corners"].astype(np.float64)
                assert np.max(np.abs(ca - cb) / np.maximum(np.abs(cb), 1.0)) < REL_TOL
            ob = orc.board_detect(chain, ids, obj, capi.BOARD_PIX, fr.KNEW, None, fr.MARKER_SIZE)
            assert boards[f]["has_pose"] == 1 and boards[f]["n_markers"] == 24
            assert fr.rel_err(boards[f]["rvec"], ob["rvec"]) < REL_TOL and fr.rel_err(boards[f]["tvec"], ob["tvec"]) < REL_TOL
        # the flag: a second call is invalid, recovery and chessboard corners want the frames' own pixels
        with pytest.raises(capi.ArucoHipError) as e:
            h.fisheye_undistort_markers_batch(2, MODEL, KNEW32)
        assert e.value.code == capi.E_INVALID
        with pytest.raises(capi.ArucoHipError) as e:
            h.board_recover_batch(2, ids, obj, capi.BOARD_PIX, KNEW32, marker_size=fr.MARKER_SIZE)
        assert e.value.code == capi.E_UNSUPPORTED
        with pytest.raises(capi.ArucoHipError) as e:
            h.charuco_corners_batch(capi.charuco_layout((5, 4), 100, 70), list(range(10)), env["frames"])
        assert e.value.code == capi.E_UNSUPPORTED
        # the lists stayed as the call left them
        again = h.board_detect_batch(2, ids, obj, capi.BOARD_PIX, K=KNEW32, marker_size=fr.MARKER_SIZE)
        assert all(np.array_equal(again[f]["tvec"], boards[f]["tvec"]) for f in range(2))
        # a new detection clears the flag
        assert [m.tobytes() for m in h.detect_batch_host(env["frames"], K=fr.K.astype(np.float32), marker_size=fr.MARKER_SIZE)] == [m.tobytes() for m in before]
        out2, _, _ = h.fisheye_undistort_markers_batch(2, MODEL, KNEW32)
        assert [m.tobytes() for m in out2] == [m.tobytes() for m in out]
    finally:
        h.close()


def test_markers_device_copy_equals_the_resident_list(env):
    capi, torch = env["capi"], env["torch"]
    h = make_handle(env, 2)
    try:
        h.detect_batch_host(env["frames"])
        cap = 32
        d_out = torch.zeros((2, cap, 96), dtype=torch.uint8, device="cuda")
        d_n = torch.zeros(2, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        h.fisheye_undistort_markers_batch_device(2, MODEL, d_out.data_ptr(), cap, d_n.data_ptr(), KNEW32)
        h.synchronize()
        got = np.frombuffer(d_out.cpu().numpy().tobytes(), capi.MARKER_DTYPE).reshape(2, cap)
        assert d_n.cpu().tolist() == [24, 24]
        # the resident list, read by a fresh handle's host path on the same frames
        h2 = make_handle(env, 2)
        try:
            h2.detect_batch_host(env["frames"])
            out, n, _ = h2.fisheye_undistort_markers_batch(2, MODEL, KNEW32, cap=cap)
        finally:
            h2.close()
        assert all(got[f, :24].tobytes() == out[f].tobytes() for f in range(2))
        # and the planar solver reads the same resident corners: K = Knew, no distortion
        poses = np.frombuffer(h.planar_poses_batch(2, KNEW32, None, fr.MARKER_SIZE, cap=cap), capi.PLANAR_DTYPE).reshape(2, cap)
        assert (poses["n_solutions"][:, :24] == 2).all() and (poses["n_solutions"][:, 24:] == 0).all()
        # solution 0 of a marker about 0.2 m away
        assert (np.abs(poses["tvec"][:, :24, 0, 2] - 0.21) < 0.06).all()
        # a too small output array: the counts and ARUCOHIP_E_CAPACITY
        h.detect_batch_host(env["frames"])
        out, n, dropped = h.fisheye_undistort_markers_batch(2, MODEL, KNEW32, cap=5, allow=(capi.E_CAPACITY,))
        assert list(n) == [24, 24] and all(len(o) == 5 for o in out) and list(dropped) == [0, 0]
    finally:
        h.close()


def test_small_max_angle_drops_what_the_restatement_drops(env):
    h = make_handle(env, 2)
    try:
        before = h.detect_batch_host(env["frames"])
        out, n, dropped = h.fisheye_undistort_markers_batch(2, MODEL, KNEW32, max_angle=0.6)
        for f, want in enumerate((4, 8)):
            assert assert_ref_markers(out[f], before[f], MODEL, fr.KNEW, 0.6) == want == dropped[f]
            assert n[f] == 24 - want
    finally:
        h.close()


def test_two_lenses_interleaved(env):
    """Frame f uses models[f % nmodels]: a stream of two cameras taking turns equals two one-model runs."""
    h = make_handle(env, 4)
    try:
        frames = np.concatenate([env["frames"], env["frames"]])
        Knew2 = np.stack([fr.KNEW, fr.KNEW * np.array([[1.1], [0.9], [1.0]])]).astype(np.float32)
        before = h.detect_batch_host(frames)
        both, _, _ = h.fisheye_undistort_markers_batch(4, [MODEL, MODEL2], Knew2)
        h.detect_batch_host(frames)
        one, _, _ = h.fisheye_undistort_markers_batch(4, MODEL, Knew2[0])
        h.detect_batch_host(frames)
        two, _, _ = h.fisheye_undistort_markers_batch(4, MODEL2, Knew2[1])
        for f in range(4):
            assert both[f].tobytes() == (one, two)[f % 2][f].tobytes()
            assert_ref_markers(both[f], before[f], (MODEL, MODEL2)[f % 2], Knew2[f % 2].astype(np.float64))
        assert both[1].tobytes() != one[1].tobytes()
    finally:
        h.close()


def test_two_spans_equal_one_span(env, monkeypatch):
    """Four frames on two chunk workers give the bytes of one worker: the host lists, counts and dropped counts, and the device copy.
    max_angle = 0.6 drops markers, so that the dropped counts and the compacted lists carry something."""
    capi, torch = env["capi"], env["torch"]
    frames = np.concatenate([env["frames"], env["frames"]])
    cap = 32

    def run(h, chunks):
        h.detect_batch_host(frames)
        assert h.batch_chunks() == chunks
        out, n, dropped = h.fisheye_undistort_markers_batch(4, MODEL, KNEW32, max_angle=0.6, cap=cap)
        h.detect_batch_host(frames)
        d_out = torch.zeros((4, cap, 96), dtype=torch.uint8, device="cuda")
        d_n = torch.zeros(4, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        h.fisheye_undistort_markers_batch_device(4, MODEL, d_out.data_ptr(), cap, d_n.data_ptr(), KNEW32, max_angle=0.6)
        h.synchronize()
        dev = np.frombuffer(d_out.cpu().numpy().tobytes(), capi.MARKER_DTYPE).reshape(4, cap)
        dn = d_n.cpu().tolist()
        return [o.tobytes() for o in out], list(n), list(dropped), [dev[f, :dn[f]].tobytes() for f in range(4)], dn

    monkeypatch.setenv("ARUCOHIP_STREAMS", "2")
    h2 = make_handle(env, 4)
    monkeypatch.delenv("ARUCOHIP_STREAMS")
    h1 = make_handle(env, 4)
    try:
        two, one = run(h2, (2, 2)), run(h1, (1, 4))
        assert two == one
        lists, n, dropped, dev, dn = two
        assert dev == lists and dn == n   # the device copy holds what the host lists hold
        assert dropped == [4, 8, 4, 8] and n == [20, 16, 20, 16]   # test_small_max_angle_drops_what_the_restatement_drops
    finally:
        h1.close()
        h2.close()


def test_one_frame_detect_keeps_its_graph(env):
    capi = env["capi"]
    h = make_handle(env)
    try:
        g = env["frames"][0]
        for _ in range(3):   # eager, capture, replay of the single-frame graph
            m = h.detect(g)
        out, n, dropped = h.fisheye_undistort_markers_batch(1, MODEL, KNEW32)
        assert assert_ref_markers(out[0], m, MODEL, fr.KNEW) == 0 and n[0] == 24
        with pytest.raises(capi.ArucoHipError) as e:
            h.fisheye_undistort_markers_batch(1, MODEL, KNEW32)
        assert e.value.code == capi.E_INVALID
        again = h.detect(g)   # replays, and clears the flag
        assert again.tobytes() == m.tobytes()
        out2, _, _ = h.fisheye_undistort_markers_batch(1, MODEL, KNEW32)
        assert out2[0].tobytes() == out[0].tobytes()
    finally:
        h.close()


def test_markers_errors(env):
    capi = env["capi"]
    h = make_handle(env, 2)
    try:
        with pytest.raises(capi.ArucoHipError) as e:   # no batch yet
            h.fisheye_undistort_markers_batch(1, MODEL)
        assert e.value.code == capi.E_INVALID
        h.detect_batch_host(env["frames"])
        for call in (lambda: h.fisheye_undistort_markers_batch(3, MODEL), lambda: h.fisheye_undistort_markers_batch(2, MODEL, max_angle=1.6),
                     lambda: h.fisheye_undistort_markers_batch(2, [])):
            with pytest.raises(capi.ArucoHipError) as e:
                call()
            assert e.value.code == capi.E_INVALID
        # none of them touched the lists or set the flag
        out, n, _ = h.fisheye_undistort_markers_batch(2, MODEL, cap=0)
        assert all(len(o) == 0 for o in out) and n is None
        boards = h.board_detect_batch(2, env["ids"], env["obj"], capi.BOARD_PIX, K=fr.K.astype(np.float32), marker_size=fr.MARKER_SIZE)
        assert all(b["n_markers"] == 24 for b in boards)
    finally:
        h.close()


# ---- calibration
SIZE = (fr.W, fr.H)
# distance of the restated LM's end point from scipy's minimum in k1..k4 on the noisy views, measured on the CPU
# (tests/test_fisheye_cpu.py): 3.9e-10. k2..k4 lie in a flat valley of the cost, so the device may end that far from the restatement's
# end point, plus 1e-6 max(|k|, 1); the tests measure the distance again for the flags they run with.
LM_TO_SCIPY_K = 3.9e-10


@pytest.fixture(scope="module")
def views():
    return {"clean": fr.make_views(12), "noisy": fr.make_views(12, noise=0.3)}


def assert_matches_lm(res, objs, imgs, flags=0, model=None):
    """the device against the restated LM: f and c 1e-6 relative, rms 1e-7 relative, k within the LM's own distance from scipy's
    minimum plus 1e-6 max(|k|, 1)"""
    lm = fr.lm_calibrate(objs, imgs, SIZE, flags, model)
    sc = fr.scipy_calibrate(objs, imgs, SIZE, flags, model)
    got = fr.intr_of_result(res)
    assert np.max(np.abs(got[:4] - lm["intr"][:4]) / np.abs(lm["intr"][:4])) < 1e-6
    assert abs(res["rms"] - lm["rms"]) < 1e-7 * lm["rms"]
    dist = np.abs(lm["intr"][4:] - sc["intr"][4:])
    assert np.all(np.abs(got[4:] - lm["intr"][4:]) <= dist + 1e-6 * np.maximum(np.abs(lm["intr"][4:]), 1.0))
    return got, lm


def test_calibration_recovers_the_truth(env, views):
    h = make_handle(env)
    try:
        objs, imgs = views["clean"]
        res = h.fisheye_calibrate(objs, imgs, SIZE)
        got = fr.intr_of_result(res)
        assert np.max(np.abs(got[:4] - fr.INTR_TRUE[:4]) / fr.INTR_TRUE[:4]) < 1e-5
        assert np.max(np.abs(got[4:] - fr.INTR_TRUE[4:])) < 1e-4 and res["rms"] < 1e-3
        assert res["K"][0, 1] == 0 and res["K"][2, 2] == 1
        # the poses project the board where the views saw it
        for v in range(len(objs)):
            err = fr.project_view(got, res["rvecs"][v], res["tvecs"][v], objs[v].astype(np.float64)) - imgs[v]
            assert np.sqrt(np.mean(np.sum(err ** 2, axis=1))) == pytest.approx(res["per_view_rms"][v], rel=1e-6, abs=1e-9)
    finally:
        h.close()


def test_calibration_noisy_views_against_the_restated_lm(env, views):
    torch = env["torch"]
    h = make_handle(env)
    try:
        objs, imgs = views["noisy"]
        res = h.fisheye_calibrate(objs, imgs, SIZE)
        got, lm = assert_matches_lm(res, objs, imgs)
        assert 0.3 < res["rms"] < 0.6
        # two calls give the same bits, and device input gives the host input's
        again = h.fisheye_calibrate(objs, imgs, SIZE)
        d_obj = torch.from_numpy(np.concatenate(objs)).cuda()
        d_img = torch.from_numpy(np.concatenate(imgs)).cuda()
        d_n = torch.tensor([len(o) for o in objs], dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        dev = h.fisheye_calibrate_device(d_obj.data_ptr(), d_img.data_ptr(), d_n.data_ptr(), len(objs), SIZE)
        for other in (again, dev):
            for key in ("K", "D", "rvecs", "tvecs", "per_view_rms"):
                assert other[key].tobytes() == res[key].tobytes(), key
            assert other["rms"] == res["rms"]
    finally:
        h.close()


GUESS = (np.array([[225.0, 0, 318.0], [0, 231.0, 241.0], [0, 0, 1]]), np.array([-0.02, 0.0, 0.0, 0.0]))
F = fr.FLAGS
FLAG_CASES = [(F["USE_INTRINSIC_GUESS"], GUESS), (F["FIX_ASPECT_RATIO"], fr.model_of(fr.INTR_TRUE)), (F["FIX_PRINCIPAL_POINT"], None),
              (F["USE_INTRINSIC_GUESS"] | F["FIX_PRINCIPAL_POINT"] | F["FIX_ASPECT_RATIO"], GUESS), (F["FIX_K1"], None), (F["FIX_K2"], None),
              (F["FIX_K3"], None), (F["FIX_K4"], None), (F["USE_INTRINSIC_GUESS"] | F["FIX_K1"] | F["FIX_K2"] | F["FIX_K3"] | F["FIX_K4"], GUESS)]


@pytest.mark.parametrize("flags,model", FLAG_CASES)
def test_calibration_flags(env, views, flags, model):
    h = make_handle(env)
    try:
        objs, imgs = views["noisy"]
        res = h.fisheye_calibrate(objs, imgs, SIZE, flags, model)
        got, lm = assert_matches_lm(res, objs, imgs, flags, model)
        start = fr.calib_start(objs, imgs, SIZE, flags, model)[0]
        if flags & F["FIX_ASPECT_RATIO"]:
            assert abs(got[0] / got[1] - model[0][0, 0] / model[0][1, 1]) < 1e-15
        if flags & F["FIX_PRINCIPAL_POINT"]:
            assert got[2] == start[2] and got[3] == start[3]
        for i, name in enumerate(("FIX_K1", "FIX_K2", "FIX_K3", "FIX_K4")):
            if flags & F[name]:
                assert got[4 + i] == start[4 + i]
    finally:
        h.close()


def host_views_of(markers, ids, obj):
    """what arucohip_fisheye_calibrate_board_batch lays out for a frame: the board markers in list order, corner by corner, the board's
    units scaled to metres as the device scales them"""
    mpp = float(np.float32(fr.MARKER_SIZE)) / 100.0
    o = [(obj[ids.index(int(m["id"]))] * mpp).astype(np.float32) for m in markers if int(m["id"]) in ids]
    i = [np.asarray(m["corners"], np.float32).reshape(4, 2) for m in markers if int(m["id"]) in ids]
    return np.concatenate(o), np.concatenate(i)


def test_calibrate_board_batch_on_a_resident_stream(env):
    capi, ids, obj = env["capi"], env["ids"], env["obj"]
    h = make_handle(env, 4)
    try:
        frames = np.stack([env["frames"][0], env["frames"][1], np.full((fr.H, fr.W), 128, np.uint8), env["frames"][1][::-1, ::-1].copy()])
        markers = h.detect_batch_host(frames)
        assert [len(m) for m in markers[:3]] == [24, 24, 0]
        flags = F["FIX_K3"] | F["FIX_K4"]   # two or three views of a plane do not hold eight intrinsics down
        res = h.fisheye_calibrate_board_batch(4, ids, obj, capi.BOARD_PIX, SIZE, marker_size=fr.MARKER_SIZE, min_markers=20, flags=flags)
        want_used = [len([m for m in ms if int(m["id"]) in ids]) >= 20 for ms in markers]
        assert list(res["used"]) == want_used and want_used[:3] == [True, True, False]
        views_ = [host_views_of(markers[f], ids, obj) for f in range(4) if want_used[f]]
        ref = h.fisheye_calibrate([v[0] for v in views_], [v[1] for v in views_], SIZE, flags)
        for key in ("K", "D", "rvecs", "tvecs"):
            assert res[key].tobytes() == ref[key].tobytes(), key
        assert res["rms"] == ref["rms"] and res["rms"] < 1.5   # LINES corners on curved edges lie about a pixel off
        got = fr.intr_of_result(res)
        assert np.max(np.abs(got[:4] - fr.intr_of(fr.K, fr.D)[:4]) / fr.intr_of(fr.K, fr.D)[:4]) < 0.05
        # no frame qualifies
        with pytest.raises(capi.ArucoHipError) as e:
            h.fisheye_calibrate_board_batch(4, ids, obj, capi.BOARD_PIX, SIZE, marker_size=fr.MARKER_SIZE, min_markers=25)
        assert e.value.code == capi.E_INVALID
        # ideal corners are not the lens's pixels
        h.fisheye_undistort_markers_batch(4, MODEL, KNEW32, cap=0)
        with pytest.raises(capi.ArucoHipError) as e:
            h.fisheye_calibrate_board_batch(4, ids, obj, capi.BOARD_PIX, SIZE, marker_size=fr.MARKER_SIZE, min_markers=20, flags=flags)
        assert e.value.code == capi.E_INVALID
    finally:
        h.close()


def test_calibration_errors(env, views):
    import ctypes as C

    capi = env["capi"]
    h = make_handle(env)
    try:
        objs, imgs = views["clean"]
        bent = [o.copy() for o in objs]
        bent[3][5, 2] = 0.01   # a view that is not planar
        with pytest.raises(capi.ArucoHipError) as e:
            h.fisheye_calibrate(bent, imgs, SIZE)
        assert e.value.code == capi.E_UNSUPPORTED
        with pytest.raises(capi.ArucoHipError) as e:
            h.fisheye_calibrate([objs[0][:3]], [imgs[0][:3]], SIZE)
        assert e.value.code == capi.E_INVALID
        with pytest.raises(capi.ArucoHipError) as e:   # a guess without focal lengths
            h.fisheye_calibrate(objs, imgs, SIZE, F["USE_INTRINSIC_GUESS"], (np.zeros((3, 3)), np.zeros(4)))
        assert e.value.code == capi.E_INVALID
        # every optional output may be NULL
        oa, ia = np.ascontiguousarray(np.concatenate(objs)), np.ascontiguousarray(np.concatenate(imgs))
        npts = np.array([len(o) for o in objs], np.int32)
        m = capi.Fisheye()
        rc = h.L.arucohip_fisheye_calibrate(h.h, oa.ctypes.data_as(C.c_void_p), ia.ctypes.data_as(C.c_void_p), npts.ctypes.data_as(C.c_void_p), len(objs), 0,
                                            fr.W, fr.H, 0, C.byref(m), None, None, None, None)
        assert rc == capi.OK
        full = h.fisheye_calibrate(objs, imgs, SIZE)
        assert np.array_equal(np.array(list(m.K)).reshape(3, 3), full["K"]) and np.array_equal(np.array(list(m.D)), full["D"])
        assert h.L.arucohip_fisheye_calibrate(h.h, oa.ctypes.data_as(C.c_void_p), ia.ctypes.data_as(C.c_void_p), npts.ctypes.data_as(C.c_void_p), len(objs), 0,
                                              fr.W, fr.H, 0, None, None, None, None, None) == capi.E_INVALID
    finally:
        h.close()
