"""The fisheye restatement (tests/fisheye_ref.py) against itself and against the true board pose, on the CPU: what the device tests
(tests/test_gpu_fisheye.py) compare with has to be right first."""
import numpy as np
import pytest

from tests import fisheye_ref as fr

CHAIN_MEASURED = fr.CHAIN_MEASURED   # the CPU chain against the true pose, see tests/fisheye_ref.py
CORNER_MEASURED = [1.1879, 0.9762]   # px, LINES corners against the true fisheye corners
# The frame route (restated remap of the frame to Knew -> oracle detect -> oracle board pose), measured the same way
FRAME_MEASURED = [(2.0914e-3, 2.3838e-3), (7.6286e-4, 2.0638e-3)]


def rotation_between(ra, rb):
    R = fr.rodrigues(ra).T @ fr.rodrigues(rb)
    return float(np.arccos(min(1.0, (np.trace(R) - 1) / 2)))


def test_model_round_trips():
    rng = np.random.RandomState(3)
    th = rng.uniform(0, 1.39, 500)
    phi = rng.uniform(0, 2 * np.pi, 500)
    rays = np.stack([np.sin(th) * np.cos(phi), np.sin(th) * np.sin(phi), np.cos(th)], axis=1) * rng.uniform(0.2, 3, (500, 1))
    px, ang = fr.project(fr.K, fr.D, rays)
    assert np.max(np.abs(ang - th)) < 1e-14
    n, valid, _ = fr.unproject(fr.K, fr.D, px)
    assert valid.all()
    assert np.max(np.abs(n - rays[:, :2] / rays[:, 2:3]) / (1 + np.abs(n))) < 1e-12
    # pixels -> ideal pixels -> pixels
    ideal, valid, _ = fr.undistort_points(px, fr.K, fr.D, fr.KNEW)
    assert valid.all() and np.max(np.abs(fr.distort_points(ideal, fr.K, fr.D, fr.KNEW) - px)) < 1e-9
    # Knew = None is K
    a = fr.undistort_points(px, fr.K, fr.D)[0]
    assert np.array_equal(a, fr.undistort_points(px, fr.K, fr.D, fr.K)[0])


def test_validity_rule():
    # the principal point: theta_d = 0, valid, and its ideal pixel is Knew's principal point
    out, valid, _ = fr.undistort_points([[319.5, 239.5]], fr.K, fr.D, fr.KNEW)
    assert valid[0] and np.array_equal(out[0], [319.5, 239.5])
    # max_angle: <= 0 selects 1.4
    ma = 1.4
    r = fr.theta_d(fr.D, np.array([ma - 1e-6, ma + 1e-6])) * 230
    _, valid, _ = fr.unproject(fr.K, fr.D, np.stack([319.5 + r, [239.5, 239.5]], axis=1), 0.0)
    assert list(valid) == [True, False]
    # a non-monotone theta_d: no root beyond the turning point
    _, valid, margin = fr.unproject(fr.K, fr.D_NOT_MONOTONE, fr.not_monotone_cases(), 1.2)
    assert list(valid) == [True, False, False] and (margin > 1e-9).all()
    out, valid, _ = fr.undistort_points(fr.not_monotone_cases(), fr.K, fr.D_NOT_MONOTONE, fr.KNEW, 1.2)
    assert np.array_equal(out[1:], np.zeros((2, 2)))


def test_point_cases_keep_their_margin():
    """The inputs of the device's point test: every one of them is further than 1e-9 from an edge of the validity rule, and the set
    holds what it was built for."""
    pts, edge_from = fr.point_cases()
    _, valid, margin = fr.unproject(fr.K, fr.D, pts, fr.POINTS_MAX_ANGLE)
    assert (margin > 1e-9).all()
    assert valid.any() and (~valid).any()
    assert list(valid[edge_from:]) == [True, False, True, False]
    assert (margin[edge_from:] < 1e-6).all()   # the near-edge points are near
    assert not valid[edge_from - 3:edge_from].any()   # far beyond
    assert valid[edge_from - 4] and np.array_equal(pts[edge_from - 4], [319.5, 239.5])


def test_map_and_remap():
    """The remap table sends a destination pixel where distort_points sends it, and the fixed-point remap follows a float bilinear
    sample of the source within the weights' rounding."""
    u32, v32, beyond = fr.build_map(fr.W, fr.H, fr.K, fr.D, fr.KNEW, 1.0)
    ys, xs = np.mgrid[0:fr.H:37, 0:fr.W:41]
    want = fr.distort_points(np.stack([xs.ravel(), ys.ravel()], axis=1), fr.K, fr.D, fr.KNEW)
    assert np.allclose(u32[::37, ::41].ravel(), want[:, 0] * 32, rtol=0, atol=1e-9)
    assert np.allclose(v32[::37, ::41].ravel(), want[:, 1] * 32, rtol=0, atol=1e-9)
    # Knew f = 200: tan(1.0) * 200 = 311 px, so the frame's left and right edges lie beyond 1.0 rad and its centre does not
    assert beyond[240, 0] and beyond[240, 639] and not beyond[240, 320] and not beyond[0, 320]
    rng = np.random.RandomState(5)
    ramp = np.add.outer(np.arange(fr.H) * 0.3, np.arange(fr.W) * 0.2) + 20
    img = np.clip(ramp + rng.uniform(-0.4, 0.4, ramp.shape), 0, 255).astype(np.uint8)
    got = fr.remap(img, u32, v32, beyond)
    assert not got[beyond].any()
    u, v = u32 / 32, v32 / 32
    inside = ~beyond & (u >= 0) & (u < fr.W - 1) & (v >= 0) & (v < fr.H - 1)
    x0, y0 = np.floor(np.where(inside, u, 0)).astype(int), np.floor(np.where(inside, v, 0)).astype(int)
    a, b = u - x0, v - y0
    f = img.astype(np.float64)
    flt = (f[y0, x0] * (1 - a) + f[y0, np.minimum(x0 + 1, fr.W - 1)] * a) * (1 - b) + (f[np.minimum(y0 + 1, fr.H - 1), x0] * (1 - a)
                                                                                      + f[np.minimum(y0 + 1, fr.H - 1), np.minimum(x0 + 1, fr.W - 1)] * a) * b
    # 1/32 px of position on a ramp of slope <= 1.3 levels / px, plus the rounding to 8 bits
    assert np.max(np.abs(got.astype(np.float64) - flt)[inside]) <= 0.5 + 1.3 * 2 / 32 + 1e-9
    # three channels are three planes
    img3 = np.stack([img, 255 - img, img // 2], axis=2)
    got3 = fr.remap(img3, u32, v32, beyond)
    assert np.array_equal(got3[..., 0], got) and np.array_equal(got3[..., 2], fr.remap(img // 2, u32, v32, beyond))


def test_calibration_restatement_recovers_the_truth():
    """Noise-free float32 points: start cost 1.8 px rms, the restated Levenberg-Marquardt ends at the truth (measured 1e-8 relative on
    f and c, 3e-8 absolute on D; the float32 rounding of the points is what remains)."""
    objs, imgs = fr.make_views(12)
    p = fr._Problem(objs, imgs, (fr.W, fr.H), 0, None)
    r0 = p.resid(p.x0)
    assert 1.0 < np.sqrt(r0 @ r0 / p.npoints) < 3.0
    lm = fr.lm_calibrate(objs, imgs, (fr.W, fr.H))
    assert lm["iterations"] < 30
    assert np.max(np.abs(lm["intr"][:4] - fr.INTR_TRUE[:4]) / fr.INTR_TRUE[:4]) < 1e-7
    assert np.max(np.abs(lm["intr"][4:] - fr.INTR_TRUE[4:])) < 1e-6 and lm["rms"] < 1e-4


# Distance between the restated LM's end point and scipy's minimum on the noisy views (0.3 px, seed 5), measured here: f and c 9e-11
# relative, k1..k4 (2.1e-11, 2.0e-10, 3.9e-10, 2.1e-10) absolute, rms 2e-15 relative. k2..k4 sit in a flat valley of the cost (they move
# by 1e-2 under this noise), which is why they end further from the minimum than f and c.
LM_TO_SCIPY_K = 3.9e-10


@pytest.mark.parametrize("flags", [0, fr.FLAGS["FIX_K3"] | fr.FLAGS["FIX_K4"], fr.FLAGS["FIX_ASPECT_RATIO"] | fr.FLAGS["FIX_PRINCIPAL_POINT"]])
def test_calibration_restatement_against_scipy(flags):
    objs, imgs = fr.make_views(12, noise=0.3)
    model = fr.model_of(fr.INTR_TRUE) if flags & fr.FLAGS["FIX_ASPECT_RATIO"] else None
    lm = fr.lm_calibrate(objs, imgs, (fr.W, fr.H), flags, model)
    sc = fr.scipy_calibrate(objs, imgs, (fr.W, fr.H), flags, model)
    print("flags %d: f, c %.2e, k %.2e, rms %.2e" % (flags, np.max(np.abs(lm["intr"][:4] - sc["intr"][:4]) / sc["intr"][:4]),
                                                    np.max(np.abs(lm["intr"][4:] - sc["intr"][4:])), abs(lm["rms"] - sc["rms"]) / sc["rms"]))
    assert np.max(np.abs(lm["intr"][:4] - sc["intr"][:4]) / sc["intr"][:4]) < 1e-8
    assert np.max(np.abs(lm["intr"][4:] - sc["intr"][4:])) < 10 * LM_TO_SCIPY_K
    assert abs(lm["rms"] - sc["rms"]) < 1e-10 * sc["rms"]
    assert 0.3 < lm["rms"] < 0.6
    if flags & fr.FLAGS["FIX_K3"]:
        assert lm["intr"][6] == 0 and lm["intr"][7] == 0
    if flags & fr.FLAGS["FIX_ASPECT_RATIO"]:
        assert abs(lm["intr"][0] / lm["intr"][1] - 230.0 / 228.0) < 1e-15 and lm["intr"][2] == 319.5 and lm["intr"][3] == 239.5


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o

    o.build()
    return o


@pytest.mark.parametrize("pose", [0, 1])
def test_cpu_chain_against_the_true_pose(orc, pose):
    ids, obj = fr.board()
    rvec, tvec = fr.POSES[pose]
    markers = orc.Oracle().detect(fr.fisheye_frame(pose))
    assert sorted(m["id"] for m in markers) == sorted(ids)
    truth = fr.true_corners(rvec, tvec)
    corner_err = max(float(np.abs(m["corners"] - truth[ids.index(m["id"])]).max()) for m in markers)
    ideal, dropped, margin = fr.undistort_markers(markers, fr.K, fr.D, fr.KNEW)
    assert dropped == 0 and margin > 1e-9
    b = orc.board_detect(ideal, ids, obj, 0, fr.KNEW, None, fr.MARKER_SIZE)
    rot, tr = rotation_between(b["rvec"], rvec), fr.rel_err(b["tvec"], tvec)
    print("pose %d: corners %.4f px, rotation %.4e rad, translation %.4e" % (pose, corner_err, rot, tr))
    assert b["has_pose"] and b["prob"] == 1.0
    assert corner_err <= 2 * CORNER_MEASURED[pose]
    assert rot <= 2 * CHAIN_MEASURED[pose][0] and tr <= 2 * CHAIN_MEASURED[pose][1]


@pytest.mark.parametrize("pose", [0, 1])
def test_cpu_frame_route_against_the_true_pose(orc, pose):
    """The other route: the frame remapped to the ideal camera first, then an ordinary detection with K = Knew and no distortion."""
    ids, obj = fr.board()
    rvec, tvec = fr.POSES[pose]
    u32, v32, beyond = fr.build_map(fr.W, fr.H, fr.K, fr.D, fr.KNEW)
    markers = orc.Oracle().detect(fr.remap(fr.fisheye_frame(pose), u32, v32, beyond))
    assert sorted(m["id"] for m in markers) == sorted(ids)
    b = orc.board_detect(markers, ids, obj, 0, fr.KNEW, None, fr.MARKER_SIZE)
    rot, tr = rotation_between(b["rvec"], rvec), fr.rel_err(b["tvec"], tvec)
    print("pose %d: rotation %.4e rad, translation %.4e" % (pose, rot, tr))
    assert b["has_pose"] and rot <= 2 * FRAME_MEASURED[pose][0] and tr <= 2 * FRAME_MEASURED[pose][1]


def test_small_max_angle_drops_markers(orc):
    """What the device's drop test relies on: at max_angle = 0.6 both frames lose some markers and keep others, every corner with margin."""
    for pose, want in ((0, 4), (1, 8)):
        markers = orc.Oracle().detect(fr.fisheye_frame(pose))
        ideal, dropped, margin = fr.undistort_markers(markers, fr.K, fr.D, fr.KNEW, 0.6)
        assert dropped == want and len(ideal) == 24 - want and margin > 1e-9
        assert [m["id"] for m in ideal] == [m["id"] for m in markers if m["id"] in {q["id"] for q in ideal}]
