"""Camera calibration on the device at its edges (k_calib.hip through arucohip_calibrate_camera and the start-value hook
arucohip_debug_calib_start), against the float64 references that tests/test_calib_edges_cpu.py pins first: the families of
calib_ref.edge_views (point counts around every stride of the kernels from 4 to 512, few points, planes z = z0 != 0, frontal views and
views turned by about pi, one view, two views), flag combinations down to nothing free, a fisheye run of mixed counts, and the error paths
of the start kernels.

Bounds. Intrinsics and rms: the project's own, 1e-6 scaled and 1e-7 relative (test_gpu_calib.assert_matches_scipy). Poses: ten times the
worst distance between two float64 references over the families, measured on the CPU as 5.5e-9 (test_calib_edges_cpu.POSE_SPREAD; the
`small` family with nothing free, where a 4-point view holds its pose weakly), so 5.5e-8 in rotation-matrix entries and in t relative to
its largest entry. Start focal lengths: the reference's DLT by lstsq and by normal equations differ by at most 2.5e-14 relative, a
hundred times that is below the floor, so 1e-9 relative. Costs and per-view rms: 1e-12 relative against float64 recomputed from the
device's own parameters (the order of at most 1024 FP64 terms is the only difference). Start poses: pose_ref.POSE_TOL against the per-view
pose minimum under the start intrinsics, which is what the start (a planar solvePnP per view) aims at.

Measured on one MI355X (the tests print each figure): intrinsics at most 8.6e-9 scaled (fix_k2), rms 7e-15, poses 3.9e-9 (nothing free),
per-view rms 2.5e-13 (small), start fx, fy 1.3e-14, start poses 1.2e-7 (planes), start cost 5e-15, start poses from a guess against the
CPU restatement of solvePnP 8.7e-10, fisheye start poses 3.9e-10."""
import ctypes as C

import numpy as np
import pytest

from tests import calib_ref as cr
from tests import pose_ref
from tests.test_calib_edges_cpu import POSE_SPREAD
from tests.test_gpu_calib import assert_matches_scipy

pytestmark = pytest.mark.gpu

POSE_BOUND = max(10 * POSE_SPREAD, 1e-8)
START_F_BOUND = 1e-9
SUM_BOUND = 1e-12
FAMILIES = tuple(cr.EDGE_COUNTS)
KEYS = ("K", "dist", "rvecs", "tvecs", "per_view_rms")


@pytest.fixture(scope="module")
def handle():
    import torch  # noqa: F401
    from aruco_amd import capi

    h = capi.Handle(640, 480, max_batch=1)
    yield h
    h.close()


def run(h, fam, flags=None, K=None, dist=None):
    if flags is None:
        flags, K, dist = fam["flags"], fam["K"], fam["dist"]
    return h.calibrate_camera(fam["objs"], fam["imgs"], cr.SIZE, flags=flags, K=K, dist=dist)


def assert_poses(got_r, got_t, ref_r, ref_t, bound, what):
    dev = np.array([pose_ref.pose_dev(r, t, r2, t2) for r, t, r2, t2 in zip(got_r, got_t, ref_r, ref_t)])
    print("%s: poses against the reference, worst R %.3g, worst t %.3g (bound %.3g)" % (what, dev[:, 0].max(), dev[:, 1].max(), bound))
    assert dev.max() <= bound, dev


def assert_result(r, fam, ref, what):
    """everything a finished calibration returns, against the reference and against itself"""
    got = cr.intr_of_result(r)
    print("%s: intrinsics %.3g scaled, rms %.3g relative" % (what, cr.scaled_diff(got, ref["intr"]).max(), abs(r["rms"] - ref["rms"]) / ref["rms"]))
    assert_matches_scipy(r, ref)
    assert_poses(r["rvecs"], r["tvecs"], ref["rvecs"], ref["tvecs"], POSE_BOUND, what)
    n = np.array(fam["counts"])
    own = np.array([np.sqrt(cr.view_cost(got, np.concatenate([rv, tv]), o, m) / len(o))
                    for rv, tv, o, m in zip(r["rvecs"], r["tvecs"], fam["objs"], fam["imgs"])])
    print("%s: per-view rms against float64 from the returned parameters %.3g" % (what, np.max(np.abs(r["per_view_rms"] - own) / own)))
    assert np.all(np.abs(r["per_view_rms"] - own) <= SUM_BOUND * own), (r["per_view_rms"], own)
    assert abs(np.sqrt(np.sum(n * r["per_view_rms"] ** 2) / n.sum()) - r["rms"]) < 1e-12 * r["rms"]
    assert r["K"][2, 2] == 1 and r["K"][0, 1] == 0 and r["K"][1, 0] == 0 and r["K"][2, 0] == 0 and r["K"][2, 1] == 0


@pytest.mark.parametrize("name", FAMILIES)
def test_final_result(handle, name):
    """POSE_BOUND is 5.5e-8: ten times the references' own spread, 5.5e-9. Measured here at most 1.2e-9 (small)."""
    fam = cr.edge_views(name)
    r = run(handle, fam)
    assert_result(r, fam, cr.edge_reference(name), name)
    # without the optional outputs: the same bits of K and dist
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    oa, ia = np.ascontiguousarray(np.concatenate(fam["objs"])), np.ascontiguousarray(np.concatenate(fam["imgs"]))
    npts = np.array(fam["counts"], np.int32)
    K = np.zeros(9) if fam["K"] is None else np.array(fam["K"], np.float64).reshape(9)
    d = np.zeros(5) if fam["dist"] is None else np.array(fam["dist"], np.float64)
    rc = handle.L.arucohip_calibrate_camera(handle.h, p(oa), p(ia), p(npts), len(npts), 0, cr.SIZE[0], cr.SIZE[1], fam["flags"], p(K), p(d),
                                            None, None, None, None)
    assert rc == 0 and K.tobytes() == r["K"].tobytes() and d.tobytes() == r["dist"].tobytes()


@pytest.mark.parametrize("name", ["strides", "planes"])
def test_device_resident_input(handle, name):
    import torch

    fam = cr.edge_views(name)
    a = run(handle, fam)
    o = torch.from_numpy(np.concatenate(fam["objs"])).cuda()
    m = torch.from_numpy(np.concatenate(fam["imgs"])).cuda()
    n = torch.tensor(list(fam["counts"]), dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    b = handle.calibrate_camera_device(o.data_ptr(), m.data_ptr(), n.data_ptr(), len(fam["counts"]), cr.SIZE)
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["rms"] == b["rms"]


@pytest.mark.parametrize("name", ["strides", "planes", "poses"])
def test_start_values(handle, name):
    """calib_homography_kernel, calib_focal_kernel, calib_pose_kernel and step 0 of calib_eval_kernel, which the finished calibration
    hides (Levenberg-Marquardt reaches its minimum from a wrong start too). START_F_BOUND is the floor, 1e-9: the reference's own two routes
    differ by 2.5e-14."""
    fam = cr.edge_views(name)
    s = handle.debug_calib_start(fam["objs"], fam["imgs"], cr.SIZE)
    ref, _, ref_poses = cr.start_values(fam["objs"], fam["imgs"], cr.SIZE)
    assert s["err"] == 0
    print("%s: start fx, fy against the reference %s" % (name, np.abs(s["intr"][:2] - ref[:2]) / ref[:2]))
    assert np.all(np.abs(s["intr"][:2] - ref[:2]) <= START_F_BOUND * ref[:2]), (s["intr"], ref)
    assert s["intr"][2] == (cr.SIZE[0] - 1) / 2 and s["intr"][3] == (cr.SIZE[1] - 1) / 2 and np.all(s["intr"][4:] == 0)
    minima = np.array([cr.pose_minimum(o, m, s["intr"], p) for o, m, p in zip(fam["objs"], fam["imgs"], ref_poses)])
    assert_poses(s["poses"][:, :3], s["poses"][:, 3:], minima[:, :3], minima[:, 3:], pose_ref.POSE_TOL, name + " start")
    own = sum(cr.view_cost(s["intr"], p, o, m) for p, o, m in zip(s["poses"], fam["objs"], fam["imgs"]))
    print("%s: start cost %.6g against float64 from the start's own parameters %.3g" % (name, s["cost"], abs(s["cost"] - own) / own))
    assert abs(s["cost"] - own) <= SUM_BOUND * own
    # a guess is the start, bit for bit
    K, dist = cr.ONE_GUESS
    tang = dist + np.array([0, 0, 1e-3, -8e-4, 0])
    g = handle.debug_calib_start(fam["objs"], fam["imgs"], cr.SIZE, flags=cr.FLAGS["USE_INTRINSIC_GUESS"], K=K, dist=tang)
    assert g["err"] == 0 and g["intr"].tobytes() == cr.intr_of(K, tang).tobytes()
    # And the poses are made with it. The reference here is the CPU restatement of solvePnP on the plane moved to z = 0, then moved back
    # (what calib_pose_kernel says it does), not the pose minimum: from a guess 2 % off, solvePnP's own stopping rule (a relative step
    # below FLT_EPSILON) ends 3e-4 beside the minimum on the 96-point view of `planes`, on the CPU as on the device. The guess has no
    # tangential terms, whose derivative the pose solver keeps as the reference's cvProjectPoints2 has it.
    from oracle import orc

    g = handle.debug_calib_start(fam["objs"], fam["imgs"], cr.SIZE, flags=cr.FLAGS["USE_INTRINSIC_GUESS"], K=K, dist=dist)
    assert g["err"] == 0 and g["intr"].tobytes() == cr.intr_of(K, dist).tobytes()
    want = []
    for o, m in zip(fam["objs"], fam["imgs"]):
        flat = o.copy()
        flat[:, 2] = 0
        ok, r, t = orc.solve_pnp(flat, m, K.astype(np.float32).reshape(-1), dist)
        assert ok
        r, t = np.asarray(r, np.float64), np.asarray(t, np.float64)
        want.append(np.concatenate([r, t - float(o[0, 2]) * cr.rodrigues(r)[:, 2]]))
    want = np.array(want)
    assert_poses(g["poses"][:, :3], g["poses"][:, 3:], want[:, :3], want[:, 3:], pose_ref.POSE_TOL, name + " start from a guess")
    own = sum(cr.view_cost(g["intr"], p, o, m) for p, o, m in zip(g["poses"], fam["objs"], fam["imgs"]))
    assert abs(g["cost"] - own) <= SUM_BOUND * own


@pytest.mark.parametrize("case", list(cr.FLAG_CASES))
def test_flags(handle, case):
    flags, K, dist, name = cr.FLAG_CASES[case]
    fam = cr.edge_views(name)
    r = run(handle, fam, flags, K, dist)
    ref = cr.edge_reference(name, flags, K, dist)
    assert_result(r, fam, ref, case)
    got, start = cr.intr_of_result(r), ref["start"]
    fixed = ~cr.free_of(flags)
    if case == "two_free":
        fixed[0] = False   # fx follows fy
        assert abs(got[0] / got[1] - 700.0 / 695.0) < 1e-15 and got[2] == 959.5 and got[3] == 539.5
        assert got[4] != 0 and np.all(got[5:] == 0)
    assert got[fixed].tobytes() == start[fixed].tobytes(), (got, start)   # a fixed entry keeps its start bits
    assert np.all(got[~fixed] != start[~fixed])                           # and a free one moved
    if case == "nothing_free":
        assert got.tobytes() == cr.intr_of(K, dist * np.array([1, 1, 0, 0, 1])).tobytes() and got[6] == 0 and got[7] == 0
        # every view's pose is its own pose-only minimum
        minima = np.array([cr.pose_minimum(o, m, got, np.concatenate([rv, tv]))
                           for o, m, rv, tv in zip(fam["objs"], fam["imgs"], ref["rvecs"], ref["tvecs"])])
        assert_poses(r["rvecs"], r["tvecs"], minima[:, :3], minima[:, 3:], POSE_BOUND, case + " per view")


def test_fisheye_mixed_counts(handle):
    """the fisheye branch of the same kernels at counts below 32, either side of 64 and at 96, by test_gpu_fisheye's rule; its start
    poses against the pose minimum on the points undistorted with the start model (fisheye_ref.calib_start's model of the start)"""
    from tests import fisheye_ref as fr
    from tests.test_gpu_fisheye import SIZE, assert_matches_lm

    objs, imgs = fr.mixed_views()
    res = handle.fisheye_calibrate(objs, imgs, SIZE)
    assert_matches_lm(res, objs, imgs)
    s = handle.debug_calib_start(objs, imgs, SIZE, fisheye=True)
    intr, _, ref_poses = fr.calib_start(objs, imgs, SIZE)
    assert s["err"] == 0 and s["intr"][:8].tobytes() == intr.tobytes() and s["intr"][8] == 0
    identity = np.array([1.0, 1, 0, 0, 0, 0, 0, 0, 0])
    minima = np.array([cr.pose_minimum(o, fr.start_points(intr, m).astype(np.float32), identity, p) for o, m, p in zip(objs, imgs, ref_poses)])
    assert_poses(s["poses"][:, :3], s["poses"][:, 3:], minima[:, :3], minima[:, 3:], pose_ref.POSE_TOL, "fisheye start")


# ---- the error paths of the start kernels
def broken_views(kind):
    """`planes` with one view spoilt: (objs, imgs). Counts 33, 40, 65, 96, ...: view 3 has 96 points, view 2 has 65."""
    fam = cr.edge_views("planes")
    objs, imgs = [o.copy() for o in fam["objs"]], [m.copy() for m in fam["imgs"]]
    if kind == "nonplanar_95_of_96":     # the last lane of the second pass over the view's points
        objs[3][95, 2] += 0.01
    elif kind == "nonplanar_64_of_65":   # the only point of the second pass
        objs[2][64, 2] += 0.01
    elif kind == "collinear":            # a row of the grid: Y is one float, its mean absolute deviation is exactly 0
        objs[0][:, :2] = cr.planar_grid(33, 1, 0.009)[:, :2]
        imgs[0][:, 1] = imgs[0][0, 1] + 0.3 * (imgs[0][:, 0] - imgs[0][0, 0])
    elif kind == "identical":
        objs[0][:] = objs[0][0]
        imgs[0][:] = imgs[0][0]
    elif kind == "nan":
        imgs[1][17, 0] = np.nan
    return objs, imgs


@pytest.fixture(scope="module")
def fresh_planes():
    import torch  # noqa: F401
    from aruco_amd import capi

    h = capi.Handle(640, 480, max_batch=1)
    try:
        return run(h, cr.edge_views("planes"))
    finally:
        h.close()


def assert_handle_still_calibrates(handle, fresh_planes):
    again = run(handle, cr.edge_views("planes"))
    for k in KEYS:
        assert again[k].tobytes() == fresh_planes[k].tobytes(), k
    assert again["rms"] == fresh_planes["rms"]


@pytest.mark.parametrize("kind,code,bit", [("nonplanar_95_of_96", "E_UNSUPPORTED", 2), ("nonplanar_64_of_65", "E_UNSUPPORTED", 2),
                                           ("collinear", "E_INVALID", 1), ("identical", "E_INVALID", 1), ("nan", "E_INVALID", 1)])
def test_start_errors(handle, fresh_planes, kind, code, bit):
    """Without a guess. Non-planar: calib_pose_kernel's s_bad, whichever pass and lane sees the point. Collinear along a grid row and
    identical points: calib_homography_kernel's spread test (the mean absolute deviation of equal floats is exactly 0). NaN: the same test,
    which a NaN spread fails. The hook reports the same condition as a bit."""
    from aruco_amd import capi

    objs, imgs = broken_views(kind)
    with pytest.raises(capi.ArucoHipError) as e:
        handle.calibrate_camera(objs, imgs, cr.SIZE)
    assert e.value.code == getattr(capi, code)
    assert handle.debug_calib_start(objs, imgs, cr.SIZE)["err"] & bit
    assert_handle_still_calibrates(handle, fresh_planes)


@pytest.mark.parametrize("kind", ["nonplanar_95_of_96", "nan", "collinear", "identical"])
def test_start_errors_with_a_guess(handle, fresh_planes, kind):
    """With USE_INTRINSIC_GUESS only calib_pose_kernel makes start values. Every loop of solve_pnp_planar_wave is counted (20 outer
    rounds, lambda up to 1e16 inside, 5 rounds in undistort_point), so each of these ends. A point off the plane is E_UNSUPPORTED as
    before. A NaN coordinate makes the start cost NaN: E_INVALID. Collinear or identical points have no homography, the pose search starts
    at zero and project_point guards z = 0, so the start cost is finite and the run is not refused: all that is asked of it is that it ends,
    with ARUCOHIP_OK or E_INVALID, and leaves the handle as it was."""
    from aruco_amd import capi

    objs, imgs = broken_views(kind)
    K, dist = cr.ONE_GUESS
    code = None
    try:
        handle.calibrate_camera(objs, imgs, cr.SIZE, flags=cr.FLAGS["USE_INTRINSIC_GUESS"], K=K, dist=dist)
    except capi.ArucoHipError as e:
        code = e.code
    if kind == "nonplanar_95_of_96":
        assert code == capi.E_UNSUPPORTED
    elif kind == "nan":
        assert code == capi.E_INVALID
    else:
        assert code in (None, capi.E_INVALID)
    assert_handle_still_calibrates(handle, fresh_planes)
