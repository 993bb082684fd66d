"""Both planar pose solutions per marker on the device (arucohip_planar_poses / _batch) against the numpy restatement of the method
(tests/planar_ref.py), the library's own pose path and the shim."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import planar_ref as pr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = pr.MARKER_SIZE
K = pr.K_DEFAULT
# Device against planar_ref on the same float32 corners, refine = 0. The ceiling is the project's pose tolerance (1e-4 relative,
# test_gpu_fullsize); TOL is ten times the largest deviation the first run on an MI355X showed (OBSERVED), the margin for the
# device's normal-equation solves against the reference's SVD / lstsq.
POSE_TOL = 1e-4
OBSERVED = 2.72e-12   # 256 markers without distortion; 1.55e-12 with the five coefficients
TOL = 10 * OBSERVED
assert TOL <= POSE_TOL
NS = (1, 15, 16, 17, 256)   # partial groups of sixteen and partial waves


def _golden_camera():
    from aruco_amd.fixtures import load_case

    gray, doc = load_case("single")
    intr = doc["intrinsics"]
    return gray, np.array(intr["K"], np.float32).reshape(3, 3), np.array(intr["dist"], np.float32)


def _markers(corners):
    from aruco_amd import capi

    c = np.asarray(corners, np.float32).reshape(-1, 8)
    m = np.zeros(len(c), capi.MARKER_DTYPE)
    m["id"] = np.arange(len(c))
    m["corners"] = c
    m["ssize"] = -1
    return m


def _view(out):
    from aruco_amd import capi

    return np.frombuffer(out, capi.PLANAR_DTYPE).copy()


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


@pytest.fixture(scope="module")
def poses():
    """256 generated poses and their float32 corners without distortion; the reference's solutions for them are computed once."""
    R, t, corners = pr.generate_poses(256, seed=977)
    c32 = corners.astype(np.float32)
    ref = [pr.planar_poses(c.astype(np.float64)) for c in c32]
    assert all(r is not None for r in ref)
    return {"R": R, "t": t, "corners": c32, "ref": ref}


@pytest.fixture(scope="module")
def distorted():
    """The same poses seen through the golden camera's five distortion coefficients, scaled to this camera."""
    _, _, dist = _golden_camera()
    R, t, _ = pr.generate_poses(256, seed=977)
    P = pr.object_points()
    c32 = np.array([pr.brown_project(P, Ri, ti, K, dist) for Ri, ti in zip(R, t)]).astype(np.float32)
    ref = [pr.planar_poses(c.astype(np.float64), K, dist) for c in c32]
    assert all(r is not None for r in ref)
    return {"corners": c32, "ref": ref, "dist": dist}


@pytest.fixture(scope="module")
def handle():
    from aruco_amd import capi

    h = capi.Handle(640, 480, max_batch=1, device=0)
    yield h
    h.close()


def _compare(got, ref, tol):
    """Worst deviation of rvec / tvec (relative to the vector's largest entry) and rms (relative to max(rms, 1 px))."""
    worst = 0.0
    for g, r in zip(got, ref):
        assert g["n_solutions"] == 2
        assert g["rms"][0] <= g["rms"][1]
        for j in range(2):
            worst = max(worst, _rel(g["rvec"][j], r["rvec"][j]), _rel(g["tvec"][j], r["tvec"][j]))
            worst = max(worst, abs(g["rms"][j] - r["rms"][j]) / max(r["rms"][j], 1.0))
    print("worst deviation from planar_ref: %.3g (tolerance %.3g)" % (worst, tol))
    assert worst < tol
    return worst


@pytest.mark.parametrize("n", NS)
def test_analytic_solutions_match_the_reference(handle, poses, n):
    got = _view(handle.planar_poses(_markers(poses["corners"][:n]), K, None, SIZE, refine=False))
    assert len(got) == n
    _compare(got, poses["ref"][:n], TOL)


@pytest.mark.parametrize("n", NS)
def test_distorted_camera_matches_the_reference(handle, distorted, n):
    got = _view(handle.planar_poses(_markers(distorted["corners"][:n]), K, distorted["dist"], SIZE, refine=False))
    _compare(got, distorted["ref"][:n], TOL)
    for g, r in zip(got, distorted["ref"][:n]):   # the errors go through the Brown model on both sides
        assert np.all(np.abs(g["rms"] - r["rms"]) <= TOL * np.maximum(r["rms"], 1.0))


def test_refinement_lowers_the_error_and_meets_the_pose_path(handle, poses):
    m = _markers(poses["corners"])
    raw = _view(handle.planar_poses(m, K, None, SIZE, refine=False))
    ref = _view(handle.planar_poses(m, K, None, SIZE, refine=True))
    own = np.concatenate([handle.calculate_extrinsics(m[i:i + 64], K, None, SIZE, y_perp=False) for i in range(0, len(m), 64)])   # a handle of one frame
    worst = 0.0
    rise = float(np.max(ref["rms"] - raw["rms"]))
    print("largest rise of an error under refinement: %.3g px" % rise)
    for b, o in zip(ref, own):
        assert b["n_solutions"] == 2 and b["rms"][0] <= b["rms"][1]
        assert o["has_pose"] == 1
        worst = max(worst, _rel(b["rvec"][0], o["rvec"]), _rel(b["tvec"][0], o["tvec"]))
    print("solution 0 against calculate_extrinsics: worst relative deviation %.3g" % worst)
    assert rise <= 1e-9
    assert worst < POSE_TOL


def test_refinement_with_noisy_corners_stays_ordered_and_finite(handle, poses):
    rng = np.random.default_rng(5)
    noisy = (poses["corners"].astype(np.float64) + rng.normal(0.0, 0.5, poses["corners"].shape)).astype(np.float32)
    got = _view(handle.planar_poses(_markers(noisy), K, None, SIZE, refine=True))
    assert np.all(got["n_solutions"] == 2)
    for name in ("rvec", "tvec", "rms"):
        assert np.all(np.isfinite(got[name]))
    assert np.all(got["rms"][:, 0] <= got["rms"][:, 1])


@pytest.mark.parametrize("refine", (False, True))
def test_degenerate_markers_give_no_solution_and_leave_their_neighbours(handle, poses, refine):
    corners = poses["corners"][:17].copy()
    corners[3] = np.tile([[320.5, 240.25]], (4, 1))                                          # four equal corners
    corners[8] = np.array([[100, 100], [150, 125], [200, 150], [250, 175]], np.float32)       # four corners on one line
    corners[16] = np.array([[300, 200], [380, 260], [380, 260], [300, 200]], np.float32)      # zero area: folded onto a segment
    got = _view(handle.planar_poses(_markers(corners), K, None, SIZE, refine=refine))
    clean = _view(handle.planar_poses(_markers(poses["corners"][:17]), K, None, SIZE, refine=refine))
    for i in range(17):
        if i in (3, 8, 16):
            assert got[i]["n_solutions"] == 0
            assert got[i].tobytes()[:112] == bytes(112)   # every double exactly 0 (no -0, no NaN)
        else:
            assert got[i].tobytes() == clean[i].tobytes()


def test_y_perpendicular_rotates_both_solutions(handle, poses):
    m = _markers(poses["corners"][:17])
    plain = _view(handle.planar_poses(m, K, None, SIZE, refine=False))
    turned = _view(handle.planar_poses(m, K, None, SIZE, refine=False, y_perp=True))
    for a, b in zip(plain, turned):
        assert b["n_solutions"] == 2
        assert a["tvec"].tobytes() == b["tvec"].tobytes() and a["rms"].tobytes() == b["rms"].tobytes()
        for j in range(2):
            assert _rel(b["rvec"][j], pr.rotate_x_axis(a["rvec"][j])) < TOL


def test_argument_checks(handle, poses):
    from aruco_amd import capi

    m = _markers(poses["corners"][:2])
    assert len(handle.planar_poses(m[:0], K, None, SIZE)) == 0
    for kwargs in ({"K": None, "dist": None, "marker_size": SIZE}, {"K": K, "dist": None, "marker_size": 0.0},
                   {"K": K, "dist": np.zeros(3, np.float32), "marker_size": SIZE}):
        with pytest.raises(capi.ArucoHipError) as e:
            handle.planar_poses(m, kwargs["K"], kwargs["dist"], kwargs["marker_size"])
        assert e.value.code == capi.E_INVALID


def _batch_frames():
    """Four 640 x 480 frames, one of them empty."""
    from aruco_amd import synth

    # make_stream scales its markers with the frame: at 640 x 480 they fall below the detector's smallest size, so the sides are set here
    rng = np.random.RandomState(31)
    frames = np.empty((4, 480, 640), np.uint8)
    for f in range(4):
        lay = synth.frame_layout(rng, 640, 480, n_markers=6, side_range=(60, 110), margin=20)
        frames[f] = synth.render_frame(lay, 640, 480, rng).numpy()
    frames[2] = 128
    return frames


@pytest.fixture(scope="module")
def batch():
    """The four frames detected without a pose on a handle of four frames."""
    from aruco_amd import capi

    h = capi.Handle(640, 480, max_batch=4, device=0)
    markers = h.detect_batch_host(_batch_frames())
    yield h, markers
    h.close()


@pytest.mark.parametrize("refine", (False, True))
def test_batch_equals_the_single_call_on_the_returned_markers(batch, refine):
    import torch
    from aruco_amd import capi

    h, markers = batch
    _, Kc, dist = _golden_camera()
    counts = [len(m) for m in markers]
    assert counts[2] == 0 and sum(counts) >= 8 and max(counts) <= 16
    cap = 16
    host = _view(h.planar_poses_batch(4, Kc, dist, 0.05, refine=refine, cap=cap, fill=0xA5))
    dev = torch.full((4 * cap * 120,), 0xA5, dtype=torch.uint8, device="cuda:0")
    h.planar_poses_batch_device(4, C.c_void_p(dev.data_ptr()), cap, Kc, dist, 0.05, refine=refine)
    torch.cuda.synchronize()
    devv = np.frombuffer(dev.cpu().numpy().tobytes(), capi.PLANAR_DTYPE)
    sentinel = bytes([0xA5]) * 120
    for f in range(4):
        single = _view(h.planar_poses(markers[f], Kc, dist, 0.05, refine=refine))
        for out in (host, devv):
            got = out[f * cap:(f + 1) * cap]
            assert got[:counts[f]].tobytes() == single.tobytes()
            assert np.all(got[:counts[f]]["n_solutions"] == 2)
            for e in got[counts[f]:]:
                assert e.tobytes() == sentinel


def test_two_spans_equal_one_span(batch, monkeypatch):
    """The four frames on two chunk workers give the bytes of the one-worker handle, in host and in device memory."""
    import torch
    from aruco_amd import capi

    h1, markers = batch
    _, Kc, dist = _golden_camera()
    cap = 16
    monkeypatch.setenv("ARUCOHIP_STREAMS", "2")
    h2 = capi.Handle(640, 480, max_batch=4, device=0)
    monkeypatch.delenv("ARUCOHIP_STREAMS")
    try:
        assert [m.tobytes() for m in h2.detect_batch_host(_batch_frames())] == [m.tobytes() for m in markers]
        assert h2.batch_chunks() == (2, 2) and h1.batch_chunks() == (1, 4)
        got = []
        for h in (h2, h1):
            host = bytes(h.planar_poses_batch(4, Kc, dist, 0.05, cap=cap, fill=0xA5))
            dev = torch.full((4 * cap * 120,), 0xA5, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            h.planar_poses_batch_device(4, C.c_void_p(dev.data_ptr()), cap, Kc, dist, 0.05)
            torch.cuda.synchronize()
            got.append((host, dev.cpu().numpy().tobytes()))
        assert got[0] == got[1]
        assert got[0][0] == got[0][1]   # entries beyond a frame's markers keep the fill byte in both forms
    finally:
        h2.close()


def test_batch_capacity_and_missing_batch(batch):
    from aruco_amd import capi

    h, markers = batch
    _, Kc, dist = _golden_camera()
    with pytest.raises(capi.ArucoHipError) as e:
        h.planar_poses_batch(4, Kc, dist, 0.05, cap=max(len(m) for m in markers) - 1)
    assert e.value.code == capi.E_CAPACITY
    fresh = capi.Handle(640, 480, max_batch=4, device=0)
    try:
        with pytest.raises(capi.ArucoHipError) as e:
            fresh.planar_poses_batch(1, Kc, dist, 0.05)
        assert e.value.code == capi.E_INVALID
    finally:
        fresh.close()


def test_single_frame_graph_survives_a_planar_call(poses):
    from aruco_amd import capi

    gray, Kc, dist = _golden_camera()
    h = capi.Handle(640, 480, max_batch=1, device=0)
    try:
        seq = [h.detect(gray, K=Kc, dist=dist, marker_size=0.05) for _ in range(3)]
        got = _view(h.planar_poses(_markers(poses["corners"]), K, None, SIZE))
        assert np.all(got["n_solutions"] == 2)
        after = h.detect(gray, K=Kc, dist=dist, marker_size=0.05)
        assert len(after) == 6
        for s in seq:
            assert np.asarray(s).tobytes() == np.asarray(after).tobytes()
    finally:
        h.close()


def build_shim_planar(out):
    from aruco_amd import build_library

    build_library()
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_planar.cpp"),
                    "-o", str(out), "-L" + os.path.join(ROOT, "aruco_amd"), "-larucohip", "-L/opt/rocm/lib",
                    "-Wl,-rpath," + os.path.join(ROOT, "aruco_amd"), "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_shim_calculate_extrinsics_both(tmp_path):
    """Marker::calculateExtrinsicsBoth on the six markers of the golden still: two solutions each, and the marker's own pose (detect with
    a camera) is one of the two refined solutions. Real corners carry noise, so which one is printed, not asserted."""
    _, Kc, dist = _golden_camera()
    exe = tmp_path / "shim_planar"
    build_shim_planar(exe)
    args = [str(exe), os.path.join(ROOT, "tests", "golden", "single.pgm"), "0.05", repr(float(Kc[0, 0])), repr(float(Kc[1, 1])), repr(float(Kc[0, 2])),
            repr(float(Kc[1, 2]))] + [repr(float(d)) for d in dist]
    lines = subprocess.run(args, stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    heads = [i for i, l in enumerate(lines) if l.startswith("marker ")]
    assert len(heads) == 6
    for i in heads:
        w = lines[i].split()
        assert int(w[3]) == 2
        own = np.array(w[5:11], float)
        sols = [np.array(lines[i + 1 + j].split()[2:], float) for j in range(2)]
        dev = [max(_rel(s[1:4], own[:3]), _rel(s[4:7], own[3:])) for s in sols]
        print("marker %s: own pose is solution %d (deviations %.3g, %.3g; rms %.4g, %.4g)" % (w[1], int(np.argmin(dev)), dev[0], dev[1], sols[0][0], sols[1][0]))
        assert sols[0][0] <= sols[1][0]
        assert min(dev) < POSE_TOL
