"""Camera rigs through the reference-shaped C++ API: tests/cpp/shim_rig.cpp (aruco::CameraRig::calibrate and ::detect on rendered frames
detected one by one, and their last-batch overloads on a handle that detected the frames as one batch) against the Python calls on the same
frames. Compiled plain and against the mock OpenCV headers."""
import os
import subprocess

import numpy as np
import pytest

from tests import board3d_ref as b3
from tests.test_gpu_rig import _rendered

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shim_rig_equals_the_c_abi(tmp_path):
    import torch  # noqa: F401  (torch's HIP runtime first, see aruco_amd/capi.py)
    from aruco_amd import build_library, capi

    build_library()
    src = os.path.join(ROOT, "tests", "cpp", "shim_rig.cpp")
    link = ["-L" + os.path.join(ROOT, "aruco_amd"), "-larucohip", "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(ROOT, "aruco_amd"), "-Wl,-rpath,/opt/rocm/lib"]
    exe = tmp_path / "shim_rig"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", str(exe)] + link, check=True)
    mock = subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-DARUCOHIP_USE_OPENCV", "-I" + os.path.join(ROOT, "tests", "cpp", "mock_opencv"),
                           "-I" + os.path.join(ROOT, "include"), src, "-o", str(tmp_path / "shim_rig_cv")] + link, capture_output=True, text=True)
    assert mock.returncode == 0 and "warning" not in mock.stderr, mock.stderr[-3000:]
    ids, obj, frames, cams, _ = _rendered()
    board_txt = tmp_path / "board.txt"
    with open(board_txt, "w") as f:
        for i, q in zip(ids, obj):
            f.write("%d " % i + " ".join("%.9g" % v for v in q.reshape(-1)) + "\n")
    pgms = []
    for i, gray in enumerate(frames):
        pgms.append(str(tmp_path / ("frame%d.pgm" % i)))
        with open(pgms[-1], "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (b3.W, b3.H) + gray.tobytes())
    Kf = b3.K_FRAME
    args = [repr(float(v)) for v in (Kf[0, 0], Kf[1, 1], Kf[0, 2], Kf[1, 2])] + [str(board_txt)] + pgms
    out = subprocess.run([str(exe)] + args, stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    h = capi.Handle(b3.W, b3.H)
    try:
        markers = [h.detect(gray) for gray in frames]
        obs = (np.concatenate([np.full(len(m), f, np.int32) for f, m in enumerate(markers)]), np.concatenate([m["id"] for m in markers]).astype(np.int32),
               np.concatenate([m["corners"] for m in markers]).astype(np.float32).reshape(-1, 8))
        cams4 = [dict(c, dist=np.zeros(4, np.float32)) for c in cams]   # the CameraParameters of the caller hold four zero coefficients
        r = h.rig_calibrate(*obs, 4, cams4, ids, obj, capi.BOARD_METERS)
        p = h.rig_pose(*obs, 4, r["cams"], ids, obj, capi.BOARD_METERS)
    finally:
        h.close()
    h8 = capi.Handle(b3.W, b3.H, max_batch=8)
    try:
        bmarkers = h8.detect_batch_host(frames)
        rb = h8.rig_calibrate_batch(8, cams4, ids, obj, capi.BOARD_METERS)
        pb = h8.rig_pose_batch(8, rb["cams"], ids, obj, capi.BOARD_METERS)
    finally:
        h8.close()

    def rows(tag):
        return {int(l.split()[1]): np.array([float(v) for v in l.split()[2:]]) for l in out if l.startswith(tag + " ")}

    assert out[0] == "views " + " ".join(str(len(m)) for m in markers) and all(len(m) == 6 for m in markers)
    assert "calibrated 1 1" in out and r["calibrated"].all()
    assert float([l for l in out if l.startswith("rms ")][0].split()[1]) == r["rms"]
    cam = rows("cam")
    for c in range(2):
        assert np.array_equal(cam[c], np.concatenate([r["rvecs"][c], r["tvecs"][c]]))
    calib, pose = rows("calib"), rows("pose")
    assert sorted(calib) == sorted(pose) == [0, 1, 2, 3] and r["used"].all()
    for t in range(4):
        assert np.array_equal(calib[t], np.concatenate([r["board_rvecs"][t], r["board_tvecs"][t]]))
        assert p[t]["has_pose"] == 1 and np.array_equal(pose[t], np.concatenate([p[t]["rvec"], p[t]["tvec"]]))
    assert "batch calibrate -215" in out
    # the last-batch overloads on a handle holding the eight frames: the overloads taking the views give the same numbers on the markers
    # read back, and the Python batch forms give them on a batch of their own
    assert "bviews " + " ".join(str(len(m)) for m in bmarkers) in out
    assert "batch equals views 1" in out
    assert float([l for l in out if l.startswith("brms ")][0].split()[1]) == rb["rms"]
    bcam, bcalib, bpose = rows("bcam"), rows("bcalib"), rows("bpose")
    assert rb["calibrated"].all() and rb["used"].all() and sorted(bcalib) == sorted(bpose) == [0, 1, 2, 3]
    for c in range(2):
        assert np.array_equal(bcam[c], np.concatenate([rb["rvecs"][c], rb["tvecs"][c]]))
    for t in range(4):
        assert np.array_equal(bcalib[t], np.concatenate([rb["board_rvecs"][t], rb["board_tvecs"][t]]))
        assert pb[t]["has_pose"] == 1 and np.array_equal(bpose[t], np.concatenate([pb[t]["rvec"], pb[t]["tvec"]]))
