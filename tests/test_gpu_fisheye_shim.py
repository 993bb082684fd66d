"""A fisheye camera through the reference-shaped C++ API: tests/cpp/shim_fisheye.cpp (FisheyeCamera::calibrate, undistortMarkers on the
detector's frame, BoardDetector::detect with the ideal camera, undistortImage) against the Python calls on the same inputs."""
import os
import subprocess

import numpy as np
import pytest

from tests import fisheye_ref as fr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fnv1a(data):
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_shim_fisheye_equals_the_c_abi_and_poses_the_board(tmp_path):
    import torch  # noqa: F401  (torch's HIP runtime first, see aruco_amd/capi.py)
    from aruco_amd import build_library, capi

    build_library()
    exe = tmp_path / "shim_fisheye"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_fisheye.cpp"),
                    "-o", str(exe), "-L" + os.path.join(ROOT, "aruco_amd"), "-larucohip", "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(ROOT, "aruco_amd"),
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    # noise-free views through the lens the frame was rendered with: the calibration ends at that lens
    objs, imgs = fr.make_views(12, intr=fr.intr_of(fr.K, fr.D))
    txt = tmp_path / "views.txt"
    with open(txt, "w") as f:
        f.write("%d\n" % len(objs))
        for o, m in zip(objs, imgs):
            f.write("%d\n" % len(o))
            for p, q in zip(o, m):
                f.write("%.9g %.9g %.9g %.9g %.9g\n" % (p[0], p[1], p[2], q[0], q[1]))
    gray = fr.fisheye_frame(0)
    pgm = tmp_path / "frame.pgm"
    with open(pgm, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (fr.W, fr.H) + gray.tobytes())
    ids, obj = fr.board()
    yml = tmp_path / "board.yml"
    with open(yml, "w") as f:
        f.write("%%YAML:1.0\naruco_bc_nmarkers: %d\naruco_bc_mInfoType: 0\naruco_bc_markers:\n" % len(ids))
        for i, o in zip(ids, obj):
            f.write("   - { id:%d, corners:[ %s ] }\n" % (i, ", ".join("[ %.9g, %.9g, %.9g ]" % tuple(c) for c in o)))
    Kn = fr.KNEW
    args = [repr(float(v)) for v in (fr.MARKER_SIZE, Kn[0, 0], Kn[1, 1], Kn[0, 2], Kn[1, 2])]
    out = subprocess.run([str(exe), str(txt), str(pgm), str(yml)] + args, stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    line = {l.split()[0]: l.split()[1:] for l in out if not l.startswith("marker ")}

    h = capi.Handle(fr.W, fr.H)
    try:
        cal = h.fisheye_calibrate(objs, imgs, (fr.W, fr.H))
        found = h.detect(gray)
        model = (cal["K"], cal["D"])
        ideal, n, dropped = h.fisheye_undistort_markers_batch(1, model, Kn.astype(np.float32))
        b = h.board_detect(ideal[0], ids, obj, capi.BOARD_PIX, K=Kn.astype(np.float32), dist=np.zeros(4, np.float32), marker_size=fr.MARKER_SIZE)
        flat = h.fisheye_undistort(gray, model, Kn.astype(np.float32))
    finally:
        h.close()
    assert float(line["rms"][0]) == cal["rms"]
    assert np.array_equal(np.array([float(v) for v in line["K"]]).reshape(3, 3), cal["K"])
    assert np.array_equal(np.array([float(v) for v in line["D"]]), cal["D"])
    # the calibration found the lens
    got = fr.intr_of(cal["K"], cal["D"])
    want = fr.intr_of(fr.K, fr.D)
    assert np.max(np.abs(got[:4] - want[:4]) / want[:4]) < 1e-5 and np.max(np.abs(got[4:] - want[4:])) < 1e-4
    assert int(line["detected"][0]) == len(found) == 24 and int(line["ideal"][0]) == 24 and dropped[0] == 0
    rows = [l.split() for l in out if l.startswith("marker ")]
    assert [int(r[1]) for r in rows] == [int(m["id"]) for m in ideal[0]]
    assert np.array_equal(np.array([[float(v) for v in r[2:]] for r in rows], np.float32), np.array([m["corners"] for m in ideal[0]], np.float32))
    assert int(line["board"][0]) == 24 and b["has_pose"] == 1
    rv, tv = np.array([float(v) for v in line["Rvec"]]), np.array([float(v) for v in line["Tvec"]])
    assert np.array_equal(rv, b["rvec"]) and np.array_equal(tv, b["tvec"])
    # and the pose is the board's: twice the CPU chain's measured error against the true pose (tests/fisheye_ref.py)
    R = fr.rodrigues(rv).T @ fr.rodrigues(fr.POSES[0][0])
    assert np.arccos(min(1.0, (np.trace(R) - 1) / 2)) <= 2 * fr.CHAIN_MEASURED[0][0]
    assert fr.rel_err(tv, fr.POSES[0][1]) <= 2 * fr.CHAIN_MEASURED[0][1]
    assert int(line["image"][0]) == fnv1a(flat.tobytes())
