"""A folded board through the reference-shaped C++ API: tests/cpp/shim_board3d.cpp (BoardConfiguration::readFromFile of a METERS file with
non-zero z, MarkerDetector::detect, BoardDetector::detect) against the Python calls on the same frame."""
import os
import subprocess

import numpy as np
import pytest

from tests import board3d_ref as b3
from tests import pose_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shim_board_pose_of_a_fold_equals_the_python_call(tmp_path):
    import torch  # noqa: F401  (torch's HIP runtime first, see aruco_amd/capi.py)
    from aruco_amd import build_library, capi

    build_library()
    exe = tmp_path / "shim_board3d"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_board3d.cpp"), "-o", str(exe),
                    "-L" + os.path.join(ROOT, "aruco_amd"), "-larucohip", "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(ROOT, "aruco_amd"),
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    board = b3.fold(12, 90.0)
    ids, obj = board[0], board[1]
    rvec, tvec, R = b3.frame_pose(1)
    gray = b3.render(board, rvec, tvec, seed=6)
    pgm = tmp_path / "frame.pgm"
    with open(pgm, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (b3.W, b3.H) + gray.tobytes())
    yml = tmp_path / "fold.yml"
    with open(yml, "w") as f:
        f.write("%%YAML:1.0\naruco_bc_nmarkers: %d\naruco_bc_mInfoType: 1\naruco_bc_markers:\n" % len(ids))
        for i, o in zip(ids, obj):
            f.write("   - { id:%d, corners:[ %s ] }\n" % (i, ", ".join("[ %s ]" % ", ".join("%.9g" % v for v in c) for c in o)))
    Kf = b3.K_FRAME
    r = subprocess.run([str(exe), str(pgm), str(yml), repr(float(Kf[0, 0])), repr(float(Kf[1, 1])), repr(float(Kf[0, 2])), repr(float(Kf[1, 2]))], stdout=subprocess.PIPE, text=True, check=True)
    lines = r.stdout.splitlines()
    h = capi.Handle(b3.W, b3.H)
    try:
        KF = Kf.astype(np.float32)
        m = h.detect(gray, K=KF, dist=np.zeros(4, np.float32))
        got = h.board_detect(m, ids, obj, 1, K=KF, dist=np.zeros(4, np.float32))
    finally:
        h.close()
    assert "detected %d" % len(m) in lines and len(m) == 12
    assert "board 12" in lines and "prob 1" in lines and got["has_pose"] == 1
    rv = np.array([float(x) for x in [l for l in lines if l.startswith("Rvec ")][0].split()[1:]])
    tv = np.array([float(x) for x in [l for l in lines if l.startswith("Tvec ")][0].split()[1:]])
    assert np.array_equal(rv, got["rvec"]) and np.array_equal(tv, got["tvec"])
    d = pose_ref.pose_dev(rv, tv, R, tvec)
    print("shim pose against the painted pose: R %.3g t %.3g" % d)
