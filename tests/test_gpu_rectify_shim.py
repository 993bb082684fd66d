"""aruco::BoardRectifier (include/aruco_hip_shim.hpp) through a C++ caller on mock cv::Mat frames: the bytes of the C ABI."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_board_rectifier_writes_the_bytes_of_the_c_call(tmp_path):
    """setWindow, rectify (one frame and the vector form, 3 and 1 channels, a board without a pose) and warpPerspectiveInverse equal
    arucohip_rectify_board_window, arucohip_board_rectify_batch and arucohip_warp_plane_batch with the same arguments: the tilted board
    and the perspective map of tests/test_gpu_rectify.py's cases, on a 96 x 64 frame."""
    from aruco_amd import build_library

    build_library()
    exe = tmp_path / "shim_rectify"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-DARUCOHIP_USE_OPENCV", "-I" + os.path.join(ROOT, "tests", "cpp", "mock_opencv"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_rectify.cpp"), "-o", str(exe),
                    "-L" + os.path.join(ROOT, "aruco_amd"), "-larucohip", "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(ROOT, "aruco_amd"),
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    for what in ("window", "rectify_bgr", "rectify_gray", "rectify_vector_bgr", "rectify_vector_gray", "no_pose_bgr", "no_pose_gray", "warp_bgr", "warp_gray"):
        assert lines.count(what + " equal") == 1, r.stdout
    assert "DIFFER" not in r.stdout
