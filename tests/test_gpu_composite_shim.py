"""aruco::BoardCompositor (include/aruco_hip_shim.hpp) through a C++ caller on mock cv::Mat frames: the bytes of the C ABI."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_board_compositor_writes_the_bytes_of_the_c_call(tmp_path):
    """setWindow and paint (one frame and the vector form, 3 and 1 channels, a texture with alpha at opacity 200, a mask, a board without a
    pose, which keeps every byte) equal arucohip_rectify_board_window and arucohip_board_composite_batch with the same arguments: the
    tilted board of tests/test_gpu_rectify_shim.py on a 96 x 64 frame, a 70 x 50 texture."""
    from aruco_amd import build_library

    build_library()
    exe = tmp_path / "shim_composite"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-DARUCOHIP_USE_OPENCV", "-I" + os.path.join(ROOT, "tests", "cpp", "mock_opencv"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_composite.cpp"), "-o", str(exe),
                    "-L" + os.path.join(ROOT, "aruco_amd"), "-larucohip", "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(ROOT, "aruco_amd"),
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    for what in ("window", "paint_bgr", "paint_gray", "paint_alpha_bgr", "paint_alpha_gray", "paint_mask_bgr", "paint_mask_gray", "paint_vector_bgr",
                 "paint_vector_gray", "no_pose_bgr", "no_pose_gray"):
        assert lines.count(what + " equal") == 1, r.stdout
    assert "DIFFER" not in r.stdout
