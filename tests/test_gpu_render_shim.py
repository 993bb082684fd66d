"""aruco::Mesh and aruco::MeshRenderer (include/aruco_hip_shim.hpp) through a C++ caller on mock cv::Mat frames: the bytes of the C ABI."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_mesh_renderer_writes_the_bytes_of_the_c_call(tmp_path):
    """Mesh::cube() has 8 vertices and 12 outward triangles, Mesh::uvSphere(6, 8) 42 and 80. MeshRenderer::draw on three markers (the
    middle one without a pose) with the default style, with a style of the caller's, a coloured sphere and a mask, and on a board with a
    mask, 3 and 1 channels, equals arucohip_render_markers_batch / arucohip_render_boards_batch with the same arguments on a 96 x 64
    frame; a board without a pose keeps every byte."""
    from aruco_amd import build_library

    build_library()
    exe = tmp_path / "shim_render"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-DARUCOHIP_USE_OPENCV", "-I" + os.path.join(ROOT, "tests", "cpp", "mock_opencv"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_render.cpp"), "-o", str(exe),
                    "-L" + os.path.join(ROOT, "aruco_amd"), "-larucohip", "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(ROOT, "aruco_amd"),
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    for what in ("cube", "sphere", "markers_bgr", "markers_gray", "markers_mask_bgr", "markers_mask_gray", "board_mask_bgr", "board_mask_gray",
                 "no_pose_bgr", "no_pose_gray"):
        assert lines.count(what + " equal") == 1, r.stdout
    assert "DIFFER" not in r.stdout
