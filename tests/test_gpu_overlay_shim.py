"""The shim's drawing names (include/aruco_hip_shim.hpp, aruco::DeviceDrawing) through a C++ caller on mock cv::Mat frames."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, name, defines):
    from aruco_amd import build_library

    build_library()
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-DARUCOHIP_USE_OPENCV"] + defines +
                   ["-I" + os.path.join(ROOT, "tests", "cpp", "mock_opencv"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "shim_overlay.cpp"), "-o", str(exe), "-L" + os.path.join(ROOT, "aruco_amd"), "-larucohip",
                    "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(ROOT, "aruco_amd"), "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return str(exe)


@pytest.mark.gpu
def test_shim_drawing_names_paint_the_bytes_of_the_c_call(tmp_path):
    """With ARUCOHIP_SHIM_DEFINE_DRAWING: Marker::draw, CvDrawingUtils::draw3dCube (both forms) / draw3dAxis and the board calls on a mock
    cv::Mat equal arucohip_draw_markers_batch / arucohip_draw_boards_batch with the same arguments, on 3- and 1-channel frames."""
    exe = _build(tmp_path, "shim_overlay", ["-DARUCOHIP_SHIM_DEFINE_DRAWING"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    for what in ("marker_draw_bgr", "marker_draw_gray", "cube", "cube_yperp", "axis", "board"):
        assert lines.count(what + " equal") == (1 if what.startswith("marker_draw") else 2), r.stdout
    assert "DIFFER" not in r.stdout


def test_without_the_macro_the_header_defines_neither_name(tmp_path):
    """The caller's own Marker::draw and aruco::CvDrawingUtils compile, link and are the ones that run (nothing touches the device)."""
    exe = _build(tmp_path, "shim_overlay_own", [])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and "own definitions 11" in r.stdout, r.stdout + r.stderr
