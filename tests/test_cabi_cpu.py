"""CPU-side checks of the drop-in boundary: the library builds for gfx950, loads, and exports exactly the symbols
include/arucohip.h declares; PODs have the documented layout. No compute calls (there is no GPU here)."""
import ctypes as C
import os
import re
import subprocess

from aruco_amd import build_library, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    txt = open(os.path.join(ROOT, "include", "arucohip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(arucohip_[a-z_0-9]+)\s*\(", txt)))


def test_library_builds_and_exports_header_symbols():
    lib = build_library()
    assert os.path.exists(lib)
    out = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    declared = header_symbols()
    assert len(declared) >= 25
    missing = [s for s in declared if s not in exported]
    assert not missing, missing
    assert sorted(capi.SYMBOLS) == declared   # the ctypes binding covers the whole header


def test_library_loads_and_host_only_calls():
    L = capi.load()
    assert L.arucohip_version() == 100
    p = capi.default_params()
    # reference defaults: src/markerdetector.cpp:235-249
    assert (p.thres_method, p.thres_param1, p.thres_param2, p.thres_param1_range) == (capi.THRES_ADPT, 7.0, 7.0, 0)
    assert (p.corner_method, p.warp_size) == (capi.CORNER_LINES, 56)
    assert abs(p.min_size - 0.04) < 1e-7 and abs(p.max_size - 0.5) < 1e-7 and abs(p.border_dist - 0.025) < 1e-7
    lim = capi.Limits()
    L.arucohip_default_limits(C.byref(lim), 1920, 1080, 8)
    assert (lim.max_width, lim.max_height, lim.max_batch) == (1920, 1080, 8)
    assert C.sizeof(capi.Marker) == 96 and capi.MARKER_DTYPE.itemsize == 96
    assert L.arucohip_stage_name(0).decode() == "Threshold" and L.arucohip_kernel_name(0).decode() == "threshold_kernel"


def test_limits_below_one_are_refused_at_creation():
    """A zero would be a list of no entries and a negative value a huge unsigned capacity: arucohip_create_ex checks every limit before it touches
    the device, so this needs none."""
    L = capi.load()
    p = capi.default_params()
    for field in ("triggers_per_frame", "contours_per_frame", "points_per_frame", "candidates_per_frame", "markers_per_frame", "max_batch",
                  "max_thres_planes"):
        for bad in (0, -1, -(1 << 31)):
            lim = capi.Limits()
            L.arucohip_default_limits(C.byref(lim), 640, 480, 2)
            setattr(lim, field, bad)
            h = C.c_void_p(1)
            assert L.arucohip_create_ex(C.byref(p), 0, C.byref(lim), C.byref(h)) == capi.E_INVALID, (field, bad)
            assert not h.value


def test_shim_header_compiles_without_opencv(tmp_path):
    """The C++ shim (reference class API on the C ABI) compiles and links with a plain host compiler."""
    exe = tmp_path / "aruco_simple"
    cmd = ["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "aruco_simple.cpp"), "-o", str(exe),
           "-L" + os.path.join(ROOT, "aruco_amd"), "-larucohip", "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(ROOT, "aruco_amd"),
           "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and "Usage" in r.stderr


def test_shim_opencv_branch_compiles_against_a_mock_opencv(tmp_path):
    """The branch of the shim that is taken when <opencv2/core.hpp> exists (real cv::Mat / cv::InputArray / cv::Exception instead of the
    shim's stand-ins) goes through a compiler: tests/cpp/mock_opencv/opencv2/core.hpp is the builder's own mock of the API shapes that
    branch touches (MatStep, MatExpr from Mat::zeros, _InputArray::getMat, the five-argument cv::Exception). Both the reference-style
    caller tests/cpp/shim_opencv_branch.cpp and tools/aruco_simple.cpp compile warning-free with it and link against the library. What
    this does NOT check: behaviour against a real OpenCV build."""
    inc = ["-I" + os.path.join(ROOT, "tests", "cpp", "mock_opencv"), "-I" + os.path.join(ROOT, "include")]
    link = ["-L" + os.path.join(ROOT, "aruco_amd"), "-larucohip", "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(ROOT, "aruco_amd"), "-Wl,-rpath,/opt/rocm/lib"]
    for src, exe in ((os.path.join(ROOT, "tests", "cpp", "shim_opencv_branch.cpp"), "shim_cv"), (os.path.join(ROOT, "tools", "aruco_simple.cpp"), "simple_cv")):
        out = str(tmp_path / exe)
        r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-DARUCOHIP_USE_OPENCV"] + inc + [src, "-o", out] + link, capture_output=True, text=True)
        assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    r = subprocess.run([str(tmp_path / "shim_cv")], capture_output=True, text=True)
    assert r.returncode == 0 and "OpenCV branch" in r.stderr


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    """No CPU fallback: without libarucohip.so the product raises instead of computing anything (the oracle is test
    infrastructure and is never imported by aruco_amd)."""
    import importlib
    import pytest
    monkeypatch.setattr(capi, "_lib", None)
    monkeypatch.setattr(capi, "library_path", lambda: str(tmp_path / "libarucohip.so"))
    with pytest.raises(capi.ArucoHipError):
        capi.load()
    with pytest.raises(capi.ArucoHipError):
        capi.Handle(640, 480)
    # nothing under aruco_amd/ imports the oracle
    pkg = os.path.join(ROOT, "aruco_amd")
    for name in os.listdir(pkg):
        if name.endswith(".py"):
            assert "oracle" not in open(os.path.join(pkg, name)).read(), name
    csrc = os.path.join(pkg, "csrc")
    for name in os.listdir(csrc):
        if name.endswith((".hip", ".h")):
            txt = open(os.path.join(csrc, name)).read()
            assert "orc.h" not in txt and "liborc" not in txt, name
    importlib.reload(capi)   # leave the module in its normal state for the other tests


def test_headers_are_valid_c99_and_cxx11():
    """The boundary is a C ABI: include/arucohip.h must compile as plain C99 (a cgo / ctypes / C caller includes it) and as C++11, and
    the header-only shim as C++11 (the reference's language level), all warning-free with -Wall -Wextra."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    inc = os.path.join(root, "include")
    runs = [["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(inc, "arucohip.h")],
            ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", os.path.join(inc, "arucohip.h")],
            ["g++", "-std=c++11", "-Wall", "-Wextra", "-fsyntax-only", "-I", inc, "-include", os.path.join(inc, "aruco_hip_shim.hpp"), "-x", "c++", os.devnull]]
    for cmd in runs:
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0 and "warning" not in r.stderr, (cmd, r.stderr[-2000:])


def test_plain_c_caller_links_and_runs_host_only_calls(tmp_path):
    """tests/cpp/c_caller.c is C99 and links against the library like any C / cgo / FFI caller would; without arguments it only
    uses host-side entry points (the GPU form runs in tests/test_gpu_shim.py)."""
    lib = build_library()
    exe = str(tmp_path / "c_caller")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "c_caller.c"),
                    "-o", exe, lib, "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert out.startswith("version 100 thres 1/7/7 corner 3 warp 56 limits 1920x1080x4 marker_bytes 96 mv15 1")


def test_reference_apps_compile_against_the_shim():
    """The drop-in claim on the reference's OWN callers: utils/aruco_simple.cpp (:37-101, config 1 of BASELINE.json) and
    utils/aruco_simple_board.cpp are compiled exactly as they lie in the reference checkout (nothing copied) with "aruco.h" /
    "boarddetector.h" resolving to the shim (tests/cpp/ref_compat/) and OpenCV's core + highgui to the builder's mock headers, then linked
    against libarucohip.so with no-op drawing members (drawing is out of scope). Every detector call those apps make -
    readFromXMLFile, resize, detect with CameraParameters, operator<< of Marker, getThresholdedImage, BoardConfiguration::readFromFile,
    BoardDetector::detect(markers, conf, board, camParams, size) - therefore exists in the shim with a signature their call sites accept.
    The compile is `make -C oracle ref_apps` (run by __graft_entry__.build()): it reads the reference's sources where the checkout exists
    and keeps the binaries under oracle/_ref/, so that a tree built there carries them to machines without it; skipped where neither
    the checkout nor the binaries are present. Run without arguments they print their usage line."""
    import pytest
    build_library()
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "ref_apps"], check=True)
    apps = [os.path.join(ROOT, "oracle", "_ref", app) for app in ("aruco_simple", "aruco_simple_board")]
    if not all(os.path.exists(exe) for exe in apps):
        pytest.skip("no reference checkout, and no oracle/_ref/ binaries built from one")
    for exe in apps:
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and "Usage" in r.stderr


def test_threshold_plan_never_leaves_the_byte_image_out_under_a_strip_kernel(tmp_path):
    """aruco_amd/csrc/thr_plan.h decides, per threshold plane, which kernel family runs and whether the byte image is left out; it is
    plain C++ so that tests/cpp/thr_plan_check.cpp can walk it with the host compiler over widths, strides, alignments, block sizes, C,
    batch sizes and plane counts. The strip kernel stores through the byte image's pointer without a test: a plan that leaves the image
    out while a plane runs that kernel would fault the device, which no GPU test may provoke. The program also checks the conditions of
    the eo / wide kernels, of P16 / FAST, the segment-height rule and when the bitmap pass runs."""
    exe = str(tmp_path / "thr_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "thr_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert " 0 failures" in r.stdout
