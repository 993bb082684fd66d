"""Camera-native input through the reference-shaped C++ API: tests/cpp/shim_ingest.cpp calls MarkerDetector::detect(const RawFrame&) and
aruco::convertFrame to CV_8UC3 for one Bayer and one NV12 frame; the markers are those of the Python call on ingest_ref's grey conversion of
the same bytes, the B,G,R image is ingest_ref's, byte for byte."""
import os
import subprocess

import numpy as np
import pytest

from tests import ingest_ref as ir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["BAYER_RGGB", "NV12"])
def test_shim_detects_and_converts_a_raw_frame(tmp_path, name):
    import torch  # noqa: F401  (torch's HIP runtime first, see aruco_amd/capi.py)
    from aruco_amd import build_library, capi

    build_library()
    exe = tmp_path / "shim_ingest"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_ingest.cpp"), "-o", str(exe),
                    "-L" + os.path.join(ROOT, "aruco_amd"), "-larucohip", "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(ROOT, "aruco_amd"),
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    rng = np.random.default_rng(11)
    raw = ir.encode(name, ir.scene()[0], rng)
    src, dst = tmp_path / "frame.raw", tmp_path / "frame.bgr"
    src.write_bytes(raw.tobytes())
    r = subprocess.run([str(exe), str(src), str(ir.FORMATS.index(name)), "320", "240", str(dst)], stdout=subprocess.PIPE, text=True, check=True)
    got = [line.split() for line in r.stdout.splitlines() if line.startswith("marker ")]
    h = capi.Handle(320, 240)
    try:
        exp = h.detect(ir.to_gray(name, raw, 320, 240))
    finally:
        h.close()
    assert (name != "NV12" or len(exp) >= 2) and [int(g[1]) for g in got] == [int(m["id"]) for m in exp]
    for g, m in zip(got, exp):
        c = np.array([float(v) for v in g[2:10]], np.float32)   # nine significant digits carry a float exactly
        assert c.tobytes() == np.asarray(m["corners"], np.float32).tobytes()
    assert np.frombuffer(dst.read_bytes(), np.uint8).tobytes() == ir.to_bgr(name, raw, 320, 240).tobytes()
