"""Frames out through the reference-shaped C++ API: tests/cpp/shim_egress.cpp calls aruco::exportFrame on one B,G,R frame for NV12 and for
RGBA. The bytes are egress_ref's; MarkerDetector::detect on the NV12 view finds the markers of the Python call on egress_ref's Y plane;
a Bayer destination throws (the program's exit status)."""
import os
import subprocess

import numpy as np
import pytest

from tests import egress_ref as er
from tests import ingest_ref as ir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shim_exports_a_frame_and_detects_on_its_nv12_view(tmp_path):
    import torch  # noqa: F401  (torch's HIP runtime first, see aruco_amd/capi.py)
    from aruco_amd import build_library, capi

    build_library()
    exe = tmp_path / "shim_egress"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_egress.cpp"), "-o", str(exe),
                    "-L" + os.path.join(ROOT, "aruco_amd"), "-larucohip", "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(ROOT, "aruco_amd"),
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    g = ir.scene()[0]
    bgr = np.stack([(g.astype(np.uint16) * 3 // 4).astype(np.uint8), g, 255 - (255 - g) // 2], axis=-1)   # the three channels differ
    src, nv12, rgba = tmp_path / "frame.bgr", tmp_path / "frame.nv12", tmp_path / "frame.rgba"
    src.write_bytes(bgr.tobytes())
    r = subprocess.run([str(exe), str(src), "320", "240", str(nv12), str(rgba)], stdout=subprocess.PIPE, text=True, check=True)
    assert nv12.read_bytes() == er.export_raw("NV12", bgr).tobytes()
    assert rgba.read_bytes() == er.export_raw("RGBA8", bgr).tobytes()
    got = [line.split() for line in r.stdout.splitlines() if line.startswith("marker ")]
    h = capi.Handle(320, 240)
    try:
        exp = h.detect(er.export("NV12", bgr)[0])
    finally:
        h.close()
    assert len(exp) >= 2 and [int(g[1]) for g in got] == [int(m["id"]) for m in exp]
    for g, m in zip(got, exp):
        c = np.array([float(v) for v in g[2:10]], np.float32)   # nine significant digits carry a float exactly
        assert c.tobytes() == np.asarray(m["corners"], np.float32).tobytes()
