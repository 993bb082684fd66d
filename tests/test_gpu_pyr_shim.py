"""MarkerDetector::pyrDown(level) through the reference-shaped C++ API: tests/cpp/shim_pyr.cpp against the Python call on the same frame."""
import os
import subprocess

import numpy as np
import pytest

from tests import pyr_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shim_pyr_down_equals_the_python_call(tmp_path):
    import torch  # noqa: F401  (torch's HIP runtime first, see aruco_amd/capi.py)
    from aruco_amd import build_library, capi

    build_library()
    exe = tmp_path / "shim_pyr"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_pyr.cpp"), "-o", str(exe),
                    "-L" + os.path.join(ROOT, "aruco_amd"), "-larucohip", "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(ROOT, "aruco_amd"),
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    frames, truth = pyr_ref.frames_of("640x480")
    pgm = tmp_path / "frame.pgm"
    with open(pgm, "wb") as f:
        f.write(b"P5\n640 480\n255\n" + frames[0].tobytes())
    r = subprocess.run([str(exe), str(pgm), "1"], stdout=subprocess.PIPE, text=True, check=True)
    got = [line.split() for line in r.stdout.splitlines() if line.startswith("marker ")]
    h = capi.Handle(640, 480)
    try:
        h.set_pyr_down(1)
        exp = h.detect(frames[0])
    finally:
        h.close()
    assert [int(g[1]) for g in got] == [int(m["id"]) for m in exp] == truth[0]
    for g, m in zip(got, exp):
        c = np.array([float(v) for v in g[2:10]], np.float32)   # nine significant digits carry a float exactly
        assert c.tobytes() == np.asarray(m["corners"], np.float32).tobytes()
    assert "thres 320 240" in r.stdout.splitlines()
