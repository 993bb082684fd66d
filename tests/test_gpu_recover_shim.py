"""BoardDetector::recoverMarkers through the reference-shaped C++ API: tests/cpp/shim_recover.cpp against the Python call on the same frame."""
import os
import subprocess

import numpy as np
import pytest

from tests import recover_ref as rr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shim_recover_markers_equals_the_python_call(tmp_path):
    import torch  # noqa: F401  (torch's HIP runtime first, see aruco_amd/capi.py)
    from aruco_amd import build_library, capi

    build_library()
    exe = tmp_path / "shim_recover"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_recover.cpp"), "-o", str(exe),
                    "-L" + os.path.join(ROOT, "aruco_amd"), "-larucohip", "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(ROOT, "aruco_amd"),
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    ids, obj = rr.board12()
    gray, _ = rr.build_frame(ids, obj, {1: [(3, 3)], 6: [(2, 2), (4, 3)], 10: [(1, 1), (1, 4), (2, 3), (3, 2), (4, 5), (5, 3)]})
    pgm = tmp_path / "frame.pgm"
    with open(pgm, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (rr.W, rr.H) + gray.tobytes())
    board = tmp_path / "board.txt"
    with open(board, "w") as f:
        f.write("%d\n" % len(ids))
        for i, o in zip(ids, obj):
            f.write("%d %s\n" % (i, " ".join(repr(float(v)) for v in o.reshape(-1))))
    r = subprocess.run([str(exe), str(pgm), str(board), "600", "600", "320", "240", repr(rr.MARKER_SIZE)], stdout=subprocess.PIPE, text=True, check=True)
    lines = r.stdout.splitlines()
    h = capi.Handle(rr.W, rr.H)
    try:
        K = rr.K.astype(np.float32)
        m = h.detect(gray, K=K, marker_size=rr.MARKER_SIZE)
        out, n, rec, boards = h.board_recover_batch(1, ids, obj, rr.PIX, K, dist=np.zeros(4, np.float32), marker_size=rr.MARKER_SIZE)
    finally:
        h.close()
    assert "detected %d" % len(m) in lines and len(m) == 9
    assert "recovered %d" % rec[0] in lines and rec[0] == 2
    assert [int(l.split()[1]) for l in lines if l.startswith("marker ")] == [int(x["id"]) for x in out[0]]
    assert "board %d" % boards[0]["n_markers"] in lines and boards[0]["n_markers"] == 11
