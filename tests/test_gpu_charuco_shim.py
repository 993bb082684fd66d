"""aruco::CharucoBoard through the reference-shaped C++ API: tests/cpp/shim_charuco.cpp (paint, detect, detectCorners, estimatePose) against the
C ABI's bytes for the same frame."""
import os
import subprocess

import numpy as np
import pytest

from tests import charuco_ref as cr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fnv1a(img):
    h = 1469598103934665603
    for v in img.reshape(-1).tolist():
        h = ((h ^ v) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_shim_charuco_board_equals_the_c_abi(tmp_path):
    import torch  # noqa: F401  (torch's HIP runtime first, see aruco_amd/capi.py)
    from aruco_amd import build_library, capi

    build_library()
    exe = tmp_path / "shim_charuco"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_charuco.cpp"), "-o", str(exe),
                    "-L" + os.path.join(ROOT, "aruco_amd"), "-larucohip", "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(ROOT, "aruco_amd"),
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    L, square = cr.LAYOUT, 0.1
    r = subprocess.run([str(exe)] + [str(v) for v in L] + [repr(square)] + [str(i) for i in cr.IDS], stdout=subprocess.PIPE, text=True, check=True)
    out = dict(line.split(" ", 1) if " " in line else (line, "") for line in r.stdout.splitlines())
    h = capi.Handle(cr.W, cr.H)
    try:
        lay = capi.charuco_layout(L[:2], L[2], L[3])
        img, _, _ = h.charuco_board_image(lay, cr.IDS, centered=True)
        frame = np.full((cr.H, cr.W), 255, np.uint8)
        frame[40:440, 70:570] = img
        m = h.detect(frame)
        rec, nf = h.charuco_corners_batch(lay, cr.IDS, frame[None])
        pose = h.charuco_pose_batch(1, cr.K.astype(np.float32), dist=np.zeros(4, np.float32), square_size=square)
    finally:
        h.close()
    assert np.array_equal(img, cr.board_image(L, cr.IDS))
    assert out["size"] == "500 400" and out["image"] == "%016x" % fnv1a(img)
    assert out["markers"] == "%d" % len(m) and len(m) == 10
    assert out["found"] == "%d" % nf[0] and nf[0] == 12
    assert out["records"] == rec.tobytes().hex()
    assert out["ids"].split() == [str(c) for c in range(12)]
    assert out["has_pose"] == "1" and pose[0]["has_pose"] == 1 and out["pose"] == pose.tobytes().hex()
