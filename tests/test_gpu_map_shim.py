"""Marker mapping through the reference-shaped C++ API: tests/cpp/shim_map.cpp (BoardDetector::mapBoard, then BoardDetector::detect with
the BoardConfiguration it returned) against the Python calls on the same observations."""
import os
import subprocess

import numpy as np
import pytest

from tests import board3d_ref as b3
from tests import map_ref as mr
from tests import pose_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shim_map_equals_the_c_abi_and_feeds_board_detect(tmp_path):
    import torch  # noqa: F401  (torch's HIP runtime first, see aruco_amd/capi.py)
    from aruco_amd import build_library, capi

    build_library()
    exe = tmp_path / "shim_map"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_map.cpp"),
                    "-o", str(exe), "-L" + os.path.join(ROOT, "aruco_amd"), "-larucohip", "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(ROOT, "aruco_amd"),
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    c = mr.case("cube", pose_ref.NOISE, 1)
    sc = c["scene"]
    fr, ids, cs = c["obs"]
    frame = int(np.nonzero(np.bincount(fr, minlength=c["nframes"]) == 3)[0][0])
    txt = tmp_path / "observations.txt"
    with open(txt, "w") as f:
        f.write("%d %d\n%s\n" % (c["nframes"], len(sc["ids"]), " ".join(str(int(i)) for i in sc["ids"])))
        for a, b, q in zip(fr, ids, cs):
            f.write("%d %d %s\n" % (a, b, " ".join("%.9g" % v for v in q)))
    Kc, d = sc["K"], sc["dist"]
    args = [repr(float(v)) for v in (mr.SIZE, Kc[0, 0], Kc[1, 1], Kc[0, 2], Kc[1, 2], *d)]
    # the batch overload: one rendered frame of the folded board, detected by the board detector's own MarkerDetector
    board = b3.fold(12, 90.0)
    gray = b3.render(board, *b3.frame_pose(1)[:2], seed=6)
    pgm = tmp_path / "frame.pgm"
    with open(pgm, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (b3.W, b3.H) + gray.tobytes())
    Kf = b3.K_FRAME
    args += [str(pgm)] + [repr(float(v)) for v in (Kf[0, 0], Kf[1, 1], Kf[0, 2], Kf[1, 2])] + [str(int(board[0][0])), str(len(board[0]))]
    out = subprocess.run([str(exe), str(txt), str(frame)] + args, stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    h = capi.Handle(mr.W, mr.H)
    try:
        found = h.detect(gray, K=Kf.astype(np.float32), dist=np.zeros(4, np.float32))
        last = h.board_map_batch(1, board[0], Kf, np.zeros(4), mr.SIZE)
        r = h.board_map(fr, ids, cs, c["nframes"], sc["ids"], Kc, d, mr.SIZE)
        m = np.zeros(3, capi.MARKER_DTYPE)
        m["id"], m["corners"] = ids[fr == frame], cs[fr == frame]
        b = h.board_detect(m, sc["ids"], r["obj"], capi.BOARD_METERS, K=Kc, dist=d, marker_size=mr.SIZE)
    finally:
        h.close()
    assert out[0] == "mapped 1 1 1 1 1 1" and "info 1" in out and "board 3" in out
    assert float(out[1].split()[1]) == r["rms"]
    rows = [l.split() for l in out if l.startswith("obj ")]
    assert [int(x[1]) for x in rows] == [int(i) for i in sc["ids"]]
    obj = np.array([[float(v) for v in x[2:]] for x in rows], np.float32).reshape(-1, 4, 3)
    assert np.array_equal(obj, r["obj"])
    rv = np.array([float(x) for x in [l for l in out if l.startswith("Rvec ")][0].split()[1:]])
    tv = np.array([float(x) for x in [l for l in out if l.startswith("Tvec ")][0].split()[1:]])
    assert b["has_pose"] == 1 and np.array_equal(rv, b["rvec"]) and np.array_equal(tv, b["tvec"])
    assert max(pose_ref.pose_dev(rv, tv, r["frame_rvecs"][frame], r["frame_tvecs"][frame])) < pose_ref.POSE_TOL
    assert "last detected %d" % len(found) in out and len(found) == 12
    assert "last mapped" + " 1" * 12 in out and last["mapped"].all()
    assert float([l for l in out if l.startswith("last rms ")][0].split()[2]) == last["rms"]
    rows = [l.split() for l in out if l.startswith("last obj ")]
    assert [int(x[2]) for x in rows] == [int(i) for i in board[0]]
    assert np.array_equal(np.array([[float(v) for v in x[3:]] for x in rows], np.float32).reshape(-1, 4, 3), last["obj"])
