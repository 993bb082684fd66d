"""Two planar pose solutions per marker, the parts that need no GPU: the numpy reference (tests/planar_ref.py) recovers the true pose
from exact corners, and the C ABI carries the new structure and entry points."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import planar_ref as pr

N_POSES = 2000


@pytest.fixture(scope="module")
def solved():
    R, t, corners = pr.generate_poses(N_POSES)
    return R, t, [pr.planar_poses(c) for c in corners]


def test_reference_solves_every_pose(solved):
    assert all(s is not None for s in solved[2])


def test_first_solution_is_the_truth(solved):
    """Exact float64 corners: the solution with the smaller error is the pose that made them, R within 1e-9 per entry and t within
    1e-9 relative."""
    R, t, sols = solved
    worst_R = worst_t = 0.0
    for Ri, ti, s in zip(R, t, sols):
        worst_R = max(worst_R, np.max(np.abs(s["R"][0] - Ri)))
        worst_t = max(worst_t, np.max(np.abs(s["tvec"][0] - ti)) / np.max(np.abs(ti)))
    print("worst |dR| %.3g, worst relative |dt| %.3g" % (worst_R, worst_t))
    assert worst_R < 1e-9 and worst_t < 1e-9


def test_both_solutions_are_rotations_in_front_of_the_camera(solved):
    worst = 0.0
    for s in solved[2]:
        for j in range(2):
            Rj = s["R"][j]
            worst = max(worst, np.max(np.abs(Rj.T @ Rj - np.eye(3))), abs(np.linalg.det(Rj) - 1.0))
            assert s["tvec"][j][2] > 0
        assert s["rms"][0] <= s["rms"][1]
    print("worst orthonormality / determinant error %.3g" % worst)
    assert worst < 1e-9


def test_rvec_round_trip(solved):
    for s in solved[2][:200]:
        for j in range(2):
            assert np.max(np.abs(pr.rodrigues(s["rvec"][j]) - s["R"][j])) < 1e-9


def test_structure_is_120_bytes():
    from aruco_amd import capi

    assert C.sizeof(capi.PlanarPoses) == 120 and capi.PLANAR_DTYPE.itemsize == 120
    assert capi.PlanarPoses.rms.offset == 96 and capi.PlanarPoses.n_solutions.offset == 112
    assert capi.PLANAR_DTYPE.fields["tvec"][1] == 48


def test_header_declares_and_library_exports_the_entry_points():
    from aruco_amd import capi
    from aruco_amd.build import library_path

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "arucohip.h")).read()
    for name in ("arucohip_planar_poses", "arucohip_planar_poses_batch"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi.SYMBOLS
    assert "arucohip_planar_poses_t" in header
    lib = library_path()
    if not os.path.exists(lib):
        pytest.fail("libarucohip.so is not built")
    exported = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
    names = set(line.split()[-1] for line in exported.splitlines() if line.strip())
    assert {"arucohip_planar_poses", "arucohip_planar_poses_batch"} <= names
