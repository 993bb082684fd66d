"""The reference side of the pose edge tests, pinned before the device is compared with it: the CPU restatement of solvePnP(ITERATIVE)
(oracle/orc_pnp.cpp) on the families of tests/pose_ref.py, against the generating poses and against a polished float64 minimum.
The convergence mask computed here (pose_ref.reference_side, cached per process) is what a comparison of the device solver with the
same oracle results has to leave out, and no more."""
import numpy as np
import pytest

from tests import pose_ref as ref

MAX_UNCONVERGED = 2   # of 48: at most 5 % of a family may be left out of a device comparison


def side(name, noise):
    from oracle import orc

    return ref.reference_side(name, noise, orc.solve_pnp)


def test_generated_corners_are_the_projection_of_their_pose():
    """The families themselves: float32 corners within float rounding of the projection of the generating pose, markers of the sizes
    the family names, the rational terms present in dist8."""
    P = ref.object_points(ref.MARKER_SIZE)
    for name, noise in ref.NOISE_FREE:
        fam = ref.family(name, noise)
        assert fam["corners"].shape == (ref.N_CASES, 4, 2) and fam["corners"].dtype == np.float32
        for R, t, c in zip(fam["R"], fam["t"], fam["corners"]):
            assert abs(np.linalg.det(R) - 1.0) < 1e-12
            assert np.all(P @ R[2] + t[2] > 0)   # in front of the camera
            assert np.max(np.abs(ref.brown_project(P, R, t, fam["K"], fam["dist"]) - c)) < 2.5e-4   # half an ulp of a float at 4096 px
    far = ref.family("far")["corners"]
    # a frontal side is 0.05 m * 1400 / z = 8.75 .. 17.5 px; a tilt of up to 1.0 rad about an axis at 45 degrees to the sides shortens both
    # of them, to sqrt((1 + cos(1.0)^2) / 2) = 0.80 at the least, so the larger side of every marker lies in 7.0 .. 17.5 px (plus perspective)
    side_px = np.linalg.norm(far - np.roll(far, 1, axis=1), axis=2).max(axis=1)
    assert side_px.min() > 7.0 and side_px.max() < 18.0
    assert 9.0 < np.median(side_px) < 17.0
    assert len(ref.FAMILIES["dist8"][2]) == 8 and np.all(ref.FAMILIES["dist8"][2][5:] != 0)
    pi = ref.family("pi")
    assert all(abs(np.trace(R) + 1.0) < 1e-12 for R in pi["R"])
    assert ref.family("identity")["R"][0].tolist() == np.eye(3).tolist()
    rx = ref.rodrigues(np.array([np.pi / 2, 0.0, 0.0]))
    assert all(abs(np.trace(R @ rx) + 1.0) < 1e-12 for R in ref.family("turned")["R"])   # turned about x, a rotation by pi


@pytest.mark.parametrize("name,noise", ref.NOISE_FREE)
def test_oracle_recovers_the_generating_pose(name, noise):
    s = side(name, noise)
    assert np.all(s["ok"])
    dev = np.array([ref.pose_dev(r, t, R, tt) for r, t, R, tt in zip(s["rvec"], s["tvec"], s["R"], s["t"])])
    print("%-8s oracle against the generating pose: worst R %.3g, worst t %.3g" % (name, dev[:, 0].max(), dev[:, 1].max()))
    assert dev.max() < ref.POSE_TOL


@pytest.mark.parametrize("name,noise", ref.ALL_CASES)
def test_oracle_is_at_the_polished_minimum(name, noise):
    s = side(name, noise)
    assert np.all(s["ok"])
    left_out = int(np.sum(~s["converged"]))
    print("%-8s noise %.1f: %d of %d unconverged, worst converged deviation from the polished minimum %.3g, worst of all %.3g"
          % (name, noise, left_out, ref.N_CASES, s["polish_dev"][s["converged"]].max(), s["polish_dev"].max()))
    assert left_out <= MAX_UNCONVERGED


@pytest.mark.parametrize("nm", ref.BOARD_SIZES + (129, 292, 293))
def test_boards_are_grids_of_separate_markers_in_front_of_the_camera(nm):
    ids, obj = ref.board(nm)
    assert obj.shape == (nm, 4, 3) and obj.dtype == np.float32 and len(set(ids.tolist())) == nm
    assert np.all(obj[:, :, 2] == 0)
    assert np.allclose(obj - obj.mean(axis=1, keepdims=True), ref.object_points(ref.MARKER_SIZE), atol=1e-6)   # each one a marker, in its corner order
    centres = obj.mean(axis=1)[:, :2]
    assert np.allclose(centres.mean(axis=0), 0.0, atol=0.06 / 2 + 1e-6)   # centred to within the partial last row
    gap = np.abs(centres[:, None] - centres[None]).max(axis=2) + np.eye(nm)
    assert gap.min() > ref.MARKER_SIZE + 0.009                                # no two markers touch
    for pose in ref.BOARD_POSES:
        for noise in (0.0, ref.NOISE):
            v = ref.board_view(nm, pose, noise, ref.K_OFF, seed=nm)
            assert v["corners"].shape == (nm, 4, 2) and v["corners"].dtype == np.float32
            assert np.all(obj.reshape(-1, 3) @ v["R"][2] + v["t"][2] > 0)
            clean = ref.brown_project(obj.reshape(-1, 3).astype(np.float64), v["R"], v["t"], v["K"], v["dist"]).reshape(nm, 4, 2)
            assert np.max(np.abs(clean - v["corners"])) < (2e-3 if noise == 0 else 6 * noise)
