"""The device pose solver (aruco_amd/csrc/pnp_device.h: LDL^T without pivoting, the early Levenberg-Marquardt exit, its own Rodrigues
branches) at the edges: the families of tests/pose_ref.py through arucohip_calculate_extrinsics (four lanes per marker) and planar boards
through arucohip_board_detect (the whole wave per board), against the CPU restatement of solvePnP(ITERATIVE) and the generating poses.
Every comparison is at the project's pose tolerance, 1e-4, on rotation matrices and on tvec relative to its largest entry (an rvec at
theta ~ pi may come out as its antipode); rvec itself is compared where the reference's angle is below pi - 1e-3. The worst deviations are
printed, not asserted tighter: the reference and 1e-4 are the bar."""
import numpy as np
import pytest

from tests import pose_ref as ref
from tests.util import rel_err

pytestmark = pytest.mark.gpu

TOL = ref.POSE_TOL
SIZE = ref.MARKER_SIZE
NS = (1, 15, 16, 17, 48)            # partial groups of sixteen and a partial last workgroup of pose_kernel
K_SMALL = np.array([[600.0, 0.0, 320.0], [0.0, 600.0, 240.0], [0.0, 0.0, 1.0]])   # of the 640 x 480 frame of the in-detection test


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o

    return o


@pytest.fixture(scope="module")
def handle():
    from aruco_amd import capi

    h = capi.Handle(640, 480, max_batch=8)
    yield h
    h.close()


def _markers(corners, first_id=0):
    from aruco_amd import capi

    c = np.asarray(corners, np.float32).reshape(-1, 8)
    m = np.zeros(len(c), capi.MARKER_DTYPE)
    m["id"] = np.arange(len(c)) + first_id
    m["corners"] = c
    m["ssize"] = -1
    return m


def _side(orc, name, noise):
    return ref.reference_side(name, noise, orc.solve_pnp)


def _dev(got, rvecs, tvecs):
    """[n, 2]: pose_dev of every device marker against reference poses (rvecs: vectors or matrices)."""
    return np.array([ref.pose_dev(g["rvec"], g["tvec"], r, t) for g, r, t in zip(got, rvecs, tvecs)]).reshape(-1, 2)


def _check_family(got, s, n, label):
    """n markers of one family against its reference side: flags, the oracle (converged cases), the generating pose (without noise)."""
    assert len(got) == n
    assert np.all(got["has_pose"] == 1)
    assert np.all(np.isfinite(got["rvec"])) and np.all(np.isfinite(got["tvec"]))
    assert np.all(got["ssize"] == np.float32(SIZE))
    conv = s["converged"][:n]
    assert int(np.sum(~s["converged"])) <= 2                      # no family leaves out more than 2 of its 48 cases
    d_orc = _dev(got, s["rvec"][:n], s["tvec"][:n])
    below_pi = np.linalg.norm(s["rvec"][:n], axis=1) < np.pi - 1e-3
    d_rvec = np.array([rel_err(g["rvec"], r) for g, r in zip(got, s["rvec"][:n])])
    worst = [d_orc[conv].max() if conv.any() else 0.0, d_rvec[conv & below_pi].max() if (conv & below_pi).any() else 0.0]
    d_true = None
    if s["noise"] == 0:
        d_true = _dev(got, s["R"][:n], s["t"][:n])
    if label:
        print("%-8s noise %.1f n %2d: device against the oracle, worst R/t %.3g (%d of %d compared), worst rvec %.3g (%d below pi); all %d cases %.3g%s"
              % (s["name"], s["noise"], n, worst[0], int(conv.sum()), n, worst[1], int((conv & below_pi).sum()), n, d_orc.max(),
                 "" if d_true is None else "; against the generating pose %.3g" % d_true.max()))
    assert worst[0] < TOL
    assert worst[1] < TOL
    if d_true is not None:
        assert d_true.max() < TOL                                 # every noise-free case, no exclusions


@pytest.mark.parametrize("name,noise", ref.ALL_CASES)
def test_calculate_extrinsics_matches_the_oracle(handle, orc, name, noise):
    s = _side(orc, name, noise)
    assert np.all(s["ok"])
    for n in NS:
        got = handle.calculate_extrinsics(_markers(s["corners"][:n]), s["K"], s["dist"], SIZE)
        _check_family(got, s, n, label=True)


@pytest.mark.parametrize("name", ("mild", "steep", "pi", "turned"))
def test_y_perpendicular_is_the_oracles_rotation(handle, orc, name):
    """'turned': the rotated pose is a rotation by pi, so rotate_x_axis ends in rodrigues_mat2vec's s < 1e-5, c < 0 branch with nothing
    after it. (In the solver itself that branch only makes the start of the Levenberg-Marquardt loop, which recovers from a wrong sign.)"""
    s = _side(orc, name, 0.0)
    got = handle.calculate_extrinsics(_markers(s["corners"]), s["K"], s["dist"], SIZE, y_perp=True)
    assert np.all(got["has_pose"] == 1)
    turned = np.array([orc.rotate_x_axis(r) for r in s["rvec"]])
    d = _dev(got, turned, s["tvec"])
    assert s["converged"].all()   # no case is left out here
    print("%-8s y_perp: device against rotate_x_axis of the oracle's pose, worst R/t %.3g (all %d compared)" % (name, d.max(), len(d)))
    assert d.max() < TOL
    assert np.array_equal(got["rvec"], got["rvec"].astype(np.float32).astype(np.float64))   # kept at float precision, as rotate_x_axis leaves it


def _mixed(orc):
    """48 markers of one camera, interleaved: steep, far with noise, exactly pi, near identity; number 20 is degenerate (four equal corners)."""
    fams = [_side(orc, "steep", 0.0), _side(orc, "far", ref.NOISE), _side(orc, "pi", 0.0), _side(orc, "identity", 0.0)]
    corners = np.array([fams[i % 4]["corners"][i // 4] for i in range(48)])
    corners[20] = np.tile(np.float32([[700.25, 410.5]]), (4, 1))
    return corners, 20


def test_a_pose_does_not_depend_on_its_wave_neighbours(handle, orc):
    corners, bad = _mixed(orc)
    m = _markers(corners)
    together = handle.calculate_extrinsics(m, ref.K_MAIN, None, SIZE)
    clean = corners.copy()
    clean[bad] = _side(orc, "mild", 0.0)["corners"][0]
    without = handle.calculate_extrinsics(_markers(clean), ref.K_MAIN, None, SIZE)
    for i in range(48):
        alone = handle.calculate_extrinsics(m[i:i + 1], ref.K_MAIN, None, SIZE)[0]
        if i == bad:
            assert together[i]["has_pose"] == 0 or (np.all(np.isfinite(together[i]["rvec"])) and np.all(np.isfinite(together[i]["tvec"])))
            continue
        assert together[i]["has_pose"] == 1
        for f in ("rvec", "tvec"):
            assert together[i][f].tobytes() == alone[f].tobytes(), (i, f)
            assert together[i][f].tobytes() == without[i][f].tobytes(), (i, f)   # the degenerate one left its workgroup alone


def _hostile():
    """name -> corners [4, 2] float32."""
    P = ref.object_points(SIZE)
    R = ref.rodrigues(np.array([0.3, -0.2, 0.1])) @ ref.RX_PI
    good = ref.brown_project(P, R, np.array([0.05, -0.02, 0.8]), ref.K_MAIN, None)
    far_out = good.copy()
    far_out[2] = [1e7, -1e7]
    nan = good.copy()
    nan[1, 0] = np.nan
    behind = ref.brown_project(P, R, np.array([0.05, -0.02, -0.8]), ref.K_MAIN, None)   # the pinhole formula of a marker behind the camera
    return {"equal": np.tile([[700.25, 410.5]], (4, 1)),
            "collinear": np.array([[100.0, 100.0], [150.0, 125.0], [200.0, 150.0], [180.0, 300.0]]),
            "1e7": far_out, "nan": nan, "behind": behind}


def test_degenerate_and_hostile_corners_return(handle, orc):
    """The call returns, every output is finite or flagged has_pose = 0, has_pose equals the oracle's ok, and the valid neighbours of
    one workgroup keep their bytes. The NaN corner is the one input where the oracle, like cv::solvePnP, answers ok with a NaN pose (nothing
    in the method tests for NaN); the device does the same there, has_pose = 1 with a NaN pose, and that is what is asserted for it: a
    pose that is not finite is allowed only where the oracle's is not finite either."""
    P = ref.object_points(SIZE)
    cases = _hostile()
    valid = _side(orc, "mild", 0.0)["corners"][:16].copy()
    mixed = valid.copy()
    slots = {name: 3 * k + 1 for k, name in enumerate(cases)}
    for name, c in cases.items():
        mixed[slots[name]] = c.astype(np.float32)
    got = handle.calculate_extrinsics(_markers(mixed), ref.K_MAIN, None, SIZE)
    clean = handle.calculate_extrinsics(_markers(valid), ref.K_MAIN, None, SIZE)
    assert len(got) == 16
    for name, i in slots.items():
        ok, r, t = orc.solve_pnp(P, mixed[i], ref.K_MAIN.reshape(-1), None)
        finite = bool(np.all(np.isfinite(got[i]["rvec"])) and np.all(np.isfinite(got[i]["tvec"])))
        print("%-9s oracle ok %d (finite %d), device has_pose %d (finite %d)" % (name, ok, np.all(np.isfinite(r)) and np.all(np.isfinite(t)), got[i]["has_pose"], finite))
        assert got[i]["has_pose"] == int(ok)
        assert finite or got[i]["has_pose"] == 0 or (name == "nan" and not np.all(np.isfinite(r)))
    for i in set(range(16)) - set(slots.values()):
        assert got[i].tobytes() == clean[i].tobytes()


def _board_markers(view):
    m = _markers(view["corners"])
    m["id"] = view["ids"]
    return m


def _orc_markers(view):
    return [{"id": int(i), "corners": c} for i, c in zip(view["ids"], view["corners"])]


def _board_both(handle, orc, view, markers=None, thres=-1.0):
    from aruco_amd import capi

    m = _board_markers(view) if markers is None else markers
    om = [{"id": int(a["id"]), "corners": a["corners"].reshape(4, 2)} for a in m]
    got = handle.board_detect(m, view["ids"], view["obj"], capi.BOARD_METERS, K=view["K"], dist=view["dist"], marker_size=SIZE, repj_err_thres=thres)
    exp = orc.board_detect(om, view["ids"], view["obj"], capi.BOARD_METERS, view["K"].reshape(-1), view["dist"], SIZE, thres)
    return got, exp


def _board_dev(got, exp):
    assert got["has_pose"] == exp["has_pose"] == 1
    assert len(got["markers"]) == len(exp["markers"])
    assert abs(got["prob"] - exp["prob"]) < TOL
    assert np.all(np.isfinite(got["rvec"])) and np.all(np.isfinite(got["tvec"]))
    return ref.pose_dev(got["rvec"], got["tvec"], exp["rvec"], exp["tvec"])


@pytest.mark.parametrize("nm", ref.BOARD_SIZES)
def test_board_pose_over_the_whole_wave_matches_the_oracle(handle, orc, nm):
    """4 nm points through the G = 64 solver: fewer than a wave, no multiple of 64, and 512 (the batched kernel's MAX_BOARD_POINTS)."""
    worst = {}
    for ci, K in enumerate((ref.K_MAIN, ref.K_OFF)):
        for pi, pose in enumerate(ref.BOARD_POSES):
            for noise in (0.0, ref.NOISE):
                view = ref.board_view(nm, pose, noise, K, seed=9000 + 100 * nm + 10 * pi + ci)
                got, exp = _board_both(handle, orc, view)
                d = _board_dev(got, exp)
                worst[pose] = max(worst.get(pose, 0.0), max(d))
                if noise == 0:   # the generating pose as well
                    worst[pose + "/true"] = max(worst.get(pose + "/true", 0.0), max(ref.pose_dev(got["rvec"], got["tvec"], view["R"], view["t"])))
                assert max(d) < TOL, (pose, noise, ci, d)
    print("board of %3d markers (%3d points): worst R/t against the oracle %s" % (nm, 4 * nm, ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))
    assert all(v < TOL for k, v in worst.items() if k.endswith("/true"))


def test_board_capacity_is_what_the_header_documents(handle, orc):
    """include/arucohip.h: arucohip_board_detect solves up to 1168 correspondences (292 member markers), more give ARUCOHIP_E_CAPACITY.
    So 129 markers (one more than the batched kernel holds) and 292 are answered with the oracle's result, 293 with the error code."""
    from aruco_amd import capi

    for nm in (129, 292):
        view = ref.board_view(nm, "mild", ref.NOISE, ref.K_MAIN, seed=9900 + nm)
        got, exp = _board_both(handle, orc, view)
        d = _board_dev(got, exp)
        print("board of %3d markers: worst R/t against the oracle %.3g" % (nm, max(d)))
        assert max(d) < TOL
    view = ref.board_view(293, "mild", ref.NOISE, ref.K_MAIN, seed=9900 + 293)
    with pytest.raises(capi.ArucoHipError) as e:
        _board_both(handle, orc, view)
    assert e.value.code == capi.E_CAPACITY


@pytest.mark.parametrize("n_out", (3, 20))
def test_reprojection_filter_solves_again_without_the_outliers(handle, orc, n_out):
    view = ref.board_view(64, "mild", ref.NOISE, ref.K_MAIN, seed=9700 + n_out)
    m = _board_markers(view)
    rng = np.random.default_rng(9800 + n_out)
    for i in rng.choice(64, n_out, replace=False):
        a = rng.uniform(0.0, 2 * np.pi)
        m["corners"][i] += np.tile(np.float32([5.0 * np.cos(a), 5.0 * np.sin(a)]), 4)   # the marker's four corners, 5 px
    got, exp = _board_both(handle, orc, view, m, thres=1.5)
    _, unfiltered = _board_both(handle, orc, view, m)
    moved = max(ref.pose_dev(exp["rvec"], exp["tvec"], unfiltered["rvec"], unfiltered["tvec"]))
    d = _board_dev(got, exp)
    print("%2d displaced markers: the filter moves the oracle's pose by %.3g; device against the oracle, worst R/t %.3g" % (n_out, moved, max(d)))
    assert moved > TOL           # from the reference alone: the filter really removed points
    assert max(d) < TOL


def pose_frame():
    """One 640 x 480 frame from synth's painter with two markers seen by K_SMALL: one at 1.2 rad tilt, one of about 40 px."""
    from aruco_amd import synth

    P = ref.object_points(SIZE)[[1, 2, 3, 0]]   # the painter's order: top left, top right, bottom right, bottom left of the image
    layout = []
    for mid, tilt, t in ((77, 1.2, (-0.05, 0.0, 0.17)), (412, 0.3, (0.18, 0.1, 0.75))):
        R = ref.rodrigues(np.array([np.cos(0.4), np.sin(0.4), 0.0]) * tilt) @ ref.rot_z(0.3) @ ref.RX_PI
        quad = ref.brown_project(P, R, np.array(t), K_SMALL, None)
        layout.append({"id": mid, "quad": quad, "quad_q": ref.brown_project(P * 9.0 / 7.0, R, np.array(t), K_SMALL, None)})
    rng = np.random.RandomState(53)
    return synth.render_frame(layout, 640, 480, rng).numpy(), layout


def test_detection_pose_at_a_steep_tilt_and_40_px(handle, orc):
    """finalize_kernel -> marker_pose4, the kernel the benchmark runs, on the same solver: ids, corners and poses as the oracle's."""
    frame, layout = pose_frame()
    dist = ref.DIST8[:5]
    exp = orc.Oracle().detect(frame, K_SMALL.reshape(-1), dist, SIZE)
    assert sorted(m["id"] for m in exp) == sorted(mk["id"] for mk in layout)
    sides = {m["id"]: np.linalg.norm(m["corners"] - np.roll(m["corners"], 1, axis=0), axis=1) for m in exp}
    assert 35 < sides[412].max() < 45
    got = handle.detect(frame, K=K_SMALL, dist=dist, marker_size=SIZE)
    assert [int(m["id"]) for m in got] == [m["id"] for m in exp]
    for a, b in zip(got, exp):   # as test_gpu_parity's _compare_markers
        ca, cb = np.asarray(a["corners"], float).reshape(4, 2), np.asarray(b["corners"], float).reshape(4, 2)
        assert np.max(np.abs(ca - cb) / np.maximum(np.abs(cb), 1.0)) < TOL
        assert int(a["has_pose"]) == 1
        assert rel_err(a["rvec"], b["rvec"]) < TOL and rel_err(a["tvec"], b["tvec"]) < TOL
    d = _dev(got, [m["rvec"] for m in exp], [m["tvec"] for m in exp])
    print("in detection: device against the oracle, worst R/t %.3g" % d.max())
    assert d.max() < TOL
