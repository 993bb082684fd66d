"""The host model of the camera rig calls (tests/rig_ref.py) against the truth and against itself, the selection rules on hand-made
observations, and the CPU side of the C boundary. No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import pose_ref
from tests import rig_ref as rr
from tests.map_ref import compose, inverse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = pose_ref.POSE_TOL * rr.MARKER_SIZE   # the GPU tests' bound, 5e-6 m


@pytest.mark.parametrize("name", ["three", "pair1", "pair2", "chain", "island"])
def test_model_recovers_exact_rigs(name):
    """float32 corners without noise: the scipy minimum and even the start values lie far inside the GPU tests' bound"""
    c = rr.case(name)
    sc, ref = c["scene"], c["ref"]
    truth = rr.truth_T(sc)
    assert rr.cam_dev(ref["T"], truth, sc["obj"]) < TOL / 5 and rr.cam_dev(ref["start_T"], truth, sc["obj"]) < TOL / 5
    assert ref["rms"] < 1e-4
    for t, p in ref["poses"].items():
        assert rr.board_dev(p, sc["poses"][t], sc["obj"]) < TOL / 5
    if name == "island":
        assert ref["calibrated"].tolist() == [True, True, False] and ref["used"].tolist() == [True] * 4 + [False] * 2 and ref["T"][2] is None
    else:
        assert ref["calibrated"].all() and ref["used"].all()
    if name == "chain":
        assert ref["depth"] == [0, 1, 2]   # cameras 0 and 2 never share an instant


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_two_independent_solves_agree_on_the_noisy_scenes(seed):
    """the condition of the GPU test against scipy: Levenberg-Marquardt from the start values and a trust-region solve from the truth reach
    the same minimum within a tenth of that test's bounds (5e-6 m on the points, 1e-6 relative on the rms)"""
    c = rr.case("three", pose_ref.NOISE, seed)
    sc, ref = c["scene"], c["ref"]
    dev, rel = rr.cam_dev(ref["T"], ref["truth_T"], sc["obj"]), abs(ref["rms"] - ref["truth_rms"]) / ref["rms"]
    print("seed %d: lm from the start against trf from the truth %.3g m, rms rel %.3g; against the truth %.3g m"
          % (seed, dev, rel, rr.cam_dev(ref["T"], rr.truth_T(sc), sc["obj"])))
    assert dev < TOL / 10 and rel < 1e-7
    assert 0.2 < ref["rms"] / (pose_ref.NOISE * np.sqrt(2)) < 1.2   # the residual of 0.3 px of noise per coordinate


def test_selection_rules():
    c = rr.case("three", pose_ref.NOISE, 1)
    sc = c["scene"]
    vs, ids, cs = c["obs"]
    base = rr.select(c["obs"], sc["cams"], sc["ids"], sc["obj"], sc["ninstants"])
    assert all(v["n"] == 6 and v["counted"] for v in base)
    # an id that is not on the board; a repeat of view 0's first id behind the original
    extra = (np.concatenate([vs, [0, 0]]).astype(np.int32), np.concatenate([ids, [999, ids[0]]]).astype(np.int32),
             np.concatenate([cs, cs[:1] + 3.0, cs[:1] + 5.0]).astype(np.float32))
    more = rr.select(extra, sc["cams"], sc["ids"], sc["obj"], sc["ninstants"])
    assert more[0]["n"] == 6 and np.array_equal(more[0]["members"][0][1], base[0]["members"][0][1])
    assert np.array_equal(more[0]["V"][1], base[0]["V"][1])
    # min_markers
    few = tuple(a[(vs != 4) | (ids == sc["ids"][0])] for a in c["obs"])
    v4 = rr.select(few, sc["cams"], sc["ids"], sc["obj"], sc["ninstants"], min_markers=2)[4]
    assert v4["n"] == 1 and v4["V"] is not None and not v4["counted"]
    assert rr.select(few, sc["cams"], sc["ids"], sc["obj"], sc["ninstants"], min_markers=1)[4]["counted"]


def test_start_values_and_failures():
    c = rr.case("chain")
    sc = c["scene"]
    views = c["ref"]["views"]
    sv = rr.start_values(views, 3, sc["ninstants"])
    # camera 2 starts from the first instant it shares with camera 1: T_2 = V_t2 V_t1^-1 T_1
    t = 1
    want = compose(views[t * 3 + 2]["V"], compose(inverse(views[t * 3 + 1]["V"]), sv["T"][1]))
    assert np.array_equal(sv["T"][2][0], want[0]) and np.array_equal(sv["T"][2][1], want[1])
    # an instant's start: T_c^-1 V_tc from the lowest camera among those with the most member markers
    want = compose(inverse(sv["T"][1]), views[t * 3 + 1]["V"])
    assert np.array_equal(sv["poses"][t][1], want[1])
    vs = c["obs"][0]
    without0 = tuple(a[vs % 3 != 0] for a in c["obs"])
    assert rr.reference(without0, sc["cams"], sc["ids"], sc["obj"], sc["ninstants"]) is None
    only0 = tuple(a[vs % 3 == 0] for a in c["obs"])
    assert rr.reference(only0, sc["cams"], sc["ids"], sc["obj"], sc["ninstants"]) is None


def test_pose_model():
    c = rr.case("three")
    sc = c["scene"]
    T = rr.truth_T(sc)
    ref = rr.pose_reference(c["obs"], sc["cams"], T, [True, True, False], sc["ids"], sc["obj"], sc["ninstants"])
    for t, p in enumerate(ref):
        assert p["views_used"] == 2 and p["n_markers"] == 12
        assert rr.board_dev(p["pose"], sc["poses"][t], sc["obj"]) < TOL / 5
    vs = c["obs"][0]
    lone = tuple(a[(vs // 3 != 0) | (vs % 3 == 2)] for a in c["obs"])   # instant 0: camera 2 alone, which is not calibrated
    assert rr.pose_reference(lone, sc["cams"], T, [True, True, False], sc["ids"], sc["obj"], sc["ninstants"])[0] is None


def test_boundary_declares_the_rig_calls():
    from aruco_amd import capi

    txt = open(os.path.join(ROOT, "include", "arucohip.h")).read()
    assert int(re.search(r"#define ARUCOHIP_RIG_MAX_CAMERAS (\d+)", txt).group(1)) == capi.RIG_MAX_CAMERAS == rr.MAX_CAMERAS == 16
    for name in ("arucohip_rig_calibrate", "arucohip_rig_calibrate_batch", "arucohip_rig_pose", "arucohip_rig_pose_batch"):
        assert re.search(r"\b%s\s*\(" % name, txt) and name in capi.SYMBOLS and hasattr(capi.load(), name)
    # float K[9], dist[5]; int32 ndist, calibrated; double rvec[3], tvec[3]
    assert C.sizeof(capi.RigCamera) == 112 and capi.RigCamera.rvec.offset == 64 and capi.RigCamera.ndist.offset == 56
    arr = capi.Handle.rig_cameras(rr.cam_dicts(rr.case("pair2", solve=False)["scene"], truth=True))
    assert [cam.ndist for cam in arr] == [5, 4] and arr[1].calibrated == 1 and abs(arr[1].tvec[0] + 0.25 * np.cos(0.08)) < 1e-12
