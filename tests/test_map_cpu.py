"""The host model of marker mapping (tests/map_ref.py) against itself: on every scene the GPU tests use, the specified start values
followed by the scipy solve reach the minimum that a solve started at the truth reaches; exact data give the truth back; and the
conditions under which the GPU tests could leave a case out hold for every chosen seed, so nothing is left out."""
import numpy as np
import pytest

from tests import map_ref as mr
from tests import pose_ref

TOL = pose_ref.POSE_TOL * mr.SIZE   # metres on a corner position


@pytest.mark.parametrize("name,noise,seed", mr.EXACT_CASES + mr.NOISY_CASES)
def test_start_values_reach_the_minimum_of_the_truth(name, noise, seed):
    c = mr.case(name, noise, seed)
    ref = c["ref"]
    assert ref is not None and ref["mapped"].all()
    # the reference alone sits far inside the bound the device is held to
    assert mr.obj_dev(ref["obj"], ref["truth_solved"]["obj"]) < TOL / 10
    assert abs(ref["rms"] - ref["truth_solved"]["rms"]) <= 1e-7 * max(ref["truth_solved"]["rms"], 1e-3)


@pytest.mark.parametrize("name,noise,seed", mr.EXACT_CASES)
def test_exact_data_give_the_truth(name, noise, seed):
    c = mr.case(name, noise, seed)
    assert mr.obj_dev(c["ref"]["obj"], mr.truth_obj(c["scene"])) < TOL / 10   # float32 corners: a few 1e-8 m
    assert c["ref"]["rms"] < 1e-4


def test_nothing_is_excluded():
    """What the GPU tests rely on: every frame of the cube but those that show one face is used, no start flips a marker (the start is
    within a marker side of the truth and the tree reaches every marker), the chain is three edges deep."""
    for name, noise, seed in mr.EXACT_CASES + mr.NOISY_CASES:
        c = mr.case(name, noise, seed)
        shown = np.bincount(c["obs"][0], minlength=c["nframes"])
        assert np.array_equal(c["ref"]["used"], shown >= 2), (name, seed)
        assert c["ref"]["used"].sum() >= 2
        assert mr.obj_dev(c["ref"]["start_obj"], mr.truth_obj(c["scene"])) < mr.SIZE / 2, (name, seed)
    assert mr.case("chain")["ref"]["depth"] == [0, 1, 2, 3]
    sc = mr.case("chain")["scene"]
    assert not any(0 in s and 3 in s for s in sc["show"])
    assert max(mr.case("cube", pose_ref.NOISE, 1)["ref"]["depth"]) >= 2


def test_selection_rules():
    c = mr.case("cube", 0.0, 0)
    fr, ids, cs = c["obs"]
    n = c["nframes"]
    board = c["scene"]["ids"]
    # an unlisted id, a repeated id (the second with other corners) and a frame with one listed marker change nothing
    extra_f = np.array([0, 0, n, n + 1], np.int32)
    extra_i = np.array([999, ids[0], board[0], 999], np.int32)
    extra_c = np.stack([cs[0], cs[0] + 5.0, cs[0], cs[0]]).astype(np.float32)
    order = np.argsort(np.concatenate([fr, extra_f]), kind="stable")
    obs2 = tuple(np.concatenate([a, b])[order] for a, b in ((fr, extra_f), (ids, extra_i), (cs, extra_c)))
    a = mr.select(c["obs"], n, board, c["scene"]["K"], c["scene"]["dist"])
    b = mr.select(obs2, n + 2, board, c["scene"]["K"], c["scene"]["dist"])
    assert not b[1][n] and not b[1][n + 1] and np.array_equal(a[1], b[1][:n])
    for ka, kb in zip(a[0], b[0]):
        assert [(m, q.tolist()) for m, q, _ in ka] == [(m, q.tolist()) for m, q, _ in kb]


def test_perimeter_rule_keeps_sixteen_in_detection_order():
    sc = mr.grid(17)
    obs = mr.observe(sc)
    per_frame, used = mr.select(obs, len(sc["frames"]), sc["ids"], sc["K"], sc["dist"])
    assert used.all()
    for f, kept in enumerate(per_frame):
        assert len(kept) == mr.MAX_FRAME_MARKERS
        rows = obs[2][obs[0] == f]
        per = [mr.perimeter(r) for r in rows]
        dropped = int(np.argmin(per))
        assert [m for m, _, _ in kept] == [m for m in range(17) if m != dropped]
        # the dropped quad is clearly the smallest: the rule does not hang on rounding
        assert sorted(per)[1] - sorted(per)[0] > 1e-3
    ref = mr.reference(obs, len(sc["frames"]), sc["ids"], sc["K"], sc["dist"])
    assert ref["mapped"].all() and mr.obj_dev(ref["obj"], mr.truth_obj(sc)) < TOL


def test_unconnected_marker_and_missing_reference():
    c = mr.case("chain")
    fr, ids, cs = c["obs"]
    board = c["scene"]["ids"]
    keep = ~((ids == board[3]) | ((ids == board[2]) & np.isin(fr, [f for f, s in enumerate(c["scene"]["show"]) if 3 in s])))
    obs = (fr[keep], ids[keep], cs[keep])
    ref = mr.reference(obs, c["nframes"], board, c["scene"]["K"], c["scene"]["dist"])
    assert ref["mapped"].tolist() == [True, True, True, False] and np.all(ref["obj"][3] == 0)
    no_ref = ids != board[0]
    assert mr.reference((fr[no_ref], ids[no_ref], cs[no_ref]), c["nframes"], board, c["scene"]["K"], c["scene"]["dist"]) is None


def test_island_of_two_markers():
    """two markers that see each other but never the rest: their frames pass the two-marker rule and are dropped with them"""
    c = mr.case("chain")
    obs, frames = mr.island(c)
    per_frame, used = mr.select(obs, c["nframes"], c["scene"]["ids"], c["scene"]["K"], c["scene"]["dist"])
    assert used[frames].all()
    ref = mr.reference(obs, c["nframes"], c["scene"]["ids"], c["scene"]["K"], c["scene"]["dist"])
    assert ref["mapped"].tolist() == [True, True, False, False] and not ref["used"][frames].any() and ref["used"].sum() == 4
    assert np.all(ref["obj"][2:] == 0) and mr.obj_dev(ref["obj"][:2], mr.truth_obj(c["scene"])[:2]) < TOL / 10
