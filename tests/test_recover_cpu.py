"""Board marker recovery without a GPU: the float64 restatement (tests/recover_ref.py) on hand-made lists, its conventions against the
oracle, the frame builder on the oracle alone, and the public surface (header, binding)."""
import os
import re

import numpy as np
import pytest

from tests import recover_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DMG = {1: [(3, 3)], 6: [(2, 2), (4, 3)], 10: [(1, 1), (1, 4), (2, 3), (3, 2), (4, 5), (5, 3)]}   # 1, 2 and 6 repainted cells


def square(cx, cy, half=20):
    return np.array([[cx - half, cy - half], [cx + half, cy - half], [cx + half, cy + half], [cx - half, cy + half]], float)


def hand_board(n=3):
    """n markers of 40 units side, 100 apart, METERS board seen frontally at z = 1 through K = diag(1, 1): image = object coordinates."""
    obj = np.array([[[100 * k - 20, -20, 0], [100 * k + 20, -20, 0], [100 * k + 20, 20, 0], [100 * k - 20, 20, 0]] for k in range(n)], float)
    return list(range(10, 10 + n)), obj


def hand_case(quads, cand_ids, votes, present=(0,), opt=None, n=3, **kw):
    ids, obj = hand_board(n)
    markers = [{"id": ids[k], "corners": obj[k, :, :2]} for k in present]
    Kid = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1]])
    o = {"min_markers": 1}
    o.update(opt or {})
    return rr.recover_frame(markers, quads, cand_ids, lambda ci: votes[ci], ids, obj, rr.METERS, Kid, opt=o, pose=(np.zeros(3), np.array([0, 0, 1.0])), **kw)


def bits(marker_id, rot=0, flips=()):
    """The votes a candidate shows for marker_id when the decoder needs rot rotations, with some cells flipped."""
    from aruco_amd import synth

    v = np.rot90(synth.marker_bits(marker_id), rot).copy()
    for cy, cx in flips:
        v[cy, cx] ^= 1
    return v


def test_greedy_order_and_a_candidate_is_taken_once():
    # candidate 0 lies between entries 1 and 2 (closer to 2), candidate 1 on entry 2: entry 1 comes first in board order and takes
    # candidate 0; entry 2 cannot take it again and gets candidate 1
    quads = [square(104, 0), square(203, 0)]
    r = hand_case(quads, [-1, -1], {0: bits(11), 1: bits(12)}, opt={"max_corner_dist": 150.0})
    assert r["adopted"] == [(1, 0, 0), (2, 1, 0)]
    # a decoded candidate is never considered
    r = hand_case(quads, [7, -1], {1: bits(12)})
    assert r["adopted"] == [(2, 1, 0)] and all(c[1] == 1 for c in r["considered"])


def test_ties_go_to_the_lower_candidate_then_the_lower_rotation():
    # two identical quads: the lower index wins. A square's four rotations are equally far: rotation 0 wins
    r = hand_case([square(100, 0), square(100, 0)], [-1, -1], {0: bits(11), 1: bits(11)}, present=(0, 2))
    assert r["adopted"] == [(1, 0, 0)]
    best = [c for c in r["considered"] if c[1] == 0][0]
    assert best[2] == 0 and best[3] == 0.0


def test_a_failed_cell_check_leaves_the_candidate_free_for_later_entries():
    # entry 1's nearest candidate shows entry 2's marker: entry 1 stays missing, entry 2 (within reach at this limit) takes it
    r = hand_case([square(150, 0)], [-1], {0: bits(12)}, opt={"max_corner_dist": 60.0})
    assert r["adopted"] == [(2, 0, 0)]
    assert [c[4] is not None for c in r["considered"]] == [True, True]


def test_the_distance_threshold_is_strict_and_the_cell_limit_inclusive():
    r = hand_case([square(110, 0)], [-1], {0: bits(11)}, present=(0, 2), opt={"max_corner_dist": 10.0})
    assert r["adopted"] == [] and r["considered"][0][3] == 10.0
    r = hand_case([square(110, 0)], [-1], {0: bits(11)}, present=(0, 2), opt={"max_corner_dist": 10.5})
    assert r["adopted"] == [(1, 0, 0)]
    three = [(2, 2), (3, 4), (6, 0)]
    assert hand_case([square(100, 0)], [-1], {0: bits(11, flips=three)}, present=(0, 2))["adopted"] == [(1, 0, 0)]
    assert hand_case([square(100, 0)], [-1], {0: bits(11, flips=three + [(1, 1)])}, present=(0, 2))["adopted"] == []


def test_min_markers_and_an_overflowed_frame_leave_the_frame_alone():
    args = ([square(100, 0)], [-1], {0: bits(11)})
    assert hand_case(*args, present=(0,), opt={"min_markers": 2})["adopted"] == []
    assert hand_case(*args, present=(0, 2), opt={"min_markers": 2})["adopted"] == [(1, 0, 0)]
    ids, obj = hand_board()
    assert rr.recover_frame(None, [], [], None, ids, obj, rr.METERS, np.eye(3))["adopted"] == []


def test_the_border_rectangle_and_a_full_marker_list():
    # the rectangle holds x in [95, 125): the quad's corners round to 80 .. 120, the left ones are outside
    r = hand_case([square(100, 0)], [-1], {0: bits(11)}, present=(0, 2), rect=(95, -50, 125, 50))
    assert r["adopted"] == [] and r["dropped"] == [(1, 0, 0)]
    r = hand_case([square(100, 0)], [-1], {0: bits(11)}, present=(0, 2), rect=(80, -20, 121, 21))
    assert r["adopted"] == [(1, 0, 0)]
    r = hand_case([square(100, 0)], [-1], {0: bits(11)}, present=(0, 2), rect=(80, -20, 120, 21))   # x1 is exclusive
    assert r["adopted"] == []
    assert rr.border_rect(640, 480) == (16, 12, 624, 468)
    r = hand_case([square(100, 0), square(200, 0)], [-1, -1], {0: bits(11), 1: bits(12)}, cap_markers=2)
    assert r["adopted"] == [(1, 0, 0)] and r["full"]


@pytest.mark.parametrize("turns", [0, 1, 2, 3])
def test_rotation_convention_against_the_projection(turns):
    """A candidate whose quad starts `rot` corners further along than the marker's first corner is adopted with that rotation, shows
    the marker turned accordingly, and its canonical corners are the projected ones - for boards turned by 0 / 90 / 180 / 270 degrees."""
    from aruco_amd import synth

    ids, obj = rr.board12()
    obj = rr.turned(obj, turns)
    proj = [synth.project(rr.K, rr.RVEC, rr.TVEC, o * rr.UNIT) for o in obj]
    markers = [{"id": ids[k], "corners": proj[k]} for k in range(12) if k != 5]
    for rot in range(4):
        quad = np.rint(np.array([proj[5][(i + rot) % 4] for i in range(4)]))    # quad[(i + 4 - rot) % 4] = corner i
        got = {}
        r = rr.recover_frame(markers, [quad], [-1], lambda ci: bits(ids[5], rot), ids, obj, rr.PIX, rr.K, pose=(rr.RVEC, rr.TVEC),
                             corners_of=lambda ci, ro: got.setdefault("c", np.array([quad[(i + 4 - ro) % 4] for i in range(4)])))
        assert r["adopted"] == [(5, 0, rot)]
        assert np.max(np.abs(got["c"] - proj[5])) <= 0.5 + 1e-9
        assert [c[4] for c in r["considered"]] == [0]


def test_brown_projection_reduces_to_the_pinhole_one_and_bends_outwards():
    from aruco_amd import synth

    ids, obj = rr.board12()
    pts = obj.reshape(-1, 3) * rr.UNIT
    a = rr.project(rr.K, rr.RVEC, rr.TVEC, pts, np.zeros(5))
    assert np.array_equal(a, synth.project(rr.K, rr.RVEC, rr.TVEC, pts))
    b = rr.project(rr.K, rr.RVEC, rr.TVEC, pts, [0.1, 0, 0, 0, 0])
    ctr = np.array([320.0, 240.0])
    assert np.all(np.linalg.norm(b - ctr, axis=1) > np.linalg.norm(a - ctr, axis=1))


@pytest.fixture(scope="module")
def damaged():
    from oracle import orc

    ids, obj = rr.board12()
    gray, quads = rr.build_frame(ids, obj, DMG)
    o = orc.Oracle()
    markers = o.detect(gray)
    return ids, obj, gray, markers, o.candidates()


def test_conventions_against_the_oracle(damaged):
    """On the oracle's own decoded candidates: the votes turned by -nrot are the marker, and (corner method NONE aside) the quad it
    reports is the integer quad turned by std::rotate(begin, begin + 4 - nRotations, end)."""
    from oracle import orc

    ids, obj, gray, markers, cands = damaged
    seen = 0
    for c in cands:
        if c["id"] < 0:
            continue
        assert rr.mismatches(rr.votes_from_frame(gray, c["quad0"]), c["id"], c["nrot"]) == 0
        seen += 1
    assert seen == 9
    o = orc.Oracle(corner_method=0)
    o.detect(gray)
    for c in o.candidates():
        if c["id"] >= 0:
            assert np.array_equal(c["quad"], np.array([c["quad0"][(i + 4 - c["nrot"]) % 4] for i in range(4)]))


def test_builder_reproduces_the_feasibility_case_on_the_oracle_alone(damaged):
    """Repainting 1, 2 and 6 inner cells of three markers: 9 of 12 detected, each lost marker keeps a rejected quad under 2 px from its
    projection through the survivors' board pose, the runner-up is over 30 px away, and the votes show exactly the painted counts."""
    ids, obj, gray, markers, cands = damaged
    assert len(markers) == 9 and sorted(m["id"] for m in markers) == sorted(ids[k] for k in range(12) if k not in DMG)
    quads, cids = [c["quad0"] for c in cands], [c["id"] for c in cands]
    votes = lambda ci: rr.votes_from_frame(gray, quads[ci])   # noqa: E731
    wide = rr.recover_frame(markers, quads, cids, votes, ids, obj, rr.PIX, rr.K, opt={"max_cell_errors": 6}, rect=rr.border_rect(rr.W, rr.H))
    rr.gate(wide, {"max_cell_errors": 6}, painted=(6,))
    assert [a[0] for a in wide["adopted"]] == [1, 6, 10]
    for j, cells in DMG.items():
        d = sorted((c[3], c[4]) for c in wide["considered"] if c[0] == j)
        assert d[0][0] < 2.0 and d[0][1] == len(cells) and d[1][0] > 30.0
    default = rr.recover_frame(markers, quads, cids, votes, ids, obj, rr.PIX, rr.K, rect=rr.border_rect(rr.W, rr.H))
    rr.gate(default)
    assert [a[0] for a in default["adopted"]] == [1, 6]


def test_background_squares_put_a_match_behind_64_candidates():
    from oracle import orc

    ids, obj = rr.board12()
    _, quads = rr.build_frame(ids, obj)
    gray, _ = rr.build_frame(ids, obj, {1: [(3, 3)]}, squares=rr.background_squares(quads))
    o = orc.Oracle()
    markers = o.detect(gray)
    cands = o.candidates()
    assert len(markers) == 11 and sum(c["id"] < 0 for c in cands) > 64
    r = rr.recover_frame(markers, [c["quad0"] for c in cands], [c["id"] for c in cands], lambda ci: rr.votes_from_frame(gray, cands[ci]["quad0"]),
                         ids, obj, rr.PIX, rr.K)
    assert len(r["adopted"]) == 1 and r["adopted"][0][0] == 1 and r["adopted"][0][1] >= 64


def test_header_and_binding_have_the_entry_point():
    from aruco_amd import capi

    txt = open(os.path.join(ROOT, "include", "arucohip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("arucohip_default_recover", "arucohip_board_recover_batch"):
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in capi.SYMBOLS
    assert "arucohip_recover_t" in txt
    assert callable(getattr(capi.Handle, "board_recover_batch")) and callable(getattr(capi.Handle, "board_recover_batch_device"))
    o = capi.default_recover()
    assert (o.max_corner_dist, o.max_cell_errors, o.min_markers, o.pose_markers) == (10.0, 3, 2, 0)
    import ctypes as C
    assert C.sizeof(capi.Recover) == 16
