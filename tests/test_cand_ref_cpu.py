"""The numpy restatement of the border-start candidates (tests/cand_ref.py) against the oracle's sequential scan, and the hand-made frames against
the paths they are meant to reach. No GPU."""
import numpy as np
import pytest

from tests import cand_ref
from tests.util import load_case


def _assert_scan_starts_are_candidates(thresholded):
    """Every border the sequential scan starts (more than one point: the restatement drops 1-point outer borders) is a candidate of its kind."""
    from oracle import orc
    b = cand_ref.binary_of(thresholded)
    ref = cand_ref.start_candidates(b)
    sets = {0: set(ref["outer"].tolist()), 1: set(ref["hole"].tolist())}
    borders = orc.find_contours(np.where(b, 255, 0).astype(np.uint8))
    n = {0: 0, 1: 0}
    for c in borders:
        if len(c["pts"]) < 2:
            continue
        x, y = c["trig"]
        assert ((y << 16) | x) in sets[c["hole"]], (c["hole"], x, y, len(c["pts"]))
        n[c["hole"]] += 1
    queue, wide, holds = cand_ref.queued_tiles(b)
    assert not (holds & ~queue).any() and not (queue & ~wide).any()      # no start-rule pixel outside the queued tiles
    # necessary, never sufficient: more candidates than borders, but not the whole start rule either
    assert n[0] <= len(sets[0]) and n[1] <= len(sets[1]) and len(sets[0]) + len(sets[1]) <= ref["n_start"]
    return n, ref


@pytest.mark.parametrize("name", ["single", "board", "board4x4", "chessboard", "hrm"])
def test_scan_starts_of_the_golden_stills_are_candidates(name):
    from oracle import orc
    gray, _ = load_case(name)
    n, ref = _assert_scan_starts_are_candidates(orc.adaptive_threshold(gray, 7, 7.0))
    assert n[0] > 10 and n[1] > 10


@pytest.mark.parametrize("clutter", [False, True], ids=["flat", "clutter"])
def test_scan_starts_of_synthetic_frames_are_candidates(clutter):
    from aruco_amd import synth
    from oracle import orc
    fr, _ = synth.make_stream(1, width=1280, height=720, seed=4711, n_markers=6, clutter=clutter)
    n, ref = _assert_scan_starts_are_candidates(orc.adaptive_threshold(fr[0].numpy(), 7, 7.0))
    assert n[0] > 10 and n[1] > 10
    assert ref["n64"] > 0


def test_scan_starts_of_the_hand_made_frames_are_candidates():
    for b in (cand_ref.bars_frame()[0], cand_ref.empty_tile_frame()[0], cand_ref.empty_tile_seam_frame()[0], cand_ref.last_column_row_frame(49, 42),
              cand_ref.last_column_row_frame(50, 41)):
        _assert_scan_starts_are_candidates(b)


def test_bars_frame_reaches_the_run_rule_paths():
    b, want = cand_ref.bars_frame()
    assert b.shape == (40, 1100)
    ref = cand_ref.start_candidates(b)
    for kind, name in ((0, "outer"), (1, "hole")):
        got = set(ref[name].tolist())
        assert len(want[kind]) == 29
        for x, y, keep in want[kind]:
            assert (((y << 16) | x) in got) == keep, (kind, x, y, keep)
        xs = [x for x, _, _ in want[kind]]
        assert any(x & 7 == 0 for x in xs) and any(x & 7 == 7 for x in xs)
        assert any(x < 1024 <= x + 16 for x in xs)                      # a run across the strip seam
        assert any(keep for _, _, keep in want[kind]) and not all(keep for _, _, keep in want[kind])
    assert b[2:12, 1098].any() and b[18:32, 1098].any()                 # runs that reach the last admissible column, both kinds
    assert ref["n64"] >= 40 and ref["n_long"] >= 16                     # decided by the 64-pixel test; runs longer than its horizon


def test_empty_tile_frames_reach_the_empty_tile_start():
    for make in (cand_ref.empty_tile_frame, cand_ref.empty_tile_seam_frame):
        b, hit = make()
        ref = cand_ref.start_candidates(b)
        assert ref["n_empty_tile"] == 1 and ref["kept_empty_tile"] == 1
        assert hit in ref["hole"].tolist()
        y, x = hit >> 16, hit & 0xFFFF
        assert x % 8 == 0 and y % 8 == 0 and not b[y:y + 8, x:x + 8].any()
        # the near misses: empty tiles with only one non-empty neighbour, or both but not at the two pixels, hold no start
        tiles = b.reshape(b.shape[0] // 8, 8, b.shape[1] // 8, 8).any(axis=(1, 3))
        left = np.zeros_like(tiles)
        left[:, 1:] = tiles[:, :-1]
        up = np.zeros_like(tiles)
        up[1:] = tiles[:-1]
        assert (~tiles & left & ~up).any() and (~tiles & ~left & up).any()
        if b.shape == (64, 64):
            assert (~tiles & left & up).sum() >= 2


def test_last_column_and_row_frames_reach_their_masks():
    for W, H in ((49, 42), (50, 41)):
        b = cand_ref.last_column_row_frame(W, H)
        ref = cand_ref.start_candidates(b)
        pts = [(v & 0xFFFF, v >> 16) for v in ref["outer"].tolist()], [(v & 0xFFFF, v >> 16) for v in ref["hole"].tolist()]
        assert (W - 2, 5) in pts[0] and (9, H - 2) in pts[0] and (1, 1) in pts[0]
        assert (21, H - 2) in pts[1] and (2, 4) in pts[1]
        # the hole start-rule pixel in column W - 2 is no candidate: its clear run enters the frame column, whose upper neighbour is clear
        assert (W - 2, 12) not in pts[1] and ref["n_start"] == len(pts[0]) + len(pts[1]) + 2


def test_checkerboard_has_rounds_far_above_64_triples():
    g = cand_ref.binary_of(np.indices((480, 640)).sum(0) % 2)
    ref = cand_ref.start_candidates(g)
    assert len(ref["hole"]) > 150000 and len(ref["outer"]) > 300      # 31-32 starts per tile: about 2000 per round of 64 tiles


def test_queue_predicate_on_bench_like_frames_is_tighter_and_complete():
    """Queue "own, or left AND upper" against "own, left or upper": a quarter fewer tiles on camera-like frames, and no start-rule pixel outside."""
    from aruco_amd import synth
    from oracle import orc
    for clutter in (False, True):
        fr, _ = synth.make_stream(1, seed=4711, clutter=clutter)
        queue, wide, holds = cand_ref.queued_tiles(cand_ref.binary_of(orc.adaptive_threshold(fr[0].numpy(), 7, 7.0)))
        assert not (holds & ~queue).any()
        assert queue.sum() < 0.8 * wide.sum(), (queue.sum(), wide.sum())
