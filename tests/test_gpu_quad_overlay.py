"""GPU test of contour_quad's point / block overlay (aruco_amd/csrc/k_contours.hip: border_to_quad). A border of at most QP_LDS = 1024 points
(DUAL_MAX = 512 when two share a wave) keeps its points in the LDS array that held the emitting lanes' 32x32 blocks a moment before, and the
write-back of the points to the pool reads them from there. So the test compares, exactly, the pool's points of EVERY kept border - those that end
as no quad included - with the oracle's border following, and the candidate quads with tests/quad_ref.py, at border lengths on both sides of every
limit of the overlay:

  DUAL_MAX   496, 511, 512, 513, 528         QP_LDS   1008, 1023, 1024, 1025, 1040
  the smallest borders the size filter admits with a last stretch of 16, 1 and 15 points: 32, 33, 31 (and 26, the smallest of all)

as axis-aligned rectangles (2 (w + h) - 4 points; one corner pixel less is one point less), the turned rectangles of quad_ref's length family, and
turned rectangles with notches and bumps, chamfered corners and combs, whose recursion splits more than once. One sheet, the crowd, holds more than 40
kept borders of 26 .. 1272 points (nested rings, so that the long ones fit, and small shapes beside them): in a batch of more than 8 planes every
workgroup of a plane then takes several borders in a row - borders above 1024 points (points in the pool), pairs of short ones, unpaired short ones
and single ones of 513 .. 1024 points in whatever order the descriptor slots came out, which differs from run to run, so results are compared as sets
(contours sorted by kind and start, the candidate list in its own deterministic order).

Routes: the synchronous batch (passes 1 and 2: the borders above 960 points come from the forked generations) and a pipeline lane (late_quad_kernel
and pass 3), both with more than 8 planes and ARUCOHIP_QUAD_DUAL = 1 and 0; one frame per call on handles of max_batch 1 (segment pipeline: the
points come from the pool into the array, no blocks) and 8 (walkers, a wave per border), synchronously and through a lane.
"""
import numpy as np
import pytest

from tests import quad_ref as Q

pytestmark = pytest.mark.gpu

DUAL_LIMIT = (496, 511, 512, 513, 528)
LDS_LIMIT = (1008, 1023, 1024, 1025, 1040)
SMALLEST = (26, 31, 32, 33)


def rect_of_count(n):
    """axis-aligned filled rectangle whose outer border has n points; odd n: the rectangle of n + 1 without its lower right corner pixel"""
    m = n + (n & 1)
    h = max(3, min(100, (m + 4) // 8))
    w = (m + 4) // 2 - h
    t = Q.tile([Q.rect(0, 0, w, h)])
    if n & 1:
        t[Q.QUIET + h - 1, Q.QUIET + w - 1] = 0
    return t


def ring_tile(w, h, rings, thick=2, gap=2):
    """nested rectangular rings: ring k's outer border has 2 (wk + hk) - 4 points, its hole border (thick 2: its corners are cut) 12 fewer"""
    m = np.zeros((h + 2 * Q.QUIET, w + 2 * Q.QUIET), np.uint8)
    x0, y0, x1, y1 = Q.QUIET, Q.QUIET, Q.QUIET + w, Q.QUIET + h
    for _ in range(rings):
        if x1 - x0 < 2 * thick + 3 or y1 - y0 < 2 * thick + 3:
            break
        m[y0:y1, x0:x1] = 1
        m[y0 + thick:y1 - thick, x0 + thick:x1 - thick] = 0
        x0, y0, x1, y1 = x0 + thick + gap, y0 + thick + gap, x1 - thick - gap, y1 - thick - gap
    return m


def crowd_sheet():
    """one 640 x 480 sheet with more than 40 kept borders of mixed lengths"""
    sheet = np.zeros((Q.SHEET_H, Q.SHEET_W), np.uint8)
    rings = ring_tile(398, 240, 13, thick=2, gap=6)          # outer borders 1272, 1208, ... and hole borders 12 fewer: 8 of them above 1024 points
    sheet[1:1 + rings.shape[0], 1:1 + rings.shape[1]] = rings * 255
    small = [rect_of_count(n) for n in (31, 32, 33, 40, 47, 48, 49, 63, 64, 65, 96, 130, 200, 26, 35, 52)]
    small += [Q.bumped(40, 30, 12, 9, -6, 8.0), Q.bumped(50, 24, 20, 11, 5, 0.0, "left"), Q.tile([Q.rot(Q.chamfered(60, 40, (9, 0, 10, 0)), 13.0)]),
              Q.tile(Q.comb(3, 10, 14, 26, 10)), Q.tile([Q.rot(Q.rect(0, 0, 120, 70), 7.0)]), Q.tile([Q.rot(Q.rect(0, 0, 150, 95), 17.0)])]
    regions = [(410, 1, Q.SHEET_W - 1, Q.SHEET_H - 1), (1, 250, 410, Q.SHEET_H - 1)]   # right of the rings, then below them: shelves in each
    r, (x, y, shelf) = 0, (regions[0][0], regions[0][1], 0)
    for t in small:
        th, tw = t.shape
        while True:
            x0, _, x1, y1 = regions[r]
            if x + tw > x1:
                x, y, shelf = x0, y + shelf, 0
            if y + th <= y1 and x + tw <= x1:
                break
            r += 1
            assert r < len(regions), "the crowd sheet is full"
            x, y, shelf = regions[r][0], regions[r][1], 0
        sheet[y:y + th, x:x + tw] = t * 255
        x, shelf = x + tw, max(shelf, th)
    return sheet


def limit_tiles():
    tiles = [rect_of_count(n) for n in DUAL_LIMIT + LDS_LIMIT + SMALLEST]
    # dented and turned quadrilaterals at the limits' sizes: notches and bumps make the recursion split more than once
    # (deeper than eps = 0.05 n: 25 points at 500, 50 at 1000)
    tiles += [Q.bumped(170, 62, 40, 30, -40, 3.0), Q.bumped(180, 50, 90, 25, 34, 5.0), Q.bumped(150, 70, 20, 22, -45, 0.0, "left"),
              Q.bumped(360, 96, 150, 60, -70, 2.0), Q.bumped(330, 90, 60, 40, 62, 4.0), Q.tile([Q.rot(Q.chamfered(390, 100, (9, 11, 10, 12)), 3.0)]),
              Q.tile([Q.rot(Q.chamfered(170, 70, (34, 0, 36, 0)), 11.0)])]
    return tiles


@pytest.fixture(scope="module")
def env():
    import torch
    from aruco_amd import capi
    from oracle import orc

    assert torch.cuda.is_available()
    capi.load()
    return {"capi": capi, "orc": orc, "torch": torch}


@pytest.fixture(scope="module")
def expected(env):
    """per sheet: (name, sheet, kept borders of the oracle sorted by kind and start, candidates of the reference); computed once"""
    orc = env["orc"]
    lo, hi = Q.size_limits(Q.SHEET_W, Q.SHEET_H, Q.MIN_SIZE, Q.MAX_SIZE)
    sheets = [("crowd", crowd_sheet())]
    sheets += [("limits%d" % i, s) for i, (s, _) in enumerate(Q.pack(limit_tiles()))]
    sheets += [("length%d" % i, s) for i, (s, _) in enumerate(Q.family("length")[1])]
    res = []
    for name, sheet in sheets:
        kept = sorted_contours([c for c in orc.find_contours(sheet) if lo < len(c["pts"]) < hi])
        res.append((name, sheet, kept, Q.sheet_candidates(sheet)))
    return res


def sorted_contours(conts):
    return sorted(conts, key=lambda c: (int(c["hole"]), int(c["pts"][0][1]), int(c["pts"][0][0]), len(c["pts"])))


def test_shapes_cover_the_limits(expected):
    """the lengths the overlay's limits ask for are there, the crowd is one, and shapes of more than four raw vertices are among them"""
    lengths = [len(c["pts"]) for e in expected for c in e[2]]
    assert set(DUAL_LIMIT + LDS_LIMIT + SMALLEST) <= set(lengths), sorted(set(DUAL_LIMIT + LDS_LIMIT + SMALLEST) - set(lengths))
    crowd = [len(c["pts"]) for c in expected[0][2]]
    print("crowd: %d kept borders, %s" % (len(crowd), sorted(crowd)))
    assert len(crowd) >= 40
    assert sum(n > 1024 for n in crowd) >= 4 and sum(960 < n <= 1024 for n in crowd) >= 1
    assert sum(512 < n <= 960 for n in crowd) >= 4 and sum(n <= 512 for n in crowd) >= 12
    assert {n % 16 for n in crowd if n <= 512} >= {0, 1, 15}
    assert sum(len(e[3]) for e in expected) >= 20     # candidates to compare
    traces = []
    for _, sheet, _, _ in expected[:4]:
        Q.sheet_candidates(sheet, traces=traces)
    assert sum(tr.raw >= 6 for tr, _ in traces) >= 4   # the recursion has split more than once


def handle(env, max_batch, fixed=False):
    capi = env["capi"]
    hd = capi.Handle(Q.SHEET_W, Q.SHEET_H, max_batch=max_batch)
    p = hd.get_params()
    p.min_size, p.max_size = Q.MIN_SIZE, Q.MAX_SIZE
    if fixed:
        p.thres_method, p.thres_param1, p.thres_param1_range = capi.THRES_FIXED, 100.0, 0
    hd.set_params(p)
    return hd


def check_frame(hd, frame, kept, cands, what):
    got = sorted_contours(hd.debug_contours(frame))
    assert [(c["hole"], len(c["pts"])) for c in got] == [(c["hole"], len(c["pts"])) for c in kept], what
    for a, b in zip(got, kept):
        assert np.array_equal(a["pts"], b["pts"]), (what, len(b["pts"]), b["hole"])
    q = hd.debug_candidates(frame)[0]
    assert q.shape == cands.shape and np.array_equal(q, cands), (what, q.tolist(), cands.tolist())


def run_frames(env, hd, frames, lane):
    """one call with `frames` through THRES_FIXED: the synchronous batch or a pipeline lane"""
    capi = env["capi"]
    if lane:
        out = np.zeros((len(frames), 64), capi.MARKER_DTYPE)
        n = np.zeros(len(frames), np.int32)
        hd.wait(hd.submit_host(frames, out, n))
    else:
        hd.detect_batch_host(frames, cap=64)
    d = hd.debug_counters()
    assert d["status"] == 0
    return d


@pytest.mark.parametrize("lane", [False, True], ids=["sync", "lane"])
@pytest.mark.parametrize("dual", ["1", "0"])
def test_batch_of_more_than_eight_planes(env, expected, monkeypatch, dual, lane):
    """every sheet, inverted, the crowd three times: 12 workgroups per plane take the crowd's borders four and more in a row"""
    monkeypatch.setenv("ARUCOHIP_QUAD_DUAL", dual)
    order = [0] + list(range(len(expected))) + [0]
    while len(order) < 9:
        order.append(1)
    frames = np.ascontiguousarray(np.stack([255 - expected[i][1] for i in order]))
    hd = handle(env, len(frames), fixed=True)
    try:
        if lane:
            hd.set_pipeline_depth(2)
        d = run_frames(env, hd, frames, lane)
        long_ones = sum(len(c["pts"]) > 960 for i in order for c in expected[i][2])
        print("late walks %d, kept borders above 960 points %d" % (d["late_walks"], long_ones))
        assert d["late_walks"] >= long_ones >= 20
        for f, i in enumerate(order):
            check_frame(hd, f, expected[i][2], expected[i][3], (expected[i][0], f, dual, lane))
    finally:
        hd.close()


@pytest.mark.parametrize("max_batch", [1, 8])
def test_one_frame_per_call(env, expected, max_batch):
    """detect_rectangles on the binary sheet: max_batch 1 is the segment pipeline (the points are in the pool already and are copied into the array),
    8 the walkers with a wave per kept border"""
    hd = handle(env, max_batch)
    try:
        for name, sheet, kept, cands in expected:
            quads = hd.detect_rectangles(sheet)
            check_frame(hd, 0, kept, cands, (name, max_batch))
            assert quads.tobytes() == cands.tobytes(), (name, max_batch)
            assert hd.debug_counters()["status"] == 0
    finally:
        hd.close()


@pytest.mark.parametrize("lane", [False, True], ids=["sync", "lane"])
def test_one_frame_per_call_through_detect(env, expected, lane):
    """one frame per call on a handle of max_batch 8 through the whole detector: synchronously (a side stream: passes 1 and 2) and on a pipeline lane
    (late_quad_kernel and pass 3)"""
    hd = handle(env, 8, fixed=True)
    try:
        if lane:
            hd.set_pipeline_depth(2)
        for name, sheet, kept, cands in expected:
            d = run_frames(env, hd, np.ascontiguousarray(255 - sheet)[None], lane)
            if any(len(c["pts"]) > 960 for c in kept):
                assert d["late_walks"] >= 1, name
            check_frame(hd, 0, kept, cands, (name, lane))
    finally:
        hd.close()
