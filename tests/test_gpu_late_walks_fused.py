"""GPU test of a pipeline lane's late walks (aruco_amd/csrc/k_contours.hip: late_quad_kernel, launch_late_quads).

A lane runs generations 1..3 of the long border walks, then ONE launch whose leading workgroups walk every border of more than 960 points to its
end while the others run contour_quad over the borders known so far; the late borders go to a list of their own (from the top of each plane's
descriptor array) and a second, small contour_quad pass takes them. A handle without lanes forks the late generations onto a side stream, and one
frame per call takes the single-frame path. Here the same frames go through all three:

* a lane (set_pipeline_depth(2), submit_device / wait), the synchronous batch call, one detect() per frame: counts, ids and the bytes of every
  marker slot are equal, the ids are the oracle's and every rendered marker is among them, the status is 0;
* debug_counters' late_walks is equal on the lane and the synchronous path, zero where no border has more than 960 points and nonzero
  where one has.

Frames are drawn with numpy from a marker's 7 x 7 cells, scaled up cell by cell, with a white quiet zone of one cell on a flat gray ground, so that
the length of every border follows from the cell size: the black square of side s = 7 c has a border of about 4 s points, the quiet zone of
about 4 * 9 c. At 1920 x 1080 the size filter keeps borders of 308 .. 3839 points (max_contour = 0.5 * 1920 * 4 = 3840); generations 1..3 end at
64 + 128 + 256 + 512 = 960 steps, and the launches a side stream carries end at 1984 and 3008.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAP = 64
DEPTH = 2
GRAY, WHITE, BLACK = 120, 255, 0


def marker_tile(synth, marker_id, cell):
    """9 x 9 cells of `cell` pixels: the marker's 7 x 7 cells inside a white quiet zone"""
    m = np.ones((9, 9), np.uint8)
    m[1:8, 1:8] = synth.marker_bits(marker_id)
    return np.kron(np.where(m > 0, WHITE, BLACK).astype(np.uint8), np.ones((cell, cell), np.uint8))


def frame_with(synth, width, height, items, rect=None):
    """items: (marker id, cell size, x, y of the tile's top-left corner); rect: (x0, y0, x1, y1) painted white"""
    f = np.full((height, width), GRAY, np.uint8)
    if rect:
        f[rect[1]:rect[3], rect[0]:rect[2]] = WHITE
    for mid, cell, x, y in items:
        t = marker_tile(synth, mid, cell)
        assert 0 <= x and x + t.shape[1] <= width and 0 <= y and y + t.shape[0] <= height
        f[y:y + t.shape[0], x:x + t.shape[1]] = t
    return f


# cell sizes of the 1080p batch: border of the black square (28 c - 4 points) / of the quiet zone (36 c - 4)
#   22:  612 /  788   both below 960: no late walk, the pass over the late borders finds nothing
#   40: 1116 / 1436   960 .. 1984
#   90: 2516 / 3236   1984 .. 3008 / above 3008
#  115: 3216 / 4136   above 3008 / above max_contour: walked to the limit and dropped
RANGE_CELLS = (22, 40, 90, 115)


def range_frames(synth):
    """4 frames of 1920 x 1080 -> (frames, ids per frame, late borders expected per frame)"""
    frames, ids = [], []
    for i, cell in enumerate(RANGE_CELLS):
        items = [(100 + i, cell, 40 + 8 * i, 20 + 3 * i)]
        frames.append(frame_with(synth, 1920, 1080, items))
        ids.append(sorted(m[0] for m in items))
    return np.stack(frames), ids, [False, True, True, True]


def limit_frames(synth):
    """two 1080p frames (a batch: a one-frame handle takes the segment pipeline). The first holds a white rectangle whose border (2 * (1500 + 700) - 4 =
    4396 points) exceeds max_contour and never gets 1920 pixels away from its start, so the walk takes all 3840 steps; both hold a small marker"""
    f0 = frame_with(synth, 1920, 1080, [(77, 22, 1650, 800)], rect=(60, 50, 1560, 750))
    f1 = frame_with(synth, 1920, 1080, [(78, 22, 300, 200)])
    return np.stack([f0, f1]), [[77], [78]], [True, False]


def vga_frames(synth, n):
    """n frames of 640 x 480 (max_contour 1280), one marker of 7 * 37 = 259 px each: its black square's border has 1032 points"""
    frames, ids = [], []
    for i in range(n):
        mid = (37 * i + 5) % 1024
        frames.append(frame_with(synth, 640, 480, [(mid, 37, 20 + (i * 7) % 280, 10 + (i * 5) % 130)]))
        ids.append([mid])
    return np.stack(frames), ids, [True] * n


@pytest.fixture(scope="module")
def env():
    import torch
    from aruco_amd import capi, synth
    from oracle import orc

    assert torch.cuda.is_available()
    return {"capi": capi, "orc": orc, "synth": synth, "torch": torch}


def fetch(env, out, cnt):
    env["torch"].cuda.synchronize()
    n = out.shape[0]
    return cnt.cpu().numpy().copy(), np.frombuffer(out.cpu().numpy().tobytes(), dtype=env["capi"].MARKER_DTYPE).reshape(n, CAP).copy()


def run_sync(env, dev):
    capi, torch = env["capi"], env["torch"]
    n, H, W = dev.shape
    h = capi.Handle(W, H, max_batch=n)
    try:
        out = torch.zeros((n, CAP * capi.MARKER_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        h.detect_batch_device(dev.data_ptr(), n, W, H, out.data_ptr(), CAP, cnt.data_ptr())
        h.batch_status()
        c, m = fetch(env, out, cnt)
        return c, m, h.debug_counters()
    finally:
        h.close()


def run_lane(env, dev):
    """the batch twice through submit_device / wait, both in flight: one result per lane"""
    capi, torch = env["capi"], env["torch"]
    n, H, W = dev.shape
    h = capi.Handle(W, H, max_batch=n)
    try:
        h.set_pipeline_depth(DEPTH)
        outs = [torch.zeros((n, CAP * capi.MARKER_DTYPE.itemsize), dtype=torch.uint8, device="cuda") for _ in range(DEPTH)]
        cnts = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(DEPTH)]
        torch.cuda.synchronize()
        tickets = [h.submit_device(dev.data_ptr(), n, W, H, outs[i].data_ptr(), CAP, cnts[i].data_ptr()) for i in range(DEPTH)]
        res = []
        for i, t in enumerate(tickets):
            h.wait(t)
            c, m = fetch(env, outs[i], cnts[i])
            res.append((c, m, h.debug_counters()))   # of the waited ticket's lane: wait() adopts its batch
        return res
    finally:
        h.close()


def run_single(env, host):
    """one detect() per frame on a one-frame handle -> list of marker arrays"""
    capi = env["capi"]
    n, H, W = host.shape
    h = capi.Handle(W, H, max_batch=1)
    try:
        return [h.detect(host[f], cap=CAP) for f in range(n)]
    finally:
        h.close()


def check(env, host, ids, late, what, exact_ids=True):
    """The three paths on `host` (uint8 [n, H, W]) against each other and the oracle; ids[f]: the markers drawn into frame f (all must be found);
    late[f]: frame f has a border of more than 960 points that passes or fails the size filter only at its end"""
    torch, orc = env["torch"], env["orc"]
    n = host.shape[0]
    dev = torch.from_numpy(host).cuda().contiguous()
    c0, m0, d0 = run_sync(env, dev)
    lanes = run_lane(env, dev)
    single = run_single(env, host)
    print("%s: sync late_walks %d contours %d; lanes %s" % (what, d0["late_walks"], d0["contours"], [(d["late_walks"], d["contours"], d["side_streams"]) for _, _, d in lanes]))
    assert d0["status"] == 0
    assert (d0["late_walks"] > 0) == any(late), (what, d0)
    assert len(lanes) == DEPTH
    for c1, m1, d1 in lanes:
        assert d1["status"] == 0 and d1["side_streams"] == 0
        assert d1["late_walks"] == d0["late_walks"]
        assert d1["contours"] == d0["contours"] and d1["points"] == d0["points"]   # the late list is counted with the plane's other borders
        assert np.array_equal(c0, c1)
        for f in range(n):
            assert 0 <= c0[f] <= CAP
            assert m0[f, :c0[f]].tobytes() == m1[f, :c1[f]].tobytes(), (what, "lane", f)
    for f in range(n):
        assert len(single[f]) == c0[f], (what, "single", f)
        assert single[f].tobytes() == m0[f, :c0[f]].tobytes(), (what, "single", f)
    o = orc.Oracle()
    for f in range(n):
        ref = [int(m["id"]) for m in o.detect(host[f])]
        got = [int(x) for x in m0[f, :c0[f]]["id"]]
        assert got == ref, (what, f)
        if exact_ids:
            assert sorted(got) == sorted(ids[f]), (what, f, got)   # no exclusions: every marker drawn is one the oracle finds
    return d0


def late_of_frame(env, host):
    """late walks of ONE frame, through a lane: as a batch of two copies (a one-frame handle takes the segment pipeline, which has no walks)"""
    dev = env["torch"].from_numpy(np.stack([host, host])).cuda().contiguous()
    late = run_lane(env, dev)[0][2]["late_walks"]
    assert late % 2 == 0
    return late // 2


def test_borders_in_each_late_range(env):
    host, ids, late = range_frames(env["synth"])
    d = check(env, host, ids, late, "1080p ranges")
    # frame by frame: no late walk where every border is below 960 points (the pass over the late borders is empty), some in every other frame
    per = [late_of_frame(env, host[f]) for f in range(len(host))]
    print("late walks per frame", per)
    assert [p > 0 for p in per] == late
    assert sum(per) == d["late_walks"]


def test_border_above_max_contour(env):
    host, ids, late = limit_frames(env["synth"])
    d = check(env, host, ids, late, "1080p above max_contour")
    assert d["late_walks"] >= 1   # the rectangle's border: walked from its start to the limit, dropped


def test_sublists_and_one_list(env):
    host, ids, late = vga_frames(env["synth"], 64)
    d64 = check(env, host, ids, late, "64 x VGA (a sublist per XCD)")
    d3 = check(env, host[:3], ids[:3], late[:3], "3 x VGA (one list)")
    assert d64["late_walks"] >= 64 and d3["late_walks"] >= 3


def test_cluttered_frame(env):
    synth = env["synth"]
    # two frames: the smallest batch that takes the walkers (a one-frame handle takes the segment pipeline)
    frames, _ = synth.make_stream(2, width=1920, height=1080, seed=4711, device="cuda", clutter=True)
    host = frames.cpu().numpy()
    d = check(env, host, None, [True, True], "1080p cluttered", exact_ids=False)
    assert d["late_walks"] > 0   # many late walks that end bad or under the size filter
