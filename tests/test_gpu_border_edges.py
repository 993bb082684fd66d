"""GPU test of border following (aruco_amd/csrc/k_contours.hip: candidates_sparse_kernel, walker_kernel, walker_long_kernel, late_quad_kernel's walkers;
k_segments.hip) on the edge-topology cases of tests/border_ref.py: the same number of kept borders, the same hole flags and exactly the same points
(start pixel and direction included) as the oracle's find_contours filtered with lo < n < hi, and status 0, on every route into the kernels.
tests/test_border_edges_cpu.py proves on the CPU that these expected values equal the plain reference and that the cases reach the thresholds.

1. Handle(max_batch=1).detect_rectangles: the waypoint-segment pipeline, one frame (skipn), with ARUCOHIP_GRID 8, 16 and 32;
2. the walkers on one plane (one generation list, 32 start-candidate waves): Handle(max_batch=2), and ARUCOHIP_CONTOURS=walkers with max_batch=1;
3. the walkers on 64 planes or more (a sublist per plane % 8, 16 start-candidate waves): every case of a format repeated to 64 frames and more through
   THRES_FIXED, once synchronously (late generations forked) and once on a pipeline lane (late walks finished inside late_quad_kernel);
4. the segment pipeline's batch form (no skipn): ARUCOHIP_CONTOURS=segments with 12 planes.
The environment's switches are read once, when a handle is created: they are set before that.
"""
import ctypes as C

import numpy as np
import pytest

from tests import border_ref as B

pytestmark = pytest.mark.gpu


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
    """per format: [(family, index, image, kept borders of the oracle)]; computed once"""
    orc = env["orc"]
    res = {f: [] for f in B.FORMATS}
    for fam, i, fmt, img in B.all_cases():
        lo, hi = B.limits(fmt)
        res[fmt].append((fam, i, img, [c for c in orc.find_contours(img) if lo < len(c["pts"]) < hi]))
    return res


def handle(env, fmt, max_batch, fixed=False):
    capi = env["capi"]
    w, h, lo, hi = B.FORMATS[fmt]
    # four times the start-candidate / waypoint room a camera frame of this size gets: salt-and-pepper at 0.5 has a waypoint on every second pixel of
    # a grid line (a list that overflows is reported as such: tests/test_gpu_robustness.py; it is no matter of border following)
    lim = capi.Limits()
    capi.load().arucohip_default_limits(C.byref(lim), w, h, max_batch)
    lim.triggers_per_frame *= 4
    hd = capi.Handle(w, h, max_batch=max_batch, limits=lim)
    p = hd.get_params()
    p.min_size, p.max_size = lo, hi
    if fixed:
        p.thres_method, p.thres_param1, p.thres_param1_range = capi.THRES_FIXED, 100.0, 0
    hd.set_params(p)
    return hd


def capi_error(env):
    return env["capi"].ArucoHipError


def check_borders(got, kept, what):
    assert len(got) == len(kept), (what, len(got), len(kept))
    for a, b in zip(got, kept):
        assert a["hole"] == b["hole"] and np.array_equal(a["pts"], b["pts"]), (what, b["hole"], b["trig"], len(a["pts"]), len(b["pts"]))


def single_frames(env, expected, max_batch, what):
    """every case through detect_rectangles on a handle of its format -> borders compared, the counters summed per format"""
    total, sums = 0, {}
    for fmt, cases in expected.items():
        hd = handle(env, fmt, max_batch)
        try:
            for fam, i, img, kept in cases:
                try:
                    hd.detect_rectangles(img)
                except capi_error(env) as e:
                    raise AssertionError((what, fmt, fam, i, str(e)))
                check_borders(hd.debug_contours(0), kept, (what, fmt, fam, i))
                d = hd.debug_counters()
                assert d["status"] == 0, (what, fmt, fam, i, d)
                total += len(kept)
                s = sums.setdefault(fmt, {"long_walks": 0, "late_walks": 0})
                s["long_walks"] += d["raw"] if d["long_walks"] is None else d["long_walks"]
                s["late_walks"] += d["late_walks"]
        finally:
            hd.close()
    # a segment handle has no walks: the same counter word holds its waypoints there
    print("%s: %d borders compared, %s" % (what, total, {f: v["long_walks"] for f, v in sums.items()} if max_batch == 1 and "grid" in what else sums))
    return sums


@pytest.mark.parametrize("grid", ["8", "16", "32"])
def test_segment_pipeline_one_frame(env, expected, monkeypatch, grid):
    monkeypatch.setenv("ARUCOHIP_GRID", grid)
    monkeypatch.delenv("ARUCOHIP_CONTOURS", raising=False)
    single_frames(env, expected, 1, "segments, waypoints at grid " + grid)


@pytest.mark.parametrize("route", ["max_batch 2", "walkers"])
def test_walkers_one_plane(env, expected, monkeypatch, route):
    if route == "walkers":
        monkeypatch.setenv("ARUCOHIP_CONTOURS", "walkers")
    else:
        monkeypatch.delenv("ARUCOHIP_CONTOURS", raising=False)
    sums = single_frames(env, expected, 1 if route == "walkers" else 2, route)
    for fmt in ("sheet", "odd", "strip", "reach"):
        assert sums[fmt]["long_walks"] > 0, (fmt, sums)
    assert sums["strip"]["late_walks"] > 0 and sums["sheet"]["late_walks"] > 0, sums


def run_batch(env, fmt, frames, lane, look):
    """-> {frame: borders} of the frames in `look`, counters"""
    capi = env["capi"]
    hd = handle(env, fmt, len(frames), fixed=True)
    try:
        if lane:
            hd.set_pipeline_depth(2)
            out = np.zeros((len(frames), 64), capi.MARKER_DTYPE)
            n = np.zeros(len(frames), np.int32)
            hd.wait(hd.submit_host(frames, out, n))
        else:
            hd.detect_batch_host(frames, cap=64)
        d = hd.debug_counters()
        assert d["status"] == 0, d
        return {f: hd.debug_contours(f) for f in look}, d
    finally:
        hd.close()


@pytest.mark.parametrize("fmt", ["sheet", "strip", "odd"])
def test_walkers_64_planes_sync_and_lane(env, expected, monkeypatch, fmt):
    monkeypatch.delenv("ARUCOHIP_CONTOURS", raising=False)
    cases = expected[fmt]
    order = list(range(len(cases)))
    if len(order) % 8 == 0:
        order.append(0)                       # the second copy of a case then lies at another plane % 8
    while len(order) < 64 + len(cases):
        order += order[:len(cases) + (len(cases) % 8 == 0)]
    look = {}                                 # case -> two frames of it at different plane % 8
    for f, c in enumerate(order):
        if c not in look:
            look[c] = [f]
        elif len(look[c]) == 1 and (f - look[c][0]) % 8 != 0:
            look[c].append(f)
    assert len(order) >= 64 and all(len(v) == 2 for v in look.values())
    frames = np.ascontiguousarray(np.stack([255 - cases[c][2] for c in order]))
    chosen = sorted(f for v in look.values() for f in v)
    sync, d0 = run_batch(env, fmt, frames, False, chosen)
    lane, d1 = run_batch(env, fmt, frames, True, chosen)
    long_ones = sum(len(c["pts"]) > 960 for k in order for c in cases[k][3])
    total = 0
    for c, fs in look.items():
        fam, i, _, kept = cases[c]
        for f in fs:
            check_borders(sync[f], kept, ("sync", fmt, fam, i, f))
            check_borders(lane[f], kept, ("lane", fmt, fam, i, f))
            for a, b in zip(sync[f], lane[f]):
                assert a["start"] == b["start"] and a["pts"].tobytes() == b["pts"].tobytes()
            total += 2 * len(kept)
    print("%s, %d planes: %d borders compared; kept borders above 960 points %d; long walks sync %d lane %d, late walks sync %d lane %d, side streams %d / %d"
          % (fmt, len(order), total, long_ones, d0["long_walks"], d1["long_walks"], d0["late_walks"], d1["late_walks"], d0["side_streams"], d1["side_streams"]))
    assert d0["long_walks"] > 0 and d1["long_walks"] > 0
    if fmt != "odd":
        assert long_ones > 0
    assert d0["late_walks"] >= long_ones and d1["late_walks"] >= long_ones
    assert d1["side_streams"] == 0


@pytest.mark.parametrize("grid", ["8", "16", "32"])
def test_segment_pipeline_batch_form(env, expected, monkeypatch, grid):
    monkeypatch.setenv("ARUCOHIP_CONTOURS", "segments")
    monkeypatch.setenv("ARUCOHIP_GRID", grid)
    cases = [e for e in expected["sheet"] if e[0] in ("grid", "thin", "frame", "repass")]
    assert {"grid", "thin"} <= {e[0] for e in cases}
    order = [k % len(cases) for k in range(12)]
    assert len(cases) <= 12
    frames = np.ascontiguousarray(np.stack([255 - cases[c][2] for c in order]))
    got, d = run_batch(env, "sheet", frames, False, range(12))
    total = 0
    for f, c in enumerate(order):
        check_borders(got[f], cases[c][3], ("segments batch", grid, cases[c][0], cases[c][1], f))
        total += len(cases[c][3])
    print("segments, batch of 12, grid %s: %d borders compared" % (grid, total))
