"""GPU test of the contour-to-candidate stage (aruco_amd/csrc/k_contours.hip: contour_quad_kernel, late_quad_kernel, frame_candidates_kernel)
against the plain reference of tests/quad_ref.py on its edge-case sheets: exact equality of the kept borders' points (against the oracle's border
following, so that a mismatch is put down to the right stage) and of the candidate quads in order, status 0, on every route into the kernels and under
both settings of ARUCOHIP_QUAD_DUAL:

1. Handle(max_batch=1).detect_rectangles: the segment pipeline (points already in the pool);
2. Handle(max_batch=2).detect_rectangles: the walkers, pass 0;
3. all sheets, inverted, as one batch through THRES_FIXED (more than 8 planes: two short borders share a wave unless ARUCOHIP_QUAD_DUAL=0), once
   synchronously and once on a pipeline lane, where the borders of more than 960 points come from the late list (pass 3).
"""
import numpy as np
import pytest

from tests import quad_ref as Q

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
    """per sheet: (family, index, sheet, kept borders of the oracle, candidates of the reference); computed once"""
    orc = env["orc"]
    lo, hi = Q.size_limits(Q.SHEET_W, Q.SHEET_H, Q.MIN_SIZE, Q.MAX_SIZE)
    res = []
    for fam, i, sheet in Q.all_sheets():
        kept = [c for c in orc.find_contours(sheet) if lo < len(c["pts"]) < hi]
        res.append((fam, i, sheet, kept, Q.sheet_candidates(sheet)))
    return res


def handle(env, w, h, max_batch, min_size=Q.MIN_SIZE, max_size=Q.MAX_SIZE, fixed=False):
    capi = env["capi"]
    hd = capi.Handle(w, h, max_batch=max_batch)
    p = hd.get_params()
    p.min_size, p.max_size = min_size, max_size
    if fixed:
        p.thres_method, p.thres_param1, p.thres_param1_range = capi.THRES_FIXED, 100.0, 0
    hd.set_params(p)
    return hd


def check_frame(hd, frame, kept, cands, what, quads=None):
    got = hd.debug_contours(frame)
    assert len(got) == len(kept), what
    for a, b in zip(got, kept):
        assert a["hole"] == b["hole"] and np.array_equal(a["pts"], b["pts"]), what
    q = hd.debug_candidates(frame)[0]
    assert q.shape == cands.shape and np.array_equal(q, cands), (what, q.tolist(), cands.tolist())
    if quads is not None:
        assert quads.tobytes() == cands.tobytes(), what
    assert hd.debug_counters()["status"] == 0, what


@pytest.mark.parametrize("dual", ["1", "0"])
@pytest.mark.parametrize("max_batch", [1, 2])
def test_detect_rectangles_routes(env, expected, monkeypatch, max_batch, dual):
    monkeypatch.setenv("ARUCOHIP_QUAD_DUAL", dual)
    hd = handle(env, Q.SHEET_W, Q.SHEET_H, max_batch)
    try:
        for fam, i, sheet, kept, cands in expected:
            quads = hd.detect_rectangles(sheet)
            check_frame(hd, 0, kept, cands, (fam, i, max_batch, dual), quads)
    finally:
        hd.close()


def run_batch(env, frames, lane):
    """-> per frame (contours, candidate quads), counters"""
    capi = env["capi"]
    hd = handle(env, Q.SHEET_W, Q.SHEET_H, len(frames), fixed=True)
    try:
        if lane:
            hd.set_pipeline_depth(2)
            out = np.zeros((len(frames), 64), capi.MARKER_DTYPE)
            n = np.zeros(len(frames), np.int32)
            hd.wait(hd.submit_host(frames, out, n))
        else:
            hd.detect_batch_host(frames, cap=64)
        d = hd.debug_counters()
        assert d["status"] == 0
        return [(hd.debug_contours(f), hd.debug_candidates(f)[0]) for f in range(len(frames))], d
    finally:
        hd.close()


@pytest.mark.parametrize("dual", ["1", "0"])
def test_batch_sync_and_lane(env, expected, monkeypatch, dual):
    monkeypatch.setenv("ARUCOHIP_QUAD_DUAL", dual)
    assert len(expected) > 8           # more than 8 planes: the batch pairs short borders
    frames = np.ascontiguousarray(np.stack([255 - e[2] for e in expected]))
    sync, d0 = run_batch(env, frames, False)
    lane, d1 = run_batch(env, frames, True)
    # the borders of 961 / 1023 / 1024 / 1025 / 1279 points reach contour_quad through the late list (pass 3): a walk is late from 961 points on, so
    # every one of them is counted
    long_ones = sorted(len(c["pts"]) for e in expected for c in e[3] if len(c["pts"]) > 960)
    print("late walks: lane %d, synchronous %d; kept borders above 960 points: %s" % (d1["late_walks"], d0["late_walks"], long_ones))
    assert {961, 1023, 1024, 1025} <= set(long_ones)
    assert d1["late_walks"] >= len(long_ones)
    for f, (fam, i, _, kept, cands) in enumerate(expected):
        for name, (conts, q) in (("sync", sync[f]), ("lane", lane[f])):
            what = (fam, i, name, dual)
            assert len(conts) == len(kept), what
            for a, b in zip(conts, kept):
                assert a["hole"] == b["hole"] and np.array_equal(a["pts"], b["pts"]), what
            assert q.shape == cands.shape and np.array_equal(q, cands), (what, q.tolist(), cands.tolist())
        assert sync[f][1].tobytes() == lane[f][1].tobytes(), (fam, i)


def test_pairing_dual_equals_single(env, expected, monkeypatch):
    """the pairing sheets (odd and even kept-border counts, short and long borders in turns) and the sheet whose only two kept borders have 40 and
    512 points, so that these two share a wave whatever the order of the descriptors; repeated to 12 planes: the two settings give byte-equal candidates
    and contour points"""
    chosen = [e for e in expected if e[0].startswith("pairing") or e[0] == "couple"]
    assert sorted(len(c["pts"]) for e in chosen if e[0] == "couple" for c in e[3]) == [40, 512]
    frames = np.ascontiguousarray(np.stack([255 - e[2] for e in chosen] * 4))
    res = {}
    for dual in ("1", "0"):
        monkeypatch.setenv("ARUCOHIP_QUAD_DUAL", dual)
        res[dual], _ = run_batch(env, frames, False)
    for a, b in zip(res["1"], res["0"]):
        assert a[1].tobytes() == b[1].tobytes() and len(a[1]) >= 1
        assert len(a[0]) == len(b[0]) >= 2
        for x, y in zip(a[0], b[0]):
            assert x["hole"] == y["hole"] and x["start"] == y["start"] and x["pts"].tobytes() == y["pts"].tobytes()


@pytest.mark.parametrize("max_batch", [1, 2])
def test_far_sheet(env, max_batch):
    """coordinates near 2^14: packed 16-bit differences and the dot products of the scans"""
    orc = env["orc"]
    far = Q.far_sheet()
    cands = Q.sheet_candidates(far, 0.001, 0.5)
    lo, hi = Q.size_limits(Q.FAR_W, Q.FAR_H, 0.001, 0.5)
    kept = [c for c in orc.find_contours(far) if lo < len(c["pts"]) < hi]
    assert len(cands) == 3
    hd = handle(env, Q.FAR_W, Q.FAR_H, max_batch, 0.001, 0.5)
    try:
        quads = hd.detect_rectangles(far)
        check_frame(hd, 0, kept, cands, ("far", max_batch), quads)
    finally:
        hd.close()


@pytest.mark.parametrize("dual", ["1", "0"])
@pytest.mark.parametrize("max_batch", [1, 2])
@pytest.mark.parametrize("p1,rng", Q.MULTI_PARAMS)
def test_several_planes_through_detect(env, monkeypatch, p1, rng, max_batch, dual):
    """the adaptive threshold with thres_param1_range = 1 (three planes: identical outer quads with equal perimeters, the tie removes the earlier
    one) and = 3 (seven planes: a chain of near-duplicates in which removed quads go on removing), through detect"""
    monkeypatch.setenv("ARUCOHIP_QUAD_DUAL", dual)
    capi = env["capi"]
    g = Q.multi_frame()
    cands = Q.multi_candidates(g, p1, rng)
    assert len(cands) == Q.MULTI_COUNT[(p1, rng)]
    p = capi.default_params()
    p.thres_method, p.thres_param1, p.thres_param2, p.thres_param1_range = capi.THRES_ADPT, float(p1), 7.0, rng
    p.min_size, p.max_size = Q.MULTI_MIN, Q.MULTI_MAX
    hd = capi.Handle(Q.SHEET_W, Q.SHEET_H, max_batch=max_batch, params=p)
    try:
        hd.detect(g)
        q = hd.debug_candidates(0)[0]
        assert q.shape == cands.shape and np.array_equal(q, cands), (q.tolist(), cands.tolist())
        assert hd.debug_counters()["status"] == 0
    finally:
        hd.close()
