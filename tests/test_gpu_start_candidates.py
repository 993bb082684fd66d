"""The border-start candidate lists of the walker pipeline (candidates_sparse_kernel) against their numpy restatement (tests/cand_ref.py), as sets
and per kind, at the shapes where the kernel takes another path: more than one strip of tiles, many tile rows per wave, rounds far above 64
candidates, runs that leave the 16 pixels at hand, the strip seam, the last tile column, a start in an empty tile, the last admissible column and row,
and the bench's 1080p frames in a synchronous batch and through a pipeline lane. A pin: the sets are what the kernel produced before it dealt one
candidate per lane and queued fewer tiles."""
import ctypes as C

import numpy as np
import pytest

from tests import cand_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    from aruco_amd import capi
    from oracle import orc

    assert torch.cuda.is_available()
    capi.load()
    return {"capi": capi, "orc": orc}


def _check_markers(got, ref):
    assert [int(m["id"]) for m in got] == [m["id"] for m in ref]
    for a, b in zip(got, ref):
        ca, cb = np.asarray(a["corners"], float).reshape(4, 2), np.asarray(b["corners"], float).reshape(4, 2)
        assert np.max(np.abs(ca - cb) / np.maximum(np.abs(cb), 1.0)) < 1e-4


def _check_lists(h, frame, ref):
    """The two lists of a frame equal the restatement as sets (and hold no pixel twice); returns their sizes' sum."""
    for kind, name in ((0, "outer"), (1, "hole")):
        got = h.debug_start_candidates(frame, kind)
        srt = np.sort(got)
        assert len(srt) == len(ref[name]), (name, len(srt), len(ref[name]))
        assert np.array_equal(srt, ref[name]), name
    return len(ref["outer"]) + len(ref["hole"])


def _run(env, grays, fixed=False, triggers=None, limits=None):
    """One synchronous batch on a walker handle: thresholded image, both lists of every frame, the counters and the markers."""
    capi, orc = env["capi"], env["orc"]
    grays = np.ascontiguousarray(grays, np.uint8)
    nf, hgt, wid = grays.shape
    p = capi.default_params()
    okw = {}
    if fixed:
        p.thres_method, p.thres_param1 = 0, 128
        okw = {"thres_method": 0, "thres_p1": 128}
    lim = limits
    if lim is None:
        lim = capi.Limits()
        capi.load().arucohip_default_limits(C.byref(lim), wid, hgt, max(nf, 2))
    if triggers:
        lim.triggers_per_frame = triggers
    h = capi.Handle(wid, hgt, max_batch=max(nf, 2), params=p, limits=lim)
    out = []
    try:
        got = h.detect_batch_host(grays)
        total = 0
        o = orc.Oracle(**okw)
        for f in range(nf):
            ref_m = o.detect(grays[f])
            thr = o.thresholded()
            assert np.array_equal(h.thresholded(f, (hgt, wid)), thr), f
            ref = cand_ref.start_candidates(cand_ref.binary_of(thr))
            total += _check_lists(h, f, ref)
            _check_markers(got[f], ref_m)
            out.append((ref, thr))
        cnt = h.debug_counters()
        assert cnt["status"] == 0 and cnt["triggers"] == total, (cnt, total)
    finally:
        h.close()
    return out


def _gray_of(binimg):
    return np.where(binimg, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("shape", [(32, 32), (33, 47), (32, 1040), (1040, 32)], ids=lambda s: "%dx%d" % (s[1], s[0]))
def test_random_frames(env, shape):
    """Noise through the adaptive threshold: one tile row per wave up to many, one strip and two."""
    rng = np.random.RandomState(shape[0] * 31 + shape[1])
    (ref, _), = _run(env, rng.randint(0, 256, (1,) + shape))
    assert len(ref["outer"]) + len(ref["hole"]) > 0


def test_checkerboard_rounds_far_above_64_candidates(env):
    """Every clear pixel of the checkerboard is a hole start: about 2000 candidates per round of 64 tiles, 150 k per frame, far beyond what a wave
    stages (the straight-to-list path)."""
    g = (np.indices((480, 640)).sum(0) % 2 * 255).astype(np.uint8)
    (ref, _), = _run(env, g[None], triggers=400000)
    assert len(ref["hole"]) > 150000


def test_bars_runs_at_the_horizons_the_seam_and_the_last_column(env):
    b, want = cand_ref.bars_frame()
    (ref, thr), = _run(env, _gray_of(b)[None], fixed=True)
    assert np.array_equal(thr != 0, b)
    assert ref["n64"] >= 40 and ref["n_long"] >= 16
    for kind, name in ((0, "outer"), (1, "hole")):
        got = set(ref[name].tolist())
        assert all((((y << 16) | x) in got) == keep for x, y, keep in want[kind])


@pytest.mark.parametrize("make", [cand_ref.empty_tile_frame, cand_ref.empty_tile_seam_frame], ids=["64x64", "seam"])
def test_hole_start_in_an_empty_tile(env, make):
    """Pixel (0, 0) of a tile without a set pixel starts a hole when the left and the upper tile hold its W and N neighbours; with only one of them
    non-empty, or both but not at those pixels, the tile holds nothing."""
    b, hit = make()
    (ref, thr), = _run(env, _gray_of(b)[None], fixed=True)
    assert np.array_equal(thr != 0, b)
    assert ref["kept_empty_tile"] == 1 and hit in ref["hole"].tolist()


@pytest.mark.parametrize("shape", [(42, 49), (41, 50)], ids=lambda s: "%dx%d" % (s[1], s[0]))
def test_starts_in_the_last_admissible_column_and_row(env, shape):
    b = cand_ref.last_column_row_frame(shape[1], shape[0])
    (ref, thr), = _run(env, _gray_of(b)[None], fixed=True)
    assert np.array_equal(thr != 0, b)
    assert ((5 << 16) | (shape[1] - 2)) in ref["outer"].tolist() and (((shape[0] - 2) << 16) | 21) in ref["hole"].tolist()


def test_bench_frames_in_a_batch_and_through_a_pipeline_lane(env):
    """Three flat and two cluttered 1080p frames of the bench's stream: the synchronous batch against the restatement, then the same batch through
    a pipeline lane: the markers' bytes and the lists of the synchronous call."""
    import torch
    from aruco_amd import synth
    capi = env["capi"]
    flat, _ = synth.make_stream(3, seed=4711, device="cuda")
    clut, _ = synth.make_stream(2, seed=4711, device="cuda", clutter=True)
    torch.cuda.synchronize()
    frames = np.ascontiguousarray(torch.cat([flat, clut]).cpu().numpy())
    nf, hgt, wid = frames.shape
    lim = capi.Limits()
    capi.load().arucohip_default_limits(C.byref(lim), wid, hgt, nf)
    lim.triggers_per_frame *= 4        # what the bench gives its cluttered stream
    lim.long_walks_per_plane *= 4
    lim.contours_per_frame *= 2
    done = _run(env, frames, limits=lim)
    refs = [r for r, _ in done]
    assert all(r["n64"] > 0 for r in refs)
    assert min(len(r["outer"]) + len(r["hole"]) for r in refs[3:]) > max(len(r["outer"]) + len(r["hole"]) for r in refs[:3])
    h = capi.Handle(wid, hgt, max_batch=nf, limits=lim)
    try:
        sync = h.detect_batch_host(frames)
        assert sum(len(m) for m in sync) >= 15 * nf
        h.set_pipeline_depth(2)
        out = np.zeros((nf, 128), capi.MARKER_DTYPE)
        n = np.zeros(nf, np.int32)
        h.wait(h.submit_host(frames, out, n))
        total = 0
        for f in range(nf):
            assert n[f] == len(sync[f]) and out[f, :n[f]].tobytes() == sync[f].tobytes(), f
            total += _check_lists(h, f, refs[f])
        cnt = h.debug_counters()
        assert cnt["status"] == 0 and cnt["triggers"] == total and cnt["side_streams"] == 0
    finally:
        h.close()


def test_segment_mode_keeps_no_lists(env):
    capi = env["capi"]
    h = capi.Handle(640, 480, max_batch=1)
    try:
        h.detect(np.full((480, 640), 128, np.uint8))
        with pytest.raises(capi.ArucoHipError) as e:
            h.debug_start_candidates(0, 0)
        assert e.value.code == capi.E_INVALID
    finally:
        h.close()
