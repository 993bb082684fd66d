"""GPU test of the two ways a batch's late walker generations are scheduled (aruco_amd/csrc/k_contours.hip: launch_walkers).

A handle that runs one batch at a time owns a side stream: the generations after the third (borders above 960 points) are forked onto
it and contour_quad runs in two passes around the join. A pipeline lane (set_pipeline_depth) owns no side stream: its batch runs on the
lane's stream alone, every generation in a row and contour_quad once. Here the same frames go through both:

* submit_device / wait on a handle with lanes against detect_batch_device on a handle without: counts, ids and the bytes of every
  live marker slot are equal, and the ids are the oracle's;
* the inputs reach the late generations on both paths (debug_counters' late_walks), so the comparison cannot pass on frames that
  never take the path that differs;
* a lane reports no side stream, a handle without lanes reports one.

The order in which waves append borders to the contour lists is not deterministic on either path; results are ordered by raster key.
"""
import numpy as np
import pytest

from tests.util import load_case

pytestmark = pytest.mark.gpu

CAP = 64
DEPTH = 2


@pytest.fixture(scope="module")
def env():
    import torch
    from aruco_amd import capi, synth
    from oracle import orc

    assert torch.cuda.is_available()
    return {"capi": capi, "orc": orc, "synth": synth, "torch": torch}


def fetch(env, out, cnt):
    """-> (counts int32[n], markers [n][CAP]) on the host"""
    env["torch"].cuda.synchronize()
    n = out.shape[0]
    return cnt.cpu().numpy().copy(), np.frombuffer(out.cpu().numpy().tobytes(), dtype=env["capi"].MARKER_DTYPE).reshape(n, CAP).copy()


def run_plain(env, frames):
    """detect_batch_device on a handle without lanes -> (counts, markers, debug counters)"""
    capi, torch = env["capi"], env["torch"]
    n, H, W = frames.shape
    h = capi.Handle(W, H, max_batch=n)
    try:
        out = torch.zeros((n, CAP * capi.MARKER_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        h.detect_batch_device(frames.data_ptr(), n, W, H, out.data_ptr(), CAP, cnt.data_ptr())
        h.batch_status()
        c, m = fetch(env, out, cnt)
        return c, m, h.debug_counters()
    finally:
        h.close()


def run_lanes(env, frames):
    """The same batch DEPTH + 1 times through submit_device / wait, DEPTH of them in flight at a time, so that every lane runs and the first
    lane runs twice -> [(counts, markers, debug counters)] per ticket"""
    capi, torch = env["capi"], env["torch"]
    n, H, W = frames.shape
    h = capi.Handle(W, H, max_batch=n)
    try:
        h.set_pipeline_depth(DEPTH)
        outs = [torch.zeros((n, CAP * capi.MARKER_DTYPE.itemsize), dtype=torch.uint8, device="cuda") for _ in range(DEPTH)]
        cnts = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(DEPTH)]
        torch.cuda.synchronize()
        res, tickets = [], {}

        def finish(slot):
            h.wait(tickets.pop(slot))
            c, m = fetch(env, outs[slot], cnts[slot])
            res.append((c, m, h.debug_counters()))   # of the waited ticket's lane: wait() adopts its batch

        for t in range(DEPTH + 1):
            slot = t % DEPTH
            if slot in tickets:
                finish(slot)
                outs[slot].zero_(), cnts[slot].zero_()
                torch.cuda.synchronize()
            tickets[slot] = h.submit_device(frames.data_ptr(), n, W, H, outs[slot].data_ptr(), CAP, cnts[slot].data_ptr())
        for slot in sorted(tickets, key=lambda s: tickets[s]):
            finish(slot)
        return res
    finally:
        h.close()


def check(env, frames, what):
    """Both paths on `frames` (uint8 [n, H, W] on the device) against each other and against the oracle's ids."""
    orc = env["orc"]
    n = frames.shape[0]
    c0, m0, d0 = run_plain(env, frames)
    lanes = run_lanes(env, frames)
    print("%s: plain late_walks %d side_streams %d; lanes %s" % (what, d0["late_walks"], d0["side_streams"],
                                                                 [(d["late_walks"], d["side_streams"]) for _, _, d in lanes]))
    # structure: the handle without lanes forks onto a side stream of its own, a lane has none
    assert d0["status"] == 0 and d0["side_streams"] >= 1
    # the inputs reach the generations the fork carries: borders of more than 960 points, on both paths
    assert d0["late_walks"] > 0
    assert len(lanes) == DEPTH + 1
    for c1, m1, d1 in lanes:
        assert d1["status"] == 0 and d1["side_streams"] == 0
        assert d1["late_walks"] == d0["late_walks"]
        assert np.array_equal(c0, c1)
        for f in range(n):
            assert 0 <= c0[f] <= CAP, (what, f, c0[f])
            assert m0[f, :c0[f]].tobytes() == m1[f, :c1[f]].tobytes(), (what, f)
    host = frames.cpu().numpy()
    o = orc.Oracle()
    found = 0
    for f in range(n):
        ref = [int(m["id"]) for m in o.detect(host[f])]
        assert [int(x) for x in m0[f, :c0[f]]["id"]] == ref, (what, f)
        found += len(ref)
    return found, m0, c0


def longest_outline(markers, counts):
    """Largest sum over the four sides of max(|dx|, |dy|) of a detected marker: a lower bound of its outer border's point count."""
    best = 0.0
    for f in range(len(counts)):
        for m in markers[f, :counts[f]]:
            q = np.asarray(m["corners"], float).reshape(4, 2)
            d = np.abs(q - np.roll(q, -1, axis=0))
            best = max(best, float(d.max(axis=1).sum()))
    return best


def test_flat_and_cluttered_1080p_in_one_batch(env):
    synth, torch = env["synth"], env["torch"]
    flat, _ = synth.make_stream(64, width=1920, height=1080, seed=4711, device="cuda")
    clut, _ = synth.make_stream(64, width=1920, height=1080, seed=4711, device="cuda", clutter=True)
    frames = torch.cat([flat, clut]).contiguous()
    torch.cuda.synchronize()
    found, _, _ = check(env, frames, "1080p flat + cluttered")
    assert found > 128 * 10


def test_4k_board_frames(env):
    """Two 3840x2160 board frames, default max_size: the sheet's outline and the markers' own borders (sides of about 300 px) are
    longer than the 960 points in front of the fork."""
    synth, torch = env["synth"], env["torch"]
    _, doc = load_case("board")
    board = doc["board_conf"]
    K = np.array(doc["intrinsics"]["K"], np.float32).reshape(3, 3)
    K[0, 0] *= np.float32(3840 / 640.0); K[0, 2] *= np.float32(3840 / 640.0)
    K[1, 1] *= np.float32(2160 / 480.0); K[1, 2] *= np.float32(2160 / 480.0)
    frames, _ = synth.make_board_stream(2, board["ids"], board["obj"], K.reshape(-1), width=3840, height=2160, seed=4711, device="cuda")
    torch.cuda.synchronize()
    found, m, c = check(env, frames.contiguous(), "4K board")
    assert found >= 2 * 20
    # seen from the results as well: a detected marker whose outline is longer than the whole schedule in front of the last listed generation
    print("4K board: longest detected outline %.0f px" % longest_outline(m, c))
    assert longest_outline(m, c) > 1024
