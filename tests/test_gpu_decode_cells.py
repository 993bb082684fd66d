"""GPU tests of the decode stage's two variants (aruco_amd/csrc/k_decode.hip).

The default path of a batch (built-in 5x5 decoder, 56x56 patch, three frames or more) stores no patch: warp_hist_kernel keeps, per 8x8 cell, the 33rd-largest of the 64
samples a wave-gather holds, and otsu_kernel compares those 49 bytes with the threshold and decodes in the same lane. Every other path
(the caller's decoder, a dictionary, other warp sizes, one frame per call) still stores the patch. Here, on the same frames:

* the patches warp_hist_kernel stores - seen through the caller's-decoder callback, which receives them - equal the oracle's
  MarkerDetector::warp byte for byte (test_warp_bit_exact goes through arucohip_warp, which has a kernel of its own);
* the cell bytes the patch-free variant keeps equal the 33rd-largest of each cell of those patches;
* id and nRotations of every candidate - markers and rejected quads alike - are those of the oracle and of the patch-based path
  (the stored patch decoded by FiducidalMarkers::detect on the host), and the markers of both paths are the same bytes;

on the reference's stills, flat and cluttered 1080p streams in one batch, one frame per call (eager, captured, replayed), a frame whose
marker touches the image border and a 4K board frame.
"""
import ctypes as C

import numpy as np
import pytest

from tests.util import load_case

pytestmark = pytest.mark.gpu

WS = 56
RANK = (8 * 8) // 2 + 1   # "more than half of the cell's pixels exceed thr" = "its RANK-th largest pixel exceeds thr"
DECODER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint8), C.c_int, C.POINTER(C.c_int))


@pytest.fixture(scope="module")
def env():
    import torch  # noqa: F401
    from aruco_amd import capi, synth
    from oracle import orc

    assert torch.cuda.is_available()
    L = capi.load()
    L.arucohip_set_decoder_callback.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    return {"capi": capi, "orc": orc, "synth": synth, "torch": torch, "L": L}


def cell_medians(patch):
    """[7, 7] RANK-th largest pixel of each 8x8 cell of a 56x56 patch."""
    cells = patch.reshape(7, 8, 7, 8).transpose(0, 2, 1, 3).reshape(7, 7, 64)
    return np.sort(cells, axis=-1)[..., 64 - RANK]


class PatchPath:
    """The library's patch-storing path: the caller's decoder is registered, records every patch it is handed (calls come frame by frame
    in candidate order) and decodes it with the oracle's FiducidalMarkers::detect."""

    def __init__(self, env, handle):
        self.env, self.h, self.patches = env, handle, []
        orc = env["orc"]

        def cb(user, patch, size, nrot):
            a = np.ctypeslib.as_array(patch, shape=(size, size)).copy()
            self.patches.append(a)
            ident, r = orc.fiducial_detect(a)
            nrot[0] = r
            return ident

        self.fn = DECODER_FN(cb)

    def __enter__(self):
        assert self.env["L"].arucohip_set_decoder_callback(self.h.h, C.cast(self.fn, C.c_void_p), None) == 0
        p = self.h.get_params()
        p.decoder_kind = 2
        self.h.set_params(p)
        return self

    def __exit__(self, *exc):
        assert self.env["L"].arucohip_set_decoder_callback(self.h.h, None, None) == 0
        assert self.h.get_params().decoder_kind == 0


def check_frames(env, frames, one_per_call=False, cells=True, min_candidates=1):
    """Runs `frames` ([n, H, W] uint8) through the default path and through the patch path of one handle and compares both with the
    oracle candidate by candidate. Returns the number of candidates checked."""
    capi, orc = env["capi"], env["orc"]
    n, H, W = frames.shape
    h = capi.Handle(W, H, max_batch=1 if one_per_call else n)
    checked = 0
    cells = cells and not one_per_call and n > 2   # one frame per call and pairs of frames keep the stored patch: there is no cell array to read
    try:
        def run():
            """-> per frame: markers, (quads, ids, nrot), cell bytes or None"""
            out = []
            if one_per_call:
                for f in range(n):
                    for _ in range(3):   # eager, captured, replayed: the third call's results are the graph's
                        m = h.detect(frames[f])
                    out.append((m.copy(), h.debug_candidates(0), h.debug_cells(0) if cells and h.get_params().decoder_kind == 0 else None))
            else:
                got = h.detect_batch_host(frames, cap=64)
                assert h.debug_counters()["status"] == 0
                for f in range(n):
                    out.append((got[f].copy(), h.debug_candidates(f), h.debug_cells(f) if cells and h.get_params().decoder_kind == 0 else None))
            return out

        new = run()
        with PatchPath(env, h) as pp:
            old = run()
            patches = pp.patches
        if one_per_call:   # three calls per frame recorded three times the same patches: keep the last round of each frame
            kept, k = [], 0
            for f in range(n):
                nc = len(old[f][1][0])
                kept += patches[k + 2 * nc:k + 3 * nc]
                k += 3 * nc
            assert k == len(patches)
            patches = kept
        o = orc.Oracle()
        k = 0
        for f in range(n):
            o.detect_raw(frames[f])
            ref = o.candidates()
            (m_new, (q, ids, nrot), cb), (m_old, (q_p, ids_p, nrot_p), _) = new[f], old[f]
            assert len(ref) == len(q) == len(q_p), f
            assert m_new.tobytes() == m_old.tobytes(), f
            for i, r in enumerate(ref):
                assert np.array_equal(q[i], r["quad0"]) and np.array_equal(q_p[i], r["quad0"]), (f, i)
                patch = patches[k]
                k += 1
                assert np.array_equal(patch, orc.warp(frames[f], r["quad0"], WS)), (f, i)   # warp_hist_kernel's own samples
                if cb is not None:
                    assert np.array_equal(cb[i], cell_medians(patch)), (f, i)
                assert ids[i] == r["id"] and ids_p[i] == r["id"], (f, i, ids[i], ids_p[i], r["id"])
                if r["id"] >= 0:
                    assert nrot[i] == r["nrot"] and nrot_p[i] == r["nrot"], (f, i)
                checked += 1
        assert k == len(patches)
    finally:
        h.close()
    assert checked >= min_candidates
    return checked


def stream(env, n, seed, clutter=False):
    fr, _ = env["synth"].make_stream(n, width=1920, height=1080, seed=seed, device="cuda", clutter=clutter)
    env["torch"].cuda.synchronize()
    return fr.cpu().numpy()


def test_flat_and_cluttered_streams_in_one_batch(env):
    """192 flat + 64 cluttered bench frames (the bench's own seed first) as one batch: every candidate of every frame."""
    frames = np.concatenate([stream(env, 128, 4711), stream(env, 64, 31), stream(env, 64, 4711, clutter=True)])
    assert check_frames(env, frames) > 256 * 30


def test_golden_stills_batch_and_one_frame_per_call(env):
    for name in ("single", "board", "chessboard"):
        g, doc = load_case(name)
        check_frames(env, np.stack([g] * 4))
        check_frames(env, g[None], one_per_call=True)


def test_one_frame_per_call_on_stream_frames(env):
    frames = np.concatenate([stream(env, 3, 5), stream(env, 3, 6, clutter=True)])
    assert check_frames(env, frames, one_per_call=True) > 6 * 30


def test_marker_at_the_image_border(env):
    """A frame cropped so that a marker's black border starts one pixel from the image's left edge and another's ends one pixel from its
    bottom edge: the patches' outermost samples round onto the frame's first / last columns and rows (a sample that rounds past them reads 0)."""
    synth = env["synth"]
    fr, truth = synth.make_stream(1, width=1920, height=1080, seed=77, device="cuda")
    env["torch"].cuda.synchronize()
    g = fr[0].cpu().numpy()
    corners = [np.asarray(t["quad"], float).reshape(4, 2) for t in truth[0]]   # the markers' own outlines (their quiet zones reach further out)
    x0 = int(np.floor(min(c[:, 0].min() for c in corners if c[:, 0].min() > 200))) - 1
    y1 = int(np.ceil(max(c[:, 1].max() for c in corners if c[:, 1].max() < 900))) + 2
    crop = np.ascontiguousarray(g[:y1, x0:])
    assert check_frames(env, np.stack([crop] * 3)) >= 3 * 4
    check_frames(env, crop[None], one_per_call=True)


def board_4k():
    """The reference's board still enlarged twice in the bottom right corner of a 3840x2160 canvas: source coordinates up to 3780."""
    g, _ = load_case("board")
    big = np.full((2160, 3840), 255, np.uint8)
    up = np.kron(g, np.ones((2, 2), np.uint8))
    big[1150:1150 + up.shape[0], 2500:2500 + up.shape[1]] = up
    return big


def test_4k_frames(env):
    """4K: the enlarged board still, and a rendered 3840x2160 frame of 20 markers (sides 180-440 px: a patch sample steps over up to 8 source pixels)."""
    assert check_frames(env, np.stack([board_4k()] * 3)) >= 3 * 6
    fr, _ = env["synth"].make_stream(1, width=3840, height=2160, seed=12, device="cuda")
    env["torch"].cuda.synchronize()
    assert check_frames(env, np.concatenate([fr.cpu().numpy()] * 3)) >= 3 * 20
