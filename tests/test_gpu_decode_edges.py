"""The decode stage (aruco_amd/csrc/k_decode.hip, decode_device.h: homography_lane, warp_hist_kernel, otsu_kernel, cells_decode_kernel, hrm_decode_kernel)
held to the oracle at its edges, through the test hook arucohip_debug_decode_quads. Per candidate and without tolerances: iM against tests/decode_ref.py
bit for bit, the stored patch against orc.warp, the histogram against np.bincount of that patch, the threshold against orc.otsu, the cell bytes against
the 33rd-largest pixel of each cell, id and rotation against the oracle's decoders (the rotation where there is an id, as elsewhere in the suite). Every
family runs on the kernel paths its warp size has (decode_ref.paths_of), and the paths must agree byte for byte on what they have in common.
test_decode_edges_cpu.py pins the reference on the same cases and asserts that they are the edge cases they claim to be."""
import ctypes as C

import numpy as np
import pytest

from tests import decode_ref as ref

pytestmark = pytest.mark.gpu

MAX_W, MAX_H, MAX_BATCH, PER_FRAME = 4096, 400, 9, 512    # 512: the most candidates a frame of any handle holds


@pytest.fixture(scope="module")
def handle():
    from aruco_amd import capi

    lim = capi.Limits()
    capi.load().arucohip_default_limits(C.byref(lim), MAX_W, MAX_H, MAX_BATCH)
    lim.candidates_per_frame = PER_FRAME       # the flat list holds MAX_BATCH * 96 = 864 entries: room for the 800 of a three-frame call
    h = capi.Handle(MAX_W, MAX_H, max_batch=MAX_BATCH, limits=lim)
    yield h
    h.close()


def configure(h, ws, dictionary):
    key = (ws, None if dictionary is None else (dictionary[0], tuple(dictionary[1]), dictionary[2]))
    if getattr(h, "decode_edges_config", None) == key:
        return
    h.decode_edges_config = key
    p = h.get_params()
    if p.warp_size != ws:
        p.warp_size = ws
        h.set_params(p)
    if dictionary is None:
        h.set_dictionary(None, 0)
    else:
        n, codes, tau0 = dictionary
        h.set_dictionary(["".join("1" if (c >> i) & 1 else "0" for i in range(n * n)) for c in codes], tau0)


def run_path(h, s, nframes, dictionary, quads=None, frame_of=None, frames=None):
    configure(h, s["ws"], dictionary)
    if frames is None:
        frames, width = ref.device_frames(s, nframes)
    else:
        width = frames.shape[2]
    quads = s["quads"] if quads is None else quads
    if frame_of is None:
        frame_of = np.arange(len(quads), dtype=np.int32) % nframes
    return h.debug_decode_quads(frames, quads, frame_of=frame_of, width=width)


def compare(got, o, names, what, dictionary, idx=None):
    """every output the path left against the oracle side `o` (rows idx of it)"""
    idx = np.arange(len(names)) if idx is None else idx
    bad = []
    for k, i in enumerate(idx):
        w = "%s [%d] %s: " % (what, i, names[i])
        if got["iM"][k].tobytes() != o["iM"][i].tobytes():
            bad.append(w + "iM %r != %r" % (got["iM"][k].tolist(), o["iM"][i].tolist()))
        if got["patches"] is not None and got["patches"][k].tobytes() != o["patches"][i].tobytes():
            d = np.argwhere(got["patches"][k] != o["patches"][i])
            bad.append(w + "patch differs at %d pixels, first (y, x) = %s" % (len(d), d[0].tolist()))
        if not np.array_equal(got["hist"][k].astype(np.int64), o["hist"][i]):
            d = np.flatnonzero(got["hist"][k].astype(np.int64) != o["hist"][i])
            bad.append(w + "histogram differs at bins %s: %s != %s" % (d[:4].tolist(), got["hist"][k][d[:4]].tolist(), o["hist"][i][d[:4]].tolist()))
        if got["thr"][k] != o["thr"][i]:
            bad.append(w + "threshold %d != %d" % (got["thr"][k], o["thr"][i]))
        if got["cells"] is not None and got["cells"][k].tobytes() != o["cells"][i].tobytes():
            bad.append(w + "cell medians %s != %s" % (got["cells"][k].tolist(), o["cells"][i].tolist()))
        want = o["fid"][i] if dictionary is None else o["hrm"][i]
        if got["ids"][k] != want[0] or (want[0] >= 0 and got["nrot"][k] != want[1]):
            bad.append(w + "id, rotation (%d, %d) != (%d, %d)" % (got["ids"][k], got["nrot"][k], want[0], want[1]))
    assert not bad, "%d mismatches:\n%s" % (len(bad), "\n".join(bad[:12]))


@pytest.mark.parametrize("name", sorted(ref.case_sets()))
def test_every_path_equals_the_oracle(name, handle):
    from tests.test_decode_edges_cpu import oracle_side

    s, o = ref.case_sets()[name], oracle_side(name)
    results = []
    for path, nframes, dictionary in ref.paths_of(s):
        got = run_path(handle, s, nframes, dictionary)
        # the kernels the path is meant to take: cell medians only from three frames of the built-in decoder at 56, a stored patch otherwise
        assert (got["cells"] is not None) == (path == "three_frames" and s["ws"] == 56), path
        assert (got["patches"] is None) == (got["cells"] is not None), path
        compare(got, o, s["names"], "%s, %s" % (name, path), dictionary)
        results.append((path, dictionary, got))
    first = results[0]
    for path, dictionary, got in results[1:]:   # what the paths have in common is the same bytes
        for key in ("iM", "hist", "thr") + (("ids", "nrot") if (dictionary is None) == (first[1] is None) else ()):
            assert got[key].tobytes() == first[2][key].tobytes(), "%s: %s of %s and %s differ" % (name, key, first[0], path)
        if got["patches"] is not None and first[2]["patches"] is not None:
            assert got["patches"].tobytes() == first[2]["patches"].tobytes(), "%s: patches of %s and %s differ" % (name, first[0], path)


# ---- candidate counts: the XCD_RUN unpacking, the grid-stride loop, otsu_kernel's partial block and its 16-candidate staging
@pytest.fixture(scope="module")
def count_family():
    from oracle import orc

    W, H = ref.WIDE
    frames = np.stack([ref.noise((H, W), 40 + f) for f in range(3)])
    quads = ref.count_quads(max(ref.COUNTS), W, H)
    hn, codes, tau0 = ref.marker_dictionary()
    sides = {}
    for spread in (1, 3):          # the frame of quad i is i % spread
        n = len(quads)
        o = {"patches": np.zeros((n, 56, 56), np.uint8), "hist": np.zeros((n, 256), np.int64), "thr": np.zeros(n, np.int32), "iM": np.zeros((n, 9)),
             "fid": np.zeros((n, 2), np.int32), "hrm": np.zeros((n, 2), np.int32), "cells": np.zeros((n, 49), np.uint8)}
        for i, q in enumerate(quads):
            p = orc.warp(frames[i % spread], q.astype(np.float32), 56)
            o["patches"][i], o["hist"][i], o["thr"][i] = p, np.bincount(p.reshape(-1), minlength=256), orc.otsu(p)
            o["iM"][i], o["fid"][i], o["hrm"][i] = ref.homography(q, 56), orc.fiducial_detect(p), orc.hrm_detect(p, hn, codes, tau0)
            o["cells"][i] = ref.cell_medians(p).reshape(49)
        sides[spread] = o
    assert len({o["thr"][i] for o in sides.values() for i in range(len(quads))}) > 8    # the candidates are told apart by their results
    return {"ws": 56, "frames": frames, "quads": quads, "names": ["quad_%d" % i for i in range(len(quads))], "sides": sides}


@pytest.fixture(scope="module")
def alone(handle, count_family):
    """some of the family's quads run alone, one call each, on every path: what a candidate's outputs must be whatever runs beside it"""
    fam = count_family
    picks = sorted(set(range(0, 800, 9)) | set(range(40, 70)) | set(range(376, 392)) | {799})
    out = {}
    for path, nframes, dictionary in ref.paths_of({"kind": "three_paths", "hrm": ref.marker_dictionary()}):
        for i in picks:
            f = i % nframes
            out[path, i] = run_path(handle, fam, nframes, dictionary, quads=fam["quads"][i:i + 1], frame_of=np.array([f], np.int32), frames=fam["frames"][:nframes])
    return picks, out


@pytest.mark.parametrize("count", ref.COUNTS)
def test_candidate_counts(count, handle, count_family, alone):
    fam = count_family
    picks, single = alone
    ran = []
    for path, nframes, dictionary in ref.paths_of({"kind": "three_paths", "hrm": ref.marker_dictionary()}):
        c = min(count, nframes * PER_FRAME)     # this path's count: one frame holds 512 of the 800, three frames hold them all
        got = run_path(handle, fam, nframes, dictionary, quads=fam["quads"][:c], frames=fam["frames"][:nframes])
        assert len(got["ids"]) == c
        compare(got, fam["sides"][nframes], fam["names"], "%d candidates, %s" % (c, path), dictionary, idx=np.arange(c))
        for i in picks:
            if i < c:
                for key, v in single[path, i].items():
                    if v is not None:
                        assert got[key][i].tobytes() == v[0].tobytes(), "%d candidates, %s: %s of quad %d differs from the quad run alone" % (c, path, key, i)
        ran.append(c)
    assert ran == [min(count, PER_FRAME), count, count]     # both three-frame paths ran the count the test is named for


# ---- the hook itself
def test_hook_leaves_the_handle_usable():
    """detect, hook, detect on a golden still: the same marker bytes, through the single-frame graph (max_batch 1) and the eager path"""
    from aruco_amd import capi
    from aruco_amd.fixtures import load_case

    img, _ = load_case("board")
    H, W = img.shape
    s = ref.case_sets()["painted_basic"]
    small = np.ascontiguousarray(s["frame"][:, :1024])
    for max_batch in (1, 3):
        h = capi.Handle(max(W, 1024), max(H, small.shape[0]), max_batch=max_batch)
        try:
            before = [h.detect(img).tobytes() for _ in range(2)]
            assert before[0] == before[1] and len(before[0]) > 0
            for nframes in range(1, max_batch + 1):
                for ws in (56, 64):
                    configure(h, ws, None)
                    h.debug_decode_quads(np.stack([small] * nframes), s["quads"][:10])
                    with pytest.raises(capi.ArucoHipError):       # the hook's lists are not a batch
                        h.debug_otsu(0)
                configure(h, 56, None)
                assert h.detect(img).tobytes() == before[0], (max_batch, nframes)
        finally:
            h.close()


def test_hook_refuses_what_it_cannot_run(handle):
    from aruco_amd import capi

    s = ref.case_sets()["painted_basic"]
    configure(handle, 56, None)
    frames, width = ref.device_frames(s, 3)
    good = handle.debug_decode_quads(frames, s["quads"][:5], frame_of=[0, 1, 2, 0, 1], width=width)

    def code(fn):
        with pytest.raises(capi.ArucoHipError) as e:
            fn()
        return e.value.code

    cap_flat = MAX_BATCH * 96
    many = np.repeat(s["quads"][:1], cap_flat + 1, axis=0)
    assert code(lambda: handle.debug_decode_quads(frames, many, frame_of=np.arange(cap_flat + 1) % 3, width=width)) == capi.E_CAPACITY
    handle.debug_decode_quads(frames, many[:cap_flat], frame_of=np.arange(cap_flat) % 3, width=width)           # the list's last slot
    assert code(lambda: handle.debug_decode_quads(frames[:1], np.repeat(s["quads"][:1], PER_FRAME + 1, axis=0), width=width)) == capi.E_CAPACITY
    assert code(lambda: handle.debug_decode_quads(frames, s["quads"][:2], frame_of=[0, 3], width=width)) == capi.E_INVALID
    assert code(lambda: handle.debug_decode_quads(frames, s["quads"][:2], frame_of=[-1, 0], width=width)) == capi.E_INVALID
    assert code(lambda: handle.debug_decode_quads(frames[:1], s["quads"][:2], frame_of=[0, 1], width=width)) == capi.E_INVALID
    assert code(lambda: handle.debug_decode_quads(np.zeros((MAX_BATCH + 1, 64, 64), np.uint8), s["quads"][:1])) == capi.E_INVALID
    assert code(lambda: handle.debug_decode_quads(np.zeros((1, MAX_H + 1, 64), np.uint8), s["quads"][:1])) == capi.E_INVALID
    assert code(lambda: handle.debug_decode_quads(frames, np.zeros((0, 4, 2), np.int16), width=width)) == capi.E_INVALID
    L = handle.L
    assert L.arucohip_debug_decode_quads(handle.h, None, 1, 64, 64, 64, None, None, 1, None, None, None, None, None, None, None, None) == capi.E_INVALID
    decoder = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint8), C.c_int, C.POINTER(C.c_int))(lambda *a: -1)
    L.arucohip_set_decoder_callback.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    p = handle.get_params()
    handle._chk(L.arucohip_set_decoder_callback(handle.h, C.cast(decoder, C.c_void_p), None))
    p.decoder_kind = 2
    handle.set_params(p)
    try:
        assert code(lambda: handle.debug_decode_quads(frames, s["quads"][:2], width=width)) == capi.E_UNSUPPORTED
    finally:
        p.decoder_kind = 0
        handle.set_params(p)
        handle._chk(L.arucohip_set_decoder_callback(handle.h, None, None))
    again = handle.debug_decode_quads(frames, s["quads"][:5], frame_of=[0, 1, 2, 0, 1], width=width)      # a refusal changes nothing
    for key, v in good.items():
        assert (v is None and again[key] is None) or v.tobytes() == again[key].tobytes(), key
