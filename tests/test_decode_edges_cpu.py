"""tests/decode_ref.py held to the oracle on every family of the decode-stage edge suite (patch against orc.warp byte for byte, threshold against
orc.otsu, id and rotation against orc.fiducial_detect and orc.hrm_detect, the patch-level export of the oracle's HighlyReliableMarkers::detect), and
the properties that make each family an edge case, so that test_gpu_decode_edges.py cannot pass vacuously. oracle_side() is the reference both
files share: computed once per set."""
import functools

import numpy as np
import pytest

from oracle import orc
from tests import decode_ref as ref

SETS = sorted(ref.case_sets())


@functools.lru_cache(maxsize=None)
def oracle_side(name):
    """per quad of the set: the oracle's patch, its histogram, threshold, cell medians (ws 56), fiducial and dictionary decode; the restatement's iM"""
    s = ref.case_sets()[name]
    ws, frame = s["ws"], s["frame"]
    n = len(s["quads"])
    out = {"patches": np.zeros((n, ws, ws), np.uint8), "hist": np.zeros((n, 256), np.int64), "thr": np.zeros(n, np.int32),
           "iM": np.zeros((n, 9), np.float64), "fid": np.zeros((n, 2), np.int32), "hrm": np.zeros((n, 2), np.int32),
           "cells": np.zeros((n, 49), np.uint8)}
    for i, q in enumerate(s["quads"]):
        p = orc.warp(frame, q.astype(np.float32), ws)
        out["patches"][i] = p
        out["hist"][i] = np.bincount(p.reshape(-1), minlength=256)
        out["thr"][i] = orc.otsu(p)
        out["iM"][i] = ref.homography(q, ws)
        out["fid"][i] = orc.fiducial_detect(p)
        if s["hrm"] is not None:
            hn, codes, tau0 = s["hrm"]
            out["hrm"][i] = orc.hrm_detect(p, hn, codes, tau0)
        if ws == 56:
            out["cells"][i] = ref.cell_medians(p).reshape(49)
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.mark.parametrize("name", SETS)
def test_restatement_equals_the_oracle(name):
    s, o = ref.case_sets()[name], oracle_side(name)
    for i, q in enumerate(s["quads"]):
        what = "%s[%d] %s" % (name, i, s["names"][i])
        p = ref.warp(s["frame"], q, s["ws"], iM=o["iM"][i])
        assert p.tobytes() == o["patches"][i].tobytes(), what
        thr = ref.otsu(p)
        assert thr == o["thr"][i], what
        votes = ref.cell_votes(p, thr)
        assert np.array_equal(votes, ref.cell_medians(p) > thr), what   # "more than half exceed thr" is "the (half + 1)-th largest exceeds thr"
        fid = ref.fiducial_decode(votes)
        assert fid[0] == o["fid"][i][0] and (fid[0] < 0 or fid[1] == o["fid"][i][1]), what
        if s["hrm"] is not None:
            hn, codes, tau0 = s["hrm"]
            assert ref.hrm_decode(p, thr, hn, codes, ref.hrm_correction(tau0)) == tuple(o["hrm"][i]), what
        if s["painted"] is not None and i < len(s["painted"]):
            assert p.tobytes() == s["painted"][i].tobytes(), what + ": an identity quad's patch is the frame window under it"


def test_identity_quads_give_a_translation():
    iM = np.array(ref.homography(ref.identity_quad(1234, 77, 56), 56))
    assert np.abs(iM - np.array([1, 0, 1234, 0, 1, 77, 0, 0, 1.0])).max() < 1e-11   # 4e-15 relative of the coordinates


def test_restated_homography_is_the_float64_solution():
    """the largest relative difference of the restatement from np.linalg.solve over the well-conditioned families: the fallback bound for iM"""
    worst = 0.0
    for name in ("near_boundary", "painted_basic", "frame_edges"):
        s, o = ref.case_sets()[name], oracle_side(name)
        for q, iM in zip(s["quads"][:40], o["iM"]):
            d = 55.0
            A, b = np.zeros((8, 8)), np.zeros(8)
            for i, (dx, dy) in enumerate(((0, 0), (d, 0), (d, d), (0, d))):
                sx, sy = float(q[i][0]), float(q[i][1])
                A[i, :3], A[i, 6:] = (sx, sy, 1), (-sx * dx, -sy * dx)
                A[i + 4, 3:6], A[i + 4, 6:] = (sx, sy, 1), (-sx * dy, -sy * dy)
                b[i], b[i + 4] = dx, dy
            M = np.append(np.linalg.solve(A, b), 1.0).reshape(3, 3)
            inv = np.linalg.inv(M)
            got = np.array(iM).reshape(3, 3)
            worst = max(worst, float(np.abs(got / got[2, 2] - inv / inv[2, 2]).max() / np.abs(inv / inv[2, 2]).max()))
    print("restated iM against np.linalg: largest relative difference %.3g" % worst)
    assert worst < 1e-9


def test_near_boundary_family_has_all_three_bands():
    quads, bands, searched = ref.near_boundary_quads()
    frame = ref.wide_noise()
    print("near-boundary search: %d quads searched, %d kept" % (searched, len(quads)))
    count = {b: 0 for b in ref.BANDS}
    for q, band in zip(quads, bands):
        fX, fY = ref.sample_positions(ref.homography(q, 56), 56)
        d = ref.boundary_distance(fX, fY, frame)     # counts only samples whose two candidate source pixels lie in the frame and differ
        dmin = float(d.min())
        assert ref.band_of(dmin) == band
        if band == "exact":
            assert dmin == 0.0
        elif band == "inside_guard":
            assert 0.0 < dmin < ref.GUARD
        else:
            assert ref.GUARD <= dmin < ref.RCP_ERROR
        count[band] += 1
    assert all(c >= 16 for c in count.values()), count
    assert len({q.tobytes() for q in quads}) == len(quads)


def test_boundary_distance_counts_only_pixels_that_differ():
    flat = np.full((64, 64), 7, np.uint8)
    fX, fY = np.array([[10.5, 20.25]]), np.array([[5.0, 6.5]])
    assert np.isinf(ref.boundary_distance(fX, fY, flat)).all()
    steps = np.arange(64 * 64, dtype=np.int64).reshape(64, 64).astype(np.uint8)
    assert ref.boundary_distance(fX, fY, steps).tolist() == [[0.0, 0.0]]
    assert np.isinf(ref.boundary_distance(np.array([[63.5]]), np.array([[5.0]]), steps)).all()   # the far side lies outside the frame


def test_cell_tie_patches_hold_their_ties():
    kinds = set()
    for seed in range(6):
        p, marker_id, cells = ref.cell_tie_patch(seed)
        thr = orc.otsu(p)
        counts, med = ref.cell_counts(p, thr), ref.cell_medians(p)
        for cy, cx in cells:
            assert counts[cy, cx] in (32, 33) and med[cy, cx] in (thr, thr + 1)
            assert (counts[cy, cx] == 33) == (med[cy, cx] == thr + 1)
            kinds.add((int(counts[cy, cx]), int(med[cy, cx]) - thr))
        assert orc.fiducial_detect(p)[0] == marker_id   # and every tie is decisive: a vote the other way is another code
    assert kinds == {(32, 0), (33, 1)}


def test_painted_basic_patches_are_what_they_claim():
    s, o = ref.case_sets()["painted_basic"], oracle_side("painted_basic")
    by = {n: i for i, n in enumerate(s["names"])}
    for v in (0, 128, 255):
        i = by["uniform_%d" % v]
        assert o["thr"][i] == 0 and o["hist"][i][v] == 3136          # Otsu skips every bin; one counter takes every pixel
    for lo, hi in ((10, 12), (0, 255), (100, 180)):
        assert hi - lo >= 2                                          # sigma has a plateau lo .. hi - 1: the first bin of it wins
        for share in (1, 1568, 3135):
            i = by["two_levels_%d_%d_share_%d" % (lo, hi, share)]
            assert o["hist"][i][hi] == share and o["hist"][i][lo] == 3136 - share and o["thr"][i] == lo
    for name in ("ramp", "ramp_shuffled", "ramp_columns"):
        assert (o["hist"][by[name]] > 0).all()                       # every bin, every stage of 64, every group of 16
    assert (o["hist"][by["noise_0"]] > 0).sum() > 250


def test_marker_patches_decode_as_painted():
    s, o = ref.case_sets()["painted_markers"], oracle_side("painted_markers")
    ids = {}
    for name, (mid, nrot) in zip(s["names"], o["fid"]):
        if "_rot" in name:
            want, turn = int(name[2:name.index("_")]), int(name[-1])
            assert mid == want, name
            ids.setdefault(want, set()).add(int(nrot))
        elif "_flip" in name or "_border_" in name:
            assert mid == -1, name
    assert len(ids) == 64
    assert sum(len(v) == 4 for v in ids.values()) >= 60              # all four rotations are told apart (but for codes that are their own turn)
    assert sum("_border_" in n for n in s["names"]) == 24 and sum("_flip" in n for n in s["names"]) == 25


def test_rotation_ties_found_by_search():
    ties, n_valid, n_near = ref.rotation_ties()
    print("rotation ties: %d of the 1024 ids, %d of their one-bit neighbours" % (n_valid, n_near))
    assert (n_valid, n_near) == (1, 333)
    for bits in ties[:50]:
        rot = [bits]
        for _ in range(3):
            rot.append(ref.rotate(rot[-1]))
        d = [ref.hamm_dist(r) for r in rot]
        assert d.count(min(d)) > 1


def test_dictionary_cases_sit_on_the_correction_distance():
    accepted_at, rejected_past, saw_4095 = 0, 0, False
    for n, ws, codes, tau0, named in ref.hrm_cases():
        corr = ref.hrm_correction(tau0)
        for name, p in named:
            entry, dist = int(name.split("_entry")[1].split("_")[0]), int(name.split("_dist")[1].split("_")[0])
            got = orc.hrm_detect(p, n, codes, tau0)
            if dist == 0:
                assert got[0] >= 0 and (got[0] == entry or n < 4), name   # among 16 or 512 codes an earlier entry may be a turn of this one
                saw_4095 |= got[0] == 4095
            accepted_at += dist == corr and corr > 0 and got[0] == entry
            rejected_past += dist == corr + 1 and got[0] == -1
    assert saw_4095 and accepted_at >= 10 and rejected_past >= 10
    shapes = [(ws % (n + 2), (ws // (n + 2)) ** 2 % 2) for n, ws, _, _, _ in ref.hrm_cases()]
    assert any(r for r, _ in shapes) and any(odd for _, odd in shapes) and sorted({n for n, _, _, _, _ in ref.hrm_cases()}) == list(range(2, 9))


def test_warp_size_sets_cross_the_counter_switch():
    for ws in ref.WARP_SIZES:
        s, o = ref.case_sets()["warp_size_%d" % ws], oracle_side("warp_size_%d" % ws)
        assert o["hist"][s["names"].index("uniform_77")][77] == ws * ws
    # a histogram copy of the byte layout is shared by two lanes, which see two pixels of each 8 x 8 block
    peak = lambda ws: 2 * ((ws + 7) // 8) ** 2
    assert peak(88) == 242 and peak(88) < 256 <= peak(89)
    assert {88, 89} <= set(ref.WARP_SIZES)


def test_extreme_and_edge_quads_are_what_they_claim():
    s, o = ref.case_sets()["extreme_quads"], oracle_side("extreme_quads")
    by = {n: i for i, n in enumerate(s["names"])}
    for name in ("two_equal_corners", "all_equal"):
        i = by[name]
        assert not np.any(o["iM"][i]), name                                   # solve8 meets a zero pivot: iM = 0
        assert (o["patches"][i] == s["frame"][0, 0]).all(), name               # and every sample is pixel (0, 0)
    # Three corners on a line (or two equal ones that the elimination does not meet as a zero pivot): the system is singular, but rounding leaves
    # every pivot non-zero, so solve8 goes through. What is expected is no more than that: iM is not the zero matrix of the case above, every
    # entry and every sample position is finite, and the device equals the oracle on them as on any quad (test_restatement_equals_the_oracle
    # pins the patches here).
    for name in ("opposite_equal", "three_collinear", "four_collinear"):
        q, iM = s["quads"][by[name]].astype(np.int64), o["iM"][by[name]]
        cross = lambda a, b, c: (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
        assert any(cross(q[a], q[b], q[c]) == 0 for a, b, c in ((0, 1, 2), (1, 2, 3), (2, 3, 0), (3, 0, 1))), name
        assert np.isfinite(iM).all() and iM.any(), name
        fX, fY = ref.sample_positions(iM, 56)
        assert np.isfinite(fX).all() and np.isfinite(fY).all(), name
    for k in range(4):
        for name in ("foreshortened_%d" % k, "foreshortened_%d_t" % k):
            iM = o["iM"][by[name]]
            Wq = np.array([[iM[6] * x + (iM[7] * y + iM[8]) for x in (0, 55)] for y in (0, 55)])
            assert 9.5 < np.abs(Wq).max() / np.abs(Wq).min() < 11, name        # Wq varies tenfold over the patch (10.0 .. 10.7 here)
    s, o = ref.case_sets()["frame_edges"], oracle_side("frame_edges")
    by = {n: i for i, n in enumerate(s["names"])}
    for name in ("wholly_left", "wholly_right", "wholly_above", "wholly_below", "int16_min", "int16_max"):
        assert not o["patches"][by[name]].any(), name
    for name in ("left_out", "right_out", "top_out", "bottom_out", "corner_out", "far_corner_out", "one_past_right", "one_past_bottom"):
        p = o["patches"][by[name]]
        assert (p == 0).all(axis=0).any() or (p == 0).all(axis=1).any(), name  # a whole row or column of the patch lies outside
        assert p.any(), name
    H, W = s["frame"].shape
    assert np.array_equal(o["patches"][by["colW1_rowH1"]], s["frame"][H - 56:, W - 56:])
    assert np.array_equal(o["patches"][by["col0_row0"]], s["frame"][:56, :56])


def test_count_family_quads_are_all_different():
    q = ref.count_quads(max(ref.COUNTS), *ref.WIDE)
    assert len({x.tobytes() for x in q}) == 800 and ref.COUNTS[-1] == 800
