"""The fixed-capacity device lists at their limits: filled exactly, one entry short, with neighbours, afterwards, and retried.

tests/test_gpu_robustness.py states the contract: what a list cannot hold "is reported through the status code (never silently truncated, never
out of bounds)". Here every list between the threshold pass and the marker array is loaded by a frame of tests/limits_ref.py whose demand D the
oracle or a numpy reference gives (tests/test_limits_cpu.py pins them), or - where the demand includes the implementation's bookkeeping: pool
words, waypoints, long-walk rings - a generous handle's own counters give, held to a bound from the reference. For each list:

  A  capacity = D: status 0, and markers, candidates and borders of every frame equal the generous handle's (default limits times 4).
  B  capacity = D - 1: ARUCOHIP_E_OVERFLOW, the loaded frame has n = -1, the batch status word and the TC_STATUS word of the loaded plane carry
     exactly the list's bit, every other plane's word is 0.
  C  B with the loaded frame first, in the middle and last among frames of real markers, and once more with three threshold planes a frame (the
     tests named "on three planes": lists 1, 2, 3, 5, 6, 9 and 10), where the loaded frame's planes are neighbours of each other: every other
     frame returns the generous handle's bytes, candidates and borders. The lists are [plane][capacity] arrays: a write past plane p's list, or a
     consumer that reads a counter without clamping it to the capacity, lands in plane p + 1. Nothing here can see a write past the LAST plane of
     an allocation; the tests do not build guard pages for it.
  D  the handle that just overflowed detects a batch of marked frames: status 0, the generous bytes.
  E  arucohip_detect_batch_retry_overflowed returns the generous handle's bytes for the loaded frame, one frame retried.

All comparisons are exact. Not reachable on handles of this size, and so not pinned: the generation sublists' own guard (k_contours.hip, `at <
gen_cap / gen_nx`) - below 64 planes a batch has one sublist per kind that holds every plane's rings, which the ring guard in front of it limits.
The cases that cut the segment pipeline's waypoint graph short come last in the file.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests import cand_ref, limits_ref as L

pytestmark = pytest.mark.gpu

TRIG, CDESC, POOL, QUAD, CAND, SEGMENT = 1, 2, 4, 8, 16, 64
CAP = 128
SQ10 = (12, 10, 24, 40, 20)        # 520 x 440: 120 kept borders, quads and candidates a plane
SQ8 = (12, 8, 24, 40, 20)          # 520 x 360: 96
SQ28 = (12, 10, 28, 40, 20)        # 520 x 440: both borders of a square are kept on the 7-pixel planes: 240 borders and quads, 120 candidates
SQ_MANY = (16, 12, 28, 36, 20)     # 616 x 472: 576 quads on three planes


@functools.lru_cache(maxsize=None)
def frame(name, h, w):
    if name[0] == "m" and name[1:].isdigit():
        return L.marked(int(name[1:]), h, w)
    g = {"sq10": lambda: L.squares(*SQ10), "sq8": lambda: L.squares(*SQ8), "sq28": lambda: L.squares(*SQ28), "many": lambda: L.squares(*SQ_MANY), "mixed": L.mixed,
         "checker": lambda: L.checker(h, w), "dominoes": lambda: L.dominoes(h, w), "blank": lambda: np.full((h, w), 255, np.uint8)}[name]()
    assert g.shape == (h, w), (name, g.shape)
    return g


@functools.lru_cache(maxsize=None)
def starts_of(name, h, w):
    sc = cand_ref.start_candidates(cand_ref.binary_of(L.plane_of(frame(name, h, w), fixed=128)))
    return len(sc["outer"]), len(sc["hole"])


class Env:
    def __init__(self):
        import torch
        from aruco_amd import capi

        assert torch.cuda.is_available()
        capi.load()
        self.capi, self.rigs = capi, {}

    def rig(self, *key):
        if key not in self.rigs:
            self.rigs[key] = Rig(self.capi, *key)
        return self.rigs[key]

    def close(self):
        for r in self.rigs.values():
            r.close()


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()


class Result:
    pass


class Rig:
    """One configuration - frame size, frames per batch, threshold planes, threshold, contour pipeline - with its generous handle and what that
    handle returned for every batch asked of it."""

    def __init__(self, capi, w, h, batch=3, planes=1, fixed=None, contours=None, grid=None):
        self.capi, self.w, self.h, self.batch, self.planes, self.fixed, self.contours, self.grid = capi, w, h, batch, planes, fixed, contours, grid
        self.big, self.seen = None, {}

    def close(self):
        if self.big is not None:
            self.big.close()

    def limits(self, scale=1, **over):
        lim = self.capi.Limits()
        self.capi.load().arucohip_default_limits(C.byref(lim), self.w, self.h, self.batch)
        lim.max_thres_planes = self.planes
        if scale != 1:
            lim.triggers_per_frame *= scale
            lim.contours_per_frame *= scale
            lim.points_per_frame *= scale
            lim.long_walks_per_plane = min(lim.long_walks_per_plane * scale, 1 << 16)
            lim.candidates_per_frame = min(lim.candidates_per_frame * scale, 512)
            lim.markers_per_frame = min(lim.markers_per_frame * scale, 256)
        for k, v in over.items():
            assert hasattr(lim, k)
            setattr(lim, k, int(v))
        return lim

    def handle(self, scale=1, **over):
        p = self.capi.default_params()
        if self.fixed is not None:
            p.thres_method, p.thres_param1 = self.capi.THRES_FIXED, float(self.fixed)
        p.thres_param1_range = (self.planes - 1) // 2
        keep = {k: os.environ.get(k) for k in ("ARUCOHIP_CONTOURS", "ARUCOHIP_GRID")}
        try:   # a handle reads the switches when it is created
            for k, v in (("ARUCOHIP_CONTOURS", self.contours), ("ARUCOHIP_GRID", self.grid)):
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = str(v)
            return self.capi.Handle(self.w, self.h, max_batch=self.batch, params=p, limits=self.limits(scale, **over))
        finally:
            for k, v in keep.items():
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v

    def frames(self, names):
        return np.stack([frame(n, self.h, self.w) for n in names])

    def collect(self, h, rc, n, out, names, look):
        r = Result()
        r.rc, r.n = rc, n.copy()
        r.rows = [out[f, :n[f]].tobytes() if n[f] >= 0 else None for f in range(len(names))]
        r.status = h.debug_counters()["status"]
        r.planes = [h.debug_plane_counters(p) for p in range(len(names) * self.planes)]
        r.seen = {f: (h.debug_contours(f), h.debug_candidates(f)) for f in (range(len(names)) if look is None else look)}
        return r

    def run(self, h, names, look=None):
        """one synchronous batch on host frames -> return code, counts, marker bytes, status words, and borders and candidates of the frames in look"""
        fr = self.frames(names)
        out, n = np.zeros((len(names), CAP), self.capi.MARKER_DTYPE), np.zeros(len(names), np.int32)
        p = self.capi._ptr
        rc = h.L.arucohip_detect_batch(h.h, p(fr), len(names), self.w, self.h, self.w, self.w * self.h, 0, None, None, 0, -1.0, 0, p(out), CAP, p(n), 0)
        assert rc in (self.capi.OK, self.capi.E_OVERFLOW), rc
        return self.collect(h, rc, n, out, names, look)

    def run_lane(self, h, names, look=None):
        """the same batch through a pipeline lane"""
        fr = self.frames(names)
        out, n = np.zeros((len(names), CAP), self.capi.MARKER_DTYPE), np.zeros(len(names), np.int32)
        if not getattr(h, "has_lanes", False):
            h.set_pipeline_depth(2)
            h.has_lanes = True
        rc = h.wait(h.submit_host(fr, out, n), allow=(self.capi.E_OVERFLOW,))
        return self.collect(h, rc, n, out, names, look)

    def generous(self, names):
        names = tuple(names)
        if names not in self.seen:
            if self.big is None:
                self.big = self.handle(scale=4)
            r = self.run(self.big, names)
            assert r.rc == self.capi.OK and r.status == 0 and all(p["status"] == 0 for p in r.planes), (names, r.status)
            self.seen[names] = r
        return self.seen[names]


def same_borders(a, b):
    return len(a) == len(b) and all(x["hole"] == y["hole"] and np.array_equal(x["pts"], y["pts"]) for x, y in zip(a, b))


def same_frame(r, ref, f, what):
    assert r.n[f] == ref.n[f] and r.rows[f] == ref.rows[f], (what, f, r.n[f], ref.n[f])
    if f in r.seen:
        assert same_borders(r.seen[f][0], ref.seen[f][0]), (what, f, "borders", len(r.seen[f][0]), len(ref.seen[f][0]))
        assert all(np.array_equal(x, y) for x, y in zip(r.seen[f][1], ref.seen[f][1])) and len(r.seen[f][1][0]) == len(ref.seen[f][1][0]), (what, f, "candidates")


def batch_of(loaded, at, n=3):
    names = ["m%d" % (i + 1) for i in range(n)]
    names[at] = loaded
    return names


def check_short(rig, r, ref, at, bit, plane_bits, what, allowed=0):
    """B and C: the loaded frame `at` is given up with exactly `bit`, on the planes plane_bits names ({offset in the frame: bits}, or "any": on at
    least one of the frame's planes and nothing else), every other frame is the generous handle's. allowed: bits that may come with `bit` where the
    test says why (the words must still hold `bit`, and nothing outside the two)"""
    capi, nthr = rig.capi, rig.planes
    assert r.rc == capi.E_OVERFLOW, (what, r.rc, r.status)
    assert [int(v) for v in np.nonzero(r.n < 0)[0]] == [at], (what, r.n)
    assert r.status & bit and not r.status & ~(bit | allowed), (what, r.status)
    mine = [r.planes[at * nthr + t]["status"] for t in range(nthr)]
    assert functools.reduce(int.__or__, mine) == r.status, (what, mine, r.status)      # the batch word is the planes' words together
    if plane_bits == "any":
        assert all(m == 0 or (m & bit and not m & ~(bit | allowed)) for m in mine), (what, mine)
    else:
        for t in range(nthr):
            want = plane_bits.get(t, 0)
            assert (mine[t] & ~allowed if want else mine[t]) == want, (what, mine, plane_bits)
    for f in range(len(r.n)):
        if f != at:
            assert all(r.planes[f * nthr + t]["status"] == 0 for t in range(nthr)), (what, f)
            same_frame(r, ref, f, what)


def check_list(rig, loaded, knob, fit, short, bit, plane_bits=None, positions=(1, 0, 2), retry=True, runner="run", allowed=0):
    """properties A to E of one list on one rig; fit / short: the knob's value for capacity D and for the largest capacity below D"""
    capi, n = rig.capi, rig.batch
    plane_bits = {0: bit} if plane_bits is None else plane_bits
    others = [f for f in range(n)]
    # A
    names = batch_of(loaded, min(1, n - 1), n)
    ref = rig.generous(names)
    h = rig.handle(**{knob: fit})
    try:
        r = getattr(rig, runner)(h, names)
        assert r.rc == capi.OK and r.status == 0 and all(p["status"] == 0 for p in r.planes), (knob, fit, r.rc, r.status)
        for f in others:
            same_frame(r, ref, f, (knob, fit, "exact fit"))
    finally:
        h.close()
    # B, C
    h = rig.handle(**{knob: short})
    try:
        for at in positions:
            names = batch_of(loaded, at, n)
            ref = rig.generous(names)
            r = getattr(rig, runner)(h, names, look=[f for f in others if f != at])
            check_short(rig, r, ref, at, bit, plane_bits, (knob, short, "loaded frame at %d" % at), allowed)
        # D
        names = batch_of("m%d" % (n + 1), 0, n)
        ref = rig.generous(names)
        r = getattr(rig, runner)(h, names)
        assert r.rc == capi.OK and r.status == 0, (knob, short, "afterwards", r.rc, r.status)
        for f in others:
            same_frame(r, ref, f, (knob, short, "afterwards"))
        # E
        if retry:
            names = batch_of(loaded, positions[0], n)
            ref = rig.generous(names)
            got, retried, first = h.detect_batch_host_tolerant(rig.frames(names), cap=CAP)
            assert retried == 1 and [int(v) for v in np.nonzero(first < 0)[0]] == [positions[0]], (knob, short, retried, first)
            for f in others:
                assert got[f] is not None and got[f].tobytes() == ref.rows[f], (knob, short, "retry", f)
    finally:
        h.close()


def planes_above(demands, capacity, bit):
    """the planes of the loaded frame whose demand the capacity does not hold -> {offset in the frame: bit}"""
    return {t: bit for t, d in enumerate(demands) if d > capacity}


def demand(rig, loaded, at=1):
    """the loaded frame's plane counters on the generous handle, one dict per plane of the frame"""
    ref = rig.generous(batch_of(loaded, at, rig.batch))
    return ref.planes[at * rig.planes:(at + 1) * rig.planes]


# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_generous_handle_is_held_to_the_oracle(env):
    """the reference side of every comparison below: kept borders point for point, candidate count"""
    for name, (h, w) in (("sq10", (440, 520)), ("sq8", (360, 520)), ("mixed", (480, 640))):
        want = L.kept_borders(L.plane_of(frame(name, h, w)))
        ncand = len(L.oracle_candidates(frame(name, h, w)))
        for rig, names, at in ((env.rig(w, h), batch_of(name, 1), 1), (env.rig(w, h, 1), [name], 0)):
            ref = rig.generous(names)
            borders, cands = ref.seen[at]
            assert same_borders(borders, want), (name, rig.batch, len(borders), len(want))
            assert len(cands[0]) == ncand, (name, rig.batch, len(cands[0]), ncand)
            d = ref.planes[at]
            lo, hi = L.pool_bounds(want)
            assert d["contours"] + d["late_contours"] == len(want) and lo <= d["points"] <= hi, (name, d, lo, hi)
    rig = env.rig(520, 440, 3, 3)
    ref = rig.generous(batch_of("sq10", 1))
    assert len(ref.seen[1][1][0]) == len(L.oracle_candidates(frame("sq10", 440, 520), thres_range=1)) == 120
    assert [p["contours"] for p in ref.planes[3:6]] == [120, 120, 120]


@pytest.mark.parametrize("name, h, w, kind", [("checker", 96, 128, 1), ("dominoes", 136, 256, 0)], ids=["hole half", "outer half"])
def test_start_list_halves(env, name, h, w, kind):
    """list 1: max(triggers_per_frame, 8192) / 2 start candidates of each kind a plane"""
    rig = env.rig(w, h, 3, 1, 128)
    want = starts_of(name, h, w)
    assert demand(rig, name)[0]["starts"] == want        # the counters are the demand: they equal the numpy reference
    D = want[kind]
    assert D > 4096 and want[1 - kind] < 4096
    check_list(rig, name, "triggers_per_frame", 2 * D, 2 * D - 2, TRIG)


def test_long_walk_rings(env):
    """list 2: max(long_walks_per_plane, 64) rings of each kind a plane; every 92-point border of the squares outlasts the 64-step leash"""
    rig = env.rig(520, 440)
    rings = demand(rig, "sq10")[0]["rings"]
    assert 64 < max(rings) <= 120 and min(rings) <= 120, rings       # at most the borders of a kind (120 start candidates, no false starts)
    check_list(rig, "sq10", "long_walks_per_plane", max(rings), max(rings) - 1, TRIG)


def test_descriptors_early(env):
    """list 3: contours_per_frame descriptors a plane"""
    check_list(env.rig(520, 440), "sq10", "contours_per_frame", 120, 119, CDESC)


@pytest.mark.parametrize("runner", ["run", "run_lane"], ids=["synchronous", "lane"])
def test_descriptors_early_and_late_share_the_array(env, runner):
    """list 4: a lane keeps its late borders (above 960 points) from the top of the plane's descriptor array downwards, in the room the early ones
    left: 70 + 2 fit 72 slots, and 71 slots report on that frame alone. The synchronous call keeps all 72 in one list."""
    rig = env.rig(640, 480)
    d = demand(rig, "mixed")[0]
    assert d["contours"] + d["late_contours"] == 72
    check_list(rig, "mixed", "contours_per_frame", 72, 71, CDESC, runner=runner, retry=runner == "run")
    if runner == "run_lane":
        h = rig.handle(contours_per_frame=72)
        try:
            r = rig.run_lane(h, batch_of("mixed", 1), look=[])
            assert (r.planes[1]["contours"], r.planes[1]["late_contours"]) == (70, 2), r.planes[1]
        finally:
            h.close()


@pytest.mark.parametrize("name, h, w", [("sq10", 440, 520), ("mixed", 480, 640)])
def test_points_pool(env, name, h, w):
    """list 5: points_per_frame pool words a plane, the checkpoints of a border in front of its points. One word short, the border that does not fit
    is listed with no points and ignored downstream: the frame's remaining borders are the reference's, and no other bit is set."""
    rig = env.rig(w, h)
    want = L.kept_borders(L.plane_of(frame(name, h, w)))
    lo, hi = L.pool_bounds(want)
    D = demand(rig, name)[0]["points"]
    assert lo <= D <= hi, (lo, D, hi)
    check_list(rig, name, "points_per_frame", D, D - 1, POOL)
    hd = rig.handle(points_per_frame=D - 1)
    try:
        r = rig.run(hd, batch_of(name, 1), look=[1])
        assert r.status == POOL and r.planes[1]["contours"] == len(want)
        got = r.seen[1][0]
        assert 0 < len(got) < len(want)
        if name == "sq10":
            assert len(got) == len(want) - 1                  # equal borders: exactly one does not fit
        keys = {(c["hole"], c["pts"].tobytes()) for c in want}
        assert all(len(c["pts"]) > 0 and (c["hole"], c["pts"].tobytes()) in keys for c in got)
    finally:
        hd.close()


def test_quads_of_all_planes(env):
    """list 6: min(2 * candidates_per_frame, 512) quads a frame, all planes together. On three planes the squares give 360 quads and 120 candidates:
    candidates_per_frame = 180 fits, 179 reports QUAD (the candidate list itself is nowhere near full). With one plane the squares have as many
    quads as candidates, so the candidate list fills first (test_candidates)."""
    rig = env.rig(520, 440, 3, 3)
    check_list(rig, "sq10", "candidates_per_frame", 180, 179, QUAD, plane_bits="any")


def test_quads_of_one_plane(env):
    """list 6 on one plane: a 28-pixel square keeps its outer and its hole border (108 and 88 points), so the frame has 240 quads for 120
    candidates: candidates_per_frame = 120 fills the quad list (240) and the candidate list (120) exactly; at 119 two quads are lost. If they belong
    to one square 119 candidates remain and fit, otherwise 120 remain and the candidate list, one short as well, reports too: QUAD always, CAND
    possibly, on the frame's only plane, and nothing else."""
    rig = env.rig(520, 440)
    want = L.kept_borders(L.plane_of(frame("sq28", 440, 520)))
    assert len(want) == L.quad_demand(want) == 240 and len(L.oracle_candidates(frame("sq28", 440, 520))) == 120
    ref = rig.generous(batch_of("sq28", 1))
    assert same_borders(ref.seen[1][0], want) and len(ref.seen[1][1][0]) == 120
    check_list(rig, "sq28", "candidates_per_frame", 120, 119, QUAD, allowed=CAND)


def test_descriptors_outer_and_hole(env):
    """list 3 with both kinds of border in the array: 240 descriptors"""
    check_list(env.rig(520, 440), "sq28", "contours_per_frame", 240, 239, CDESC)


def test_more_than_512_quads_is_loud(env):
    """the hard limit: 576 quads of one frame on three planes fit no handle; the largest one reports QUAD and gives up that frame only"""
    rig = env.rig(616, 472, 3, 3)
    ref = rig.generous(["m1", "m3", "m2"])
    h = rig.handle(scale=4)
    try:
        assert rig.limits(4).candidates_per_frame == 512
        r = rig.run(h, ["m1", "many", "m2"], look=[0, 2])
        check_short(rig, r, ref, 1, QUAD, "any", "576 quads")
        assert sum(p["contours"] for p in r.planes[3:6]) == 576
    finally:
        h.close()


def test_candidates(env):
    """list 7: candidates_per_frame candidates a frame; the bit goes to the frame's first plane"""
    check_list(env.rig(520, 360), "sq8", "candidates_per_frame", 96, 95, CAND)


def test_flat_decode_list_of_a_batch(env):
    """list 8: max(F * min(candidates_per_frame, 96), candidates_per_frame) entries a batch. Two frames at candidates_per_frame = 128: 192 entries
    hold one loaded frame (120) and not two (240); a frame is complete or given up, never cut short."""
    capi, rig = env.capi, env.rig(520, 440, 2)
    h = rig.handle(candidates_per_frame=128)
    try:
        ref = rig.generous(["sq10", "blank"])
        r = rig.run(h, ["sq10", "blank"])
        assert r.rc == capi.OK and r.status == 0
        for f in (0, 1):
            same_frame(r, ref, f, "120 of 192")
        assert len(r.seen[0][1][0]) == 120
        one = ref                                             # either frame of the pair, where it is kept, is the single loaded frame's result
        r = rig.run(h, ["sq10", "sq10"], look=[])
        assert r.rc == capi.E_OVERFLOW and r.status == CAND, (r.rc, r.status)
        assert sorted(int(v) for v in r.n) == [-1, one.n[0]], r.n
        kept = int(np.argmax(r.n))
        assert r.rows[kept] == one.rows[0]
        assert [p["status"] for p in r.planes] == ([0, CAND] if kept == 0 else [CAND, 0])
        assert same_borders(h.debug_contours(kept), one.seen[0][0])
        got = h.debug_candidates(kept)
        assert len(got[0]) == 120 and all(np.array_equal(x, y) for x, y in zip(got, one.seen[0][1]))
        got, retried, first = h.detect_batch_host_tolerant(rig.frames(["sq10", "sq10"]), cap=CAP)
        assert retried == 1 and got[0].tobytes() == got[1].tobytes() == one.rows[0]
    finally:
        h.close()


def test_one_frame_fills_its_own_candidate_list(env):
    """A one-frame handle with default limits (256 candidates a frame) on a sheet of 120 squares: the flat list used to hold 96 entries whatever
    candidates_per_frame said, and the retry, a one-frame handle too, could not help."""
    capi = env.capi
    g = frame("sq10", 440, 520)
    ref = env.rig(520, 440, 2).generous(["sq10", "blank"])
    h = capi.Handle(520, 440, max_batch=1)
    try:
        for _ in range(3):                                    # eager, graph capture, graph replay
            assert h.detect(g, cap=CAP).tobytes() == ref.rows[0]
            assert h.debug_counters()["status"] == 0
        got = h.debug_candidates(0)
        assert len(got[0]) == 120 and all(np.array_equal(x, y) for x, y in zip(got, ref.seen[0][1]))
    finally:
        h.close()


@pytest.mark.parametrize("contours", ["walkers", None], ids=["walkers", "segments"])
def test_one_frame_handle_after_an_overflow(env, contours):
    """D on a one-frame handle: detect(loaded) raises, then three detect(marked) - eager, graph capture, graph replay - return the same bytes, the
    generous handle's"""
    capi = env.capi
    rig = env.rig(520, 440, 1, 1, None, contours)
    ref = rig.generous(["m1"])
    h = rig.handle(contours_per_frame=119)
    try:
        with pytest.raises(capi.ArucoHipError) as e:
            h.detect(frame("sq10", 440, 520), cap=CAP)
        assert e.value.code == capi.E_OVERFLOW
        assert h.debug_counters()["status"] == CDESC and h.debug_plane_counters(0)["status"] == CDESC
        assert h.debug_plane_counters(0)["segments"] == (contours is None)
        for _ in range(3):
            assert h.detect(frame("m1", 440, 520), cap=CAP).tobytes() == ref.rows[0]
            assert h.debug_counters()["status"] == 0
    finally:
        h.close()


@pytest.mark.parametrize("contours", [None, "segments"], ids=["walkers", "segments"])
@pytest.mark.parametrize("which", ["descriptors", "pool"])
def test_per_plane_lists_on_three_planes(env, contours, which):
    """B and C with three threshold planes a frame (windows 7, 7, 9: every plane of the squares keeps 120 borders), lists 3 and 5 and, on the segment
    pipeline, list 10: the loaded frame's own planes are neighbours of each other, and plane p of frame f is plane 3 f + p of the batch, so a guard,
    a clamp or a flag that takes the frame for the plane shows. Each plane's TC_STATUS is asserted: the bit on every plane of the loaded frame whose
    demand the capacity does not hold, 0 on every plane of the neighbours."""
    rig = env.rig(520, 440, 3, 3, None, contours)
    d = demand(rig, "sq10")
    assert [p["contours"] for p in d] == [120, 120, 120] and all(p["segments"] == (contours is not None) for p in d)
    if which == "descriptors":
        check_list(rig, "sq10", "contours_per_frame", 120, 119, CDESC, plane_bits={0: CDESC, 1: CDESC, 2: CDESC})
    else:
        for w, p in zip((7, 7, 9), d):
            lo, hi = L.pool_bounds(L.kept_borders(L.plane_of(frame("sq10", 440, 520), p1=w)))
            assert lo <= p["points"] <= hi, (w, lo, p["points"], hi)
        D = max(p["points"] for p in d)
        bits = planes_above([p["points"] for p in d], D - 1, POOL)
        assert bits
        check_list(rig, "sq10", "points_per_frame", D, D - 1, POOL, plane_bits=bits)


def test_rings_on_three_planes(env):
    """list 2 on three planes a frame"""
    rig = env.rig(520, 440, 3, 3)
    rings = [max(p["rings"]) for p in demand(rig, "sq10")]
    assert all(64 < r <= 120 for r in rings), rings
    D = max(rings)
    check_list(rig, "sq10", "long_walks_per_plane", D, D - 1, TRIG, plane_bits=planes_above(rings, D - 1, TRIG))


def test_start_list_on_three_planes(env):
    """list 1 on three planes a frame: the fixed threshold's range gives levels 127, 128 and 129, the same plane of a 0 / 255 checkerboard three
    times, so every plane of the loaded frame asks for 5766 hole starts"""
    rig = env.rig(128, 96, 3, 3, 128)
    want = starts_of("checker", 96, 128)
    assert [p["starts"] for p in demand(rig, "checker")] == [want] * 3
    D = want[1]
    check_list(rig, "checker", "triggers_per_frame", 2 * D, 2 * D - 2, TRIG, plane_bits={0: TRIG, 1: TRIG, 2: TRIG})


def test_lane_reports_like_the_synchronous_call(env):
    """list 3 one short through submit / wait: the same counts, status words and neighbour bytes as the synchronous call"""
    capi, rig = env.capi, env.rig(520, 440)
    names = batch_of("sq10", 1)
    h = rig.handle(contours_per_frame=119)
    try:
        a = rig.run(h, names, look=[0, 2])
        b = rig.run_lane(h, names, look=[0, 2])
        assert a.rc == b.rc == capi.E_OVERFLOW and a.status == b.status == CDESC
        assert list(a.n) == list(b.n) and a.n[1] == -1
        assert [p["status"] for p in a.planes] == [p["status"] for p in b.planes] == [0, CDESC, 0]
        ref = rig.generous(names)
        for f in (0, 2):
            same_frame(b, ref, f, "lane")
            assert a.rows[f] == b.rows[f]
    finally:
        h.close()


def test_segment_descriptors_and_pool(env):
    """list 10: the segment pipeline's own guards of the descriptor array and the pool (a border takes its points alone there)"""
    rig = env.rig(520, 440, 3, 1, None, "segments")
    d = demand(rig, "sq10")[0]
    assert d["segments"] and d["contours"] == 120 and d["points"] == 120 * 92
    check_list(rig, "sq10", "contours_per_frame", 120, 119, CDESC)
    check_list(rig, "sq10", "points_per_frame", d["points"], d["points"] - 1, POOL)


# ---- last: the kernels behind the waypoint list run on a graph that was cut short --------------------------------------------------------------
def waypoint_demand(rig, names, at):
    d = rig.generous(names).planes[at]
    assert d["segments"] and d["raw"] >= 240, d                 # at least the 120 + 120 start candidates of the squares
    return d["raw"]


@pytest.mark.parametrize("grid", ["8", "32"])
def test_waypoint_list_one_frame(env, grid):
    """list 9, one frame per call: triggers_per_frame waypoint records a plane, no minimum. At D the result is the generous handle's; at D - 1 and
    at D / 2 the call returns ARUCOHIP_E_OVERFLOW - and returns - with the trigger bit, possibly the segment-link bit, and nothing else."""
    capi = env.capi
    rig = env.rig(520, 440, 1, 1, None, None, grid)
    D = waypoint_demand(rig, ["sq10"], 0)
    ref, after = rig.generous(["sq10"]), rig.generous(["m1"])
    h = rig.handle(triggers_per_frame=D)
    try:
        r = rig.run(h, ["sq10"])
        assert r.rc == capi.OK and r.status == 0 and r.planes[0]["raw"] == D
        same_frame(r, ref, 0, ("waypoints", D))
    finally:
        h.close()
    for cap in (D - 1, D // 2):
        h = rig.handle(triggers_per_frame=cap)
        try:
            r = rig.run(h, ["sq10"], look=[])
            assert r.rc == capi.E_OVERFLOW and r.n[0] == -1, (cap, r.rc, r.n)
            assert r.status & TRIG and not r.status & ~(TRIG | SEGMENT), (cap, r.status)
            assert r.planes[0]["status"] == r.status and r.planes[0]["raw"] == D
            r = rig.run(h, ["m1"])
            assert r.rc == capi.OK and r.status == 0
            same_frame(r, after, 0, ("waypoints", cap, "afterwards"))
        finally:
            h.close()


@pytest.mark.parametrize("grid", ["8", "32"])
def test_waypoint_list_batch(env, grid):
    """list 9 in a batch of three on the segment pipeline: the neighbours of the frame whose graph was cut short keep their bytes"""
    capi = env.capi
    rig = env.rig(520, 440, 3, 1, None, "segments", grid)
    names = batch_of("sq10", 1)
    D = waypoint_demand(rig, names, 1)
    ref = rig.generous(names)
    assert max(ref.planes[0]["raw"], ref.planes[2]["raw"]) < D // 2
    for cap in (D, D - 1, D // 2):
        h = rig.handle(triggers_per_frame=cap)
        try:
            r = rig.run(h, names, look=[0, 2] if cap < D else None)
            if cap == D:
                assert r.rc == capi.OK and r.status == 0
                for f in range(3):
                    same_frame(r, ref, f, ("waypoints", cap))
                continue
            assert r.rc == capi.E_OVERFLOW and list(r.n < 0) == [False, True, False], (cap, r.rc, r.n)
            assert r.status & TRIG and not r.status & ~(TRIG | SEGMENT), (cap, r.status)
            assert [p["status"] for p in r.planes] == [0, r.status, 0]
            for f in (0, 2):
                same_frame(r, ref, f, ("waypoints", cap))
            got, retried, _ = h.detect_batch_host_tolerant(rig.frames(names), cap=CAP)
            assert retried == 1 and all(got[f].tobytes() == ref.rows[f] for f in range(3))
        finally:
            h.close()


def test_waypoint_list_on_three_planes(env):
    """list 9 with three planes a frame: one record short of the largest plane's demand, the planes that ask for that many report - the trigger bit,
    possibly the segment-link bit - and the neighbours' planes stay clean"""
    rig = env.rig(520, 440, 3, 3, None, "segments")
    raw = [p["raw"] for p in demand(rig, "sq10")]
    assert all(r >= 240 for r in raw), raw
    D = max(raw)
    check_list(rig, "sq10", "triggers_per_frame", D, D - 1, TRIG, plane_bits=planes_above(raw, D - 1, TRIG), allowed=SEGMENT)

