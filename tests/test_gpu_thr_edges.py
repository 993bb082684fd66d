"""The threshold stage (k_threshold.hip, chosen per plane by thr_plan.h) against tests/thr_ref.py in every variant the plan can choose: the three
kernel families, the three segment heights, the byte image and its lazy form (bit tiles + four border lines + non-empty-tile bitmap), one strip to
three, every block size, the plan's boundaries on C, FIXED, a threshold range, strides and base addresses, one handle across geometries, timing on,
and the production path. Everything is integer data and every assertion is equality.

Each case runs arucohip_debug_threshold_batch on device frames (the threshold stage and nothing behind it: noise and checkerboards would overflow
the contour lists), asserts the plan arucohip_debug_threshold_plan reports, and then for every frame and plane: bytes == thr_ref, tiles ==
tiles_of(thr_ref) with pad tiles and pad bits, and the bitmap == bitmap_of on every tile row candidates_sparse_kernel reads. That kernel reads the
words of tile rows 0 .. tiles_y - 2 (k_contours.hip, row_words: `ty < nty`): the real rows and, for frames lower than 17 pixels, the extra row
tiles_y()'s floor of 4 adds, which must be zero. It never reads the last (pad) row's words, so they are left out here."""
import ctypes as C

import numpy as np
import pytest

from tests import thr_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    from aruco_amd import capi

    assert torch.cuda.is_available()
    capi.load()
    return {"capi": capi, "torch": torch}


def _handle(capi, W, H, nframes, planes=1, params=None, lean=True):
    """A handle sized to the case (the library's floor is 32 x 32). lean: short contour lists, for handles that only threshold."""
    lim = capi.Limits()
    capi.load().arucohip_default_limits(C.byref(lim), max(W, 32), max(H, 32), nframes)
    lim.max_thres_planes = planes
    if lean:
        lim.triggers_per_frame, lim.contours_per_frame, lim.points_per_frame, lim.long_walks_per_plane = 8192, 256, 8192, 64
    return capi.Handle(max(W, 32), max(H, 32), max_batch=nframes, params=params, limits=lim)


def _params(capi, block=7, c=7.0, rng=0, fixed=None):
    p = capi.default_params()
    p.thres_param1, p.thres_param2, p.thres_param1_range = float(block), float(c), rng
    if fixed is not None:
        p.thres_method, p.thres_param1 = capi.THRES_FIXED, float(fixed)
    return p


def _upload(torch, frames, row_stride=None, frame_stride=None, offset=0):
    """The frames in device memory with the given strides, `offset` bytes into an allocation whose every other byte is hostile (random).
    Returns (tensor to keep alive, address of the first frame)."""
    nf, H, W = frames.shape
    rs = W if row_stride is None else row_stride
    fs = rs * H if frame_stride is None else frame_stride
    if rs == W and fs == W * H and offset == 0:
        t = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
        return t, t.data_ptr()
    buf = np.random.RandomState(nf * 7 + rs).randint(0, 256, size=offset + nf * fs + 64).astype(np.uint8)
    for f in range(nf):
        for y in range(H):
            at = offset + f * fs + y * rs
            buf[at:at + W] = frames[f, y]
    t = torch.from_numpy(buf).cuda()
    return t, t.data_ptr() + offset


def _reference(frames, blocks, c, fixed=None):
    """[planes][frames][H][W] thresholded bytes of the reference, a few frames at a time"""
    out = []
    for b in blocks:
        if fixed is not None:
            out.append(thr_ref.fixed(frames, fixed))
        else:
            out.append(np.concatenate([thr_ref.adaptive(frames[i:i + 16], b, c) for i in range(0, len(frames), 16)]))
    return out


def _compare(h, case, frames, ref):
    """Every plane of every frame of the handle's last batch against ref [planes][frames][H][W]."""
    nf, H, W = frames.shape
    for t, rt in enumerate(ref):
        tiles_ref = np.concatenate([thr_ref.tiles_of(rt[i:i + 64]) for i in range(0, nf, 64)])
        bits_ref = thr_ref.bitmap_of(tiles_ref, W)
        for f in range(nf):
            by, tl, tb = h.debug_threshold_plane(f, t, W, H)
            if not np.array_equal(by, rt[f]):
                x, y = thr_ref.first_diff(by, rt[f])
                pytest.fail("%s frame %d plane %d: bytes differ first at (x %d, y %d): %d, reference %d; %d pixels differ" %
                            (case, f, t, x, y, by[y, x], rt[f][y, x], int((by != rt[f]).sum())))
            if not np.array_equal(tl, tiles_ref[f]):
                x, y = thr_ref.first_diff(tl, tiles_ref[f])
                pytest.fail("%s frame %d plane %d: tiles differ first at tile (x %d, y %d): %#018x, reference %#018x" %
                            (case, f, t, x, y, int(tl[y, x]), int(tiles_ref[f][y, x])))
            rows = tl.shape[0] - 1
            if not np.array_equal(tb[:rows], bits_ref[f][:rows]):
                x, y = thr_ref.first_diff(tb[:rows], bits_ref[f][:rows])
                pytest.fail("%s frame %d plane %d: bitmap differs first at word (x %d, y %d): %#018x, reference %#018x" %
                            (case, f, t, x, y, int(tb[y, x]), int(bits_ref[f][y, x])))


def _check_plan(h, case, planes, strips, no_bytes):
    """planes: one dict per plane with the keys that matter for it; returns the reported plan"""
    pl = h.debug_threshold_plan()
    print(case, pl)
    assert len(pl["planes"]) == len(planes), (case, pl)
    for t, want in enumerate(planes):
        got = pl["planes"][t]
        for k, v in want.items():
            assert got[k] == v, (case, "plane %d" % t, k, got, want)
    assert pl["strips"] == strips and pl["no_bytes"] == no_bytes, (case, pl)
    assert pl["bitmap_pass"] == any(p["family"] == "strip" for p in pl["planes"]), (case, pl)
    return pl


def _run(env, case, frames, planes, block=7, c=7.0, rng=0, blocks=None, fixed=None, want_bytes=False, no_bytes=None, h=None, **upload):
    """One case on a handle of its own (or on h): run, assert the plan, compare everything."""
    capi, torch = env["capi"], env["torch"]
    nf, H, W = frames.shape
    blocks = blocks or [block]
    own = h is None
    if own:
        h = _handle(capi, W, H, nf, len(blocks), _params(capi, block, c, rng, fixed))
    else:
        h.set_params(_params(capi, block, c, rng, fixed))
    try:
        keep, ptr = _upload(torch, frames, **upload)
        h.debug_threshold_batch(ptr, nf, W, H, upload.get("row_stride"), upload.get("frame_stride"), want_bytes=want_bytes)
        if no_bytes is None:
            no_bytes = not want_bytes and fixed is None and all(p["family"] != "strip" for p in planes)
        _check_plan(h, case, planes, (W + 1023) // 1024, no_bytes)
        _compare(h, case, frames, _reference(frames, blocks, c, fixed))
        del keep
    finally:
        if own:
            h.close()


def _p16_holds(block, c):
    """the packed 16-bit compare's bound as the issue states it: (256 + |C|) b^2 + b^2 / 2 < 32768"""
    n = block * block
    return (256 + abs(int(np.floor(c)))) * n + n // 2 < 32768


# ---- segment heights

@pytest.mark.parametrize("want_bytes", [False, True], ids=["lazy", "bytes"])
@pytest.mark.parametrize("block", [7, 3, 5, 9], ids=["eo", "wideR1", "wideR2", "wideR4"])
@pytest.mark.parametrize("seg", [16, 32, 128])
def test_segment_heights(env, seg, block, want_bytes):
    """48 pixels wide, one strip; heights around one and two segments: a last segment of one row that is the image's last row, (H - 1) & 7 of
    0, 6 and 7, heights that are no multiple of 4 (the border columns go out four rows at a time); and at H = 129 the frame counts on both sides
    of the rule's two edges."""
    family = "eo" if block == 7 else "wide"
    for H, nf in thr_ref.SEG_HEIGHTS[seg]:
        nf = nf or thr_ref.frames_for_seg(thr_ref.SEG_W, H, seg)
        assert thr_ref.seg_rule(thr_ref.SEG_W, H, nf) == seg
        frames = thr_ref.batch("blocky", nf, H, thr_ref.SEG_W, 100 + seg + H)
        _run(env, "seg%d H %d frames %d block %d %s" % (seg, H, nf, block, "bytes" if want_bytes else "lazy"), frames,
             [{"family": family, "R": block // 2, "seg": seg}], block=block, want_bytes=want_bytes)


# ---- strips and the eo kernel's 1-D grid

@pytest.mark.parametrize("block", [7, 5], ids=["eo", "wide"])
@pytest.mark.parametrize("geom", thr_ref.STRIP_GEOMS, ids=lambda g: "%dx%dx%d" % g[:3])
def test_strips_and_the_xcd_unpacking(env, geom, block):
    """Two and three strips with workgroup counts that are no multiple of 8 x strips (30 -> 32, 390 -> 400, 516 -> 528) and frames that all
    differ: a strip, segment or frame taken for another shows. Block 5: the wide kernel's 3-D grid on the same geometry."""
    W, H, nf, seg = geom
    strips = (W + 1023) // 1024
    groups = strips * (-(-H // seg)) * nf
    assert groups % (8 * strips) != 0 and thr_ref.seg_rule(W, H, nf) == seg
    frames = thr_ref.batch("blocky", nf, H, W, 200 + seg)
    _run(env, "strips %dx%dx%d block %d" % (W, H, nf, block), frames, [{"family": "eo" if block == 7 else "wide", "R": block // 2, "seg": seg}], block=block)


# ---- widths

@pytest.mark.parametrize("block", [7, 3], ids=["eo", "wideR1"])
@pytest.mark.parametrize("seg", [128, 16])
@pytest.mark.parametrize("W", thr_ref.WIDTHS)
def test_widths(env, W, seg, block):
    """One lane that is both edges of the image (16), lane 63 right of the image, exact strips (1024, 2048) and a last strip of one lane
    (1040, 2064); the border lines set to 0, 255 and alternating against the interior."""
    H = thr_ref.WIDTH_H
    nf = 3 if seg == 16 else thr_ref.frames_for_seg(W, H, 128)
    assert thr_ref.seg_rule(W, H, nf) == seg
    frames = thr_ref.batch("lines", nf, H, W, 300 + W)
    _run(env, "width %d seg %d block %d" % (W, seg, block), frames, [{"family": "eo" if block == 7 else "wide", "R": block // 2, "seg": seg}], block=block)


# ---- every block size

def _plane_for(W, block, c):
    """what the plan must say on 272 (16-byte rows), 268 (dword rows) and 267 (byte-wise rows) pixel wide frames"""
    R = block // 2
    if W % 16 == 0 and R <= 4 and _p16_holds(block, c):
        return {"family": "eo" if R == 3 and abs(int(np.floor(c))) <= 200 else "wide", "R": R}
    if W % 4 == 0:
        return {"family": "strip", "R": R, "fast": True, "p16": R <= 5 and _p16_holds(block, c)}
    return {"family": "strip", "R": R, "fast": False, "p16": False}


@pytest.mark.parametrize("block", list(range(3, 32, 2)))
@pytest.mark.parametrize("W", thr_ref.BLOCK_WIDTHS)
def test_every_block_size(env, W, block):
    """Blocks 3 .. 31 (the strip kernel's R = 1 .. 15) at four constants, on one handle per width and block."""
    capi = env["capi"]
    frames = thr_ref.batch("blocky", 3, thr_ref.BLOCK_H, W, 400 + W)
    want = _plane_for(W, block, 7.0)
    assert want["family"] == (("eo" if block == 7 else "wide") if W == 272 and block <= 9 else "strip")
    assert W != 268 or (want["fast"] and want["p16"] == (block <= 11))
    assert W != 267 or not (want["fast"] or want["p16"])
    h = _handle(capi, W, thr_ref.BLOCK_H, 3)
    try:
        for c in thr_ref.BLOCK_CS:
            _run(env, "block %d C %g width %d" % (block, c, W), frames, [want], block=block, c=c, h=h)
    finally:
        h.close()


# ---- the plan's boundaries on C

# on 16-byte rows; P16 of the strip kernel on dword rows
BOUNDARY_PLAN = {(9, 148): ("wide", True), (9, 149): ("strip", False), (11, 14): ("strip", True), (11, 15): ("strip", False), (7, 200): ("eo", True),
                 (7, 201): ("wide", True), (7, 412): ("wide", True), (7, 413): ("strip", False), (5, 300): ("wide", True), (3, 1000): ("wide", True),
                 (7, 1000): ("strip", False)}


@pytest.mark.parametrize("bc", thr_ref.BOUNDARY_CASES, ids=lambda bc: "b%d_C%g" % bc)
@pytest.mark.parametrize("W", thr_ref.BLOCK_WIDTHS)
def test_plan_boundaries_on_c(env, W, bc):
    """Both sides of the packed compare's bound for 9x9, 11x11 and 7x7, of the eo kernel's |C| <= 200 (with floor(-200.5) = -201 outside), and
    constants far beyond; on inputs that bring g - mean to every value down to -250 and up to +250, all 0, all 255 and the checkerboard."""
    block, c = bc
    key = (block, 201 if c == -200.5 else abs(int(c)))
    family, p16 = BOUNDARY_PLAN[key]
    assert p16 == _p16_holds(block, c)
    if W == 272:
        want = {"family": family, "R": block // 2}
        if family == "strip":
            want.update(fast=True, p16=p16 and block <= 11)
    elif W == 268:
        want = {"family": "strip", "R": block // 2, "fast": True, "p16": p16}
    else:
        want = {"family": "strip", "R": block // 2, "fast": False, "p16": False}
    frames = thr_ref.batch("mix", 5, thr_ref.BLOCK_H, W, 500 + W)
    _run(env, "boundary block %d C %g width %d" % (block, c, W), frames, [want], block=block, c=c)


# ---- FIXED

@pytest.mark.parametrize("W", thr_ref.BLOCK_WIDTHS)
def test_fixed_thresholds(env, W):
    """cv::threshold(BINARY_INV) below, at and beyond the grey range; the bitmap comes from tile_bitmap_kernel."""
    capi = env["capi"]
    frames = thr_ref.batch("levels", 3, thr_ref.BLOCK_H, W, 700 + W)
    h = _handle(capi, W, thr_ref.BLOCK_H, 3)
    try:
        for thr in thr_ref.FIXED_THRS:
            _run(env, "fixed %g width %d" % (thr, W), frames, [{"family": "strip", "R": 0, "fast": W % 4 == 0, "p16": False}], fixed=thr, h=h)
    finally:
        h.close()


# ---- threshold range

@pytest.mark.parametrize("geom", thr_ref.RANGE_GEOMS, ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("rc", thr_ref.RANGE_CASES, ids=lambda rc: "p%d_r%d" % rc[:2])
def test_threshold_range_every_plane(env, rc, geom):
    """Every plane of a range, not only the middle one: 7, 7, 9 stay lazy; 5 .. 13 and 7 .. 15 hold strip planes, which force the byte image, so the
    eo and wide kernels write bytes inside a batch."""
    p1, r, blocks = rc
    W, H = geom
    planes = [_plane_for(W, b, 7.0) for b in blocks]
    assert [p["family"] for p in planes] == {(7, 1): ["eo", "eo", "wide"], (7, 2): ["wide", "eo", "wide", "strip", "strip"],
                                             (9, 2): ["eo", "wide", "strip", "strip", "strip"]}[(p1, r)]
    for p in planes:
        if p["family"] != "strip":
            p["seg"] = 16
    frames = thr_ref.batch("blocky", 3, H, W, 600 + W)
    _run(env, "range p1 %d r %d %dx%d" % (p1, r, W, H), frames, planes, block=p1, rng=r, blocks=blocks)


# ---- strides and base address

@pytest.mark.parametrize("offset", [0, 16, 4, 1])
@pytest.mark.parametrize("extra", [0, 4096], ids=["tight", "gap"])
@pytest.mark.parametrize("stride", [272, 288, 276])
def test_strides_and_base_address(env, stride, extra, offset):
    """Rows and frames apart, the first frame 0, 16, 4 and 1 bytes into its allocation, hostile bytes in every gap: the plan falls from the eo
    kernel to the strip kernel with dword loads to the byte-wise one as thr_fast16 / thr_fast say, and the image stays the same."""
    W, H, nf, seed = thr_ref.STRIDE_CASE
    frames = thr_ref.batch("blocky", nf, H, W, seed)
    if stride % 16 == 0 and offset % 16 == 0:
        want = {"family": "eo", "R": 3, "seg": 16}
    elif stride % 4 == 0 and offset % 4 == 0:
        want = {"family": "strip", "R": 3, "fast": True, "p16": True}
    else:
        want = {"family": "strip", "R": 3, "fast": False, "p16": False}
    _run(env, "stride %d frame gap %d offset %d" % (stride, extra, offset), frames, [want], row_stride=stride, frame_stride=stride * H + extra, offset=offset)


# ---- one handle across geometries

def test_one_handle_across_geometries(env):
    """2064x136, 1024x64, 48x129 and 2064x136 again on one handle, lazy and with bytes in turn, then 48x16: pad tiles and pad bits are zero
    after every change, and so are the bitmap words of the last step's third tile row, which the larger geometry before it left set and which
    only the clearing at a change of geometry resets."""
    capi = env["capi"]
    h = _handle(capi, 2064, 136, thr_ref.SHARED_FRAMES)
    try:
        for i, (W, H) in enumerate(thr_ref.SHARED_STEPS):
            frames = thr_ref.batch("blocky", thr_ref.SHARED_FRAMES, H, W, thr_ref.SHARED_SEED + i)
            _run(env, "shared handle step %d %dx%d" % (i, W, H), frames, [{"family": "eo", "R": 3, "seg": 16}], want_bytes=i % 2 == 1, h=h)
    finally:
        h.close()


# ---- timing on

@pytest.mark.parametrize("block", thr_ref.TIMING_CASE[4], ids=["eo", "wide"])
def test_timing_on_changes_nothing_and_counts_the_launches(env, block):
    """enable_timing(True) arms the per-wave clock stamps of the 16-pixel-per-lane kernels: the same bytes, tiles and bitmap as without, at 128 rows
    per wave, and threshold_exec_ms counts one span per launch. No time is asserted."""
    capi, torch = env["capi"], env["torch"]
    _, H, nf, seed, _ = thr_ref.TIMING_CASE
    frames = thr_ref.batch("blocky", nf, H, thr_ref.SEG_W, seed + block)
    ref = _reference(frames, [block], 7.0)
    want = [{"family": "eo" if block == 7 else "wide", "R": block // 2, "seg": 128}]
    h = _handle(capi, thr_ref.SEG_W, H, nf, 1, _params(capi, block))
    try:
        keep, ptr = _upload(torch, frames)
        h.debug_threshold_batch(ptr, nf, thr_ref.SEG_W, H)
        _check_plan(h, "untimed block %d" % block, want, 1, True)
        _compare(h, "untimed block %d" % block, frames, ref)
        plain = [h.debug_threshold_plane(f, 0, thr_ref.SEG_W, H) for f in (0, nf // 2, nf - 1)]
        h.enable_timing(True)
        for launches in (1, 2, 3):
            h.debug_threshold_batch(ptr, nf, thr_ref.SEG_W, H)
            assert h.threshold_exec_ms()[1] == launches
        _check_plan(h, "timed block %d" % block, want, 1, True)
        _compare(h, "timed block %d" % block, frames, ref)
        for k, f in enumerate((0, nf // 2, nf - 1)):
            assert all(np.array_equal(a, b) for a, b in zip(plain[k], h.debug_threshold_plane(f, 0, thr_ref.SEG_W, H)))
        h.enable_timing(False)
        del keep
    finally:
        h.close()


# ---- the production path

@pytest.mark.parametrize("geom", thr_ref.PRODUCTION_GEOMS, ids=lambda g: "%dx%dx%d" % g[:3])
def test_the_production_path_plans_the_same(env, geom):
    """detect_batch on device frames, not the debug call: tame frames (16-pixel squares, noise below C) keep the contour lists far from their limits;
    the batch's status is clean, the plan its threshold launch executed is the one the debug call reported for the geometry, and every plane equals
    the reference."""
    capi, torch = env["capi"], env["torch"]
    W, H, nf, seg = geom
    frames = thr_ref.batch("tame", nf, H, W, thr_ref.PRODUCTION_SEED + W)
    ref = _reference(frames, [7], 7.0)
    want = [{"family": "eo", "R": 3, "seg": seg}]
    h = _handle(capi, W, H, nf, lean=False)
    try:
        keep, ptr = _upload(torch, frames)
        h.debug_threshold_batch(ptr, nf, W, H)
        dbg = _check_plan(h, "debug call %dx%dx%d" % (W, H, nf), want, (W + 1023) // 1024, True)
        out = torch.zeros((nf, 64 * capi.MARKER_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
        n = torch.zeros(nf, dtype=torch.int32, device="cuda")
        h.detect_batch_device(ptr, nf, W, H, out.data_ptr(), 64, n.data_ptr())
        h.batch_status()
        assert h.debug_threshold_plan() == dbg
        _compare(h, "detect_batch %dx%dx%d" % (W, H, nf), frames, ref)
        h.debug_cells(0)                                     # the batch decoded from cell medians ...
        h.debug_threshold_batch(ptr, nf, W, H)
        with pytest.raises(capi.ArucoHipError) as e:         # ... which the hook's batch does not have
            h.debug_cells(0)
        assert e.value.code == capi.E_INVALID
        del keep, out, n
    finally:
        h.close()


# ---- the hooks themselves

def test_the_hooks_refuse_and_get_thresholded_is_the_middle_plane(env):
    """No plan before a threshold launch; frames beyond the handle, a plane outside the range and a short plan array are refused and change
    nothing; arucohip_get_thresholded is plane nthr / 2; a host batch gives the same planes as the device batch; the single-frame graph's
    replay reports the plan of its capture."""
    capi, torch = env["capi"], env["torch"]
    W, H, nf, seed, blocks = thr_ref.HOOKS_CASE
    frames = thr_ref.batch("tame", nf, H, W, seed)
    h = _handle(capi, W, H, nf, len(blocks), _params(capi, 7, 7.0, 1), lean=False)
    L = h.L
    try:
        n = C.c_int(-1)
        out = np.zeros(5 * 16 + 3, np.int32)
        assert L.arucohip_debug_threshold_plan(h.h, out.ctypes.data_as(C.c_void_p), out.size, C.byref(n)) == capi.E_INVALID and n.value == 0
        h.debug_threshold_batch(frames)                       # host frames
        ref = _reference(frames, blocks, 7.0)
        _check_plan(h, "host batch", [{"family": "eo"}, {"family": "eo"}, {"family": "wide", "R": 4}], 1, True)
        _compare(h, "host batch", frames, ref)
        four = np.concatenate([frames, frames[:1]])
        assert L.arucohip_debug_threshold_batch(h.h, four.ctypes.data_as(C.c_void_p), 4, W, H, W, W * H, 0, 0) == capi.E_INVALID
        assert L.arucohip_debug_threshold_batch(h.h, frames.ctypes.data_as(C.c_void_p), 3, W, H, W - 1, W * H, 0, 0) == capi.E_INVALID
        assert L.arucohip_debug_threshold_batch(h.h, None, 3, W, H, W, W * H, 0, 0) == capi.E_INVALID
        assert L.arucohip_debug_threshold_plane(h.h, 0, 3, None, None, None) == capi.E_INVALID
        assert L.arucohip_debug_threshold_plane(h.h, 0, -1, None, None, None) == capi.E_INVALID
        assert L.arucohip_debug_threshold_plane(h.h, 3, 0, None, None, None) == capi.E_INVALID
        assert L.arucohip_debug_threshold_plan(h.h, out.ctypes.data_as(C.c_void_p), 17, C.byref(n)) == capi.E_CAPACITY and n.value == 3
        _compare(h, "after the refusals", frames, ref)
        for f in range(3):
            assert np.array_equal(h.thresholded(f, (H, W)), ref[1][f])
        keep, ptr = _upload(torch, frames)
        h.debug_threshold_batch(ptr, 3, W, H, want_bytes=True)
        _check_plan(h, "device batch with bytes", [{"family": "eo"}, {"family": "eo"}, {"family": "wide", "R": 4}], 1, False)
        _compare(h, "device batch with bytes", frames, ref)
        del keep
    finally:
        h.close()
    # one host frame per call: eager, eager again (capture), then replays
    h = _handle(capi, W, H, 1, lean=False)
    try:
        seen = []
        for k in range(4):
            h.detect(frames[0])
            seen.append(h.debug_threshold_plan())
            if k == 1:                                       # another plan in between: the replay must not report this one
                h.threshold(frames[1, :, :268], capi.THRES_ADPT, 11, 7.0)
                assert h.debug_threshold_plan()["planes"][0]["family"] == "strip"
        assert all(p == seen[0] for p in seen) and seen[0]["planes"][0]["family"] == "eo"
        by, tl, tb = h.debug_threshold_plane(0, 0, W, H)
        one = thr_ref.adaptive(frames[0], 7, 7.0)
        assert np.array_equal(by, one) and np.array_equal(tl, thr_ref.tiles_of(one))
    finally:
        h.close()
