"""tests/render_ref.py against what the rendering rule of include/arucohip.h implies: watertight shared edges, the top-left rule, order
independence, closed meshes under culling, facing, the trivial blends, and the footprint of plane compositing. No GPU.

The exact camera: rvec = 0, tvec = (0, 0, 1), fx = fy = 16 and an integer principal point. A vertex (x, y, 0) with x and y multiples of
1/256 then lands on the 1/16-pixel grid at (16 x + cx, 16 y + cy) with every intermediate exact, so nothing is knife-edge."""
import numpy as np
import pytest

from tests import composite_ref as cr
from tests import render_ref as rr

K_EXACT = np.array([[16, 0, 8], [0, 16, 6], [0, 0, 1]], np.float32)
FRONT = [(np.zeros(3), np.array([0.0, 0.0, 1.0]), 1.0)]
W, H = 40, 28


def frame(cn=3, seed=5):
    return np.random.RandomState(seed).randint(0, 256, (H, W) if cn == 1 else (H, W, 3)).astype(np.uint8)


def pixels(pts):
    """object-frame vertices (z = 0) of pixel positions under K_EXACT and FRONT"""
    p = np.asarray(pts, np.float64)
    return np.stack([(p[:, 0] - 8) / 16, (p[:, 1] - 6) / 16, np.zeros(len(p))], axis=1).astype(np.float32)


def cube():
    from aruco_amd import capi

    return capi.cube_mesh()


FACE_COLORS = np.repeat(np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [255, 0, 255], [0, 255, 255]], np.uint8), 2, axis=0)


def test_right_triangles_cover_the_top_left_set():
    v = pixels([(10, 8), (14, 8), (10, 12), (14, 12)])
    y, x = np.mgrid[0:H, 0:W]
    u, w = x - 10, y - 8
    upper = (u >= 0) & (w >= 0) & (u + w <= 3)            # top and left edges own their points, the hypotenuse does not
    lower = (u <= 3) & (w <= 3) & (u + w >= 4)            # here the hypotenuse is a left edge; the right and bottom edges own nothing
    for tri, want in (((0, 1, 2), upper), ((3, 2, 1), lower), ((0, 2, 1), upper), ((3, 1, 2), lower)):
        _, info = rr.render(frame(), FRONT, K_EXACT, None, v, [tri], flags=rr.UNLIT)
        assert (info["painted"] == want).all(), tri
        assert info["fragile_vertex"] == 0 and not info["fragile_depth"].any()


@pytest.mark.parametrize("quad", [
    [(10, 8), (14, 8), (10, 12), (14, 12)],               # the shared diagonal runs through pixel centres
    [(3.5, 2.25), (30.0625, 4.5), (5.75, 20.125), (33.5, 23.9375)],
    [(2, 2), (37, 3), (3, 25), (36, 24)],
])
def test_a_shared_edge_is_painted_once(quad):
    v, src = pixels(quad), frame()
    t1, t2 = [(0, 1, 2)], [(3, 2, 1)]
    kw = dict(flags=rr.UNLIT, opacity=128, color=(10, 250, 90))
    both, ib = rr.render(src, FRONT, K_EXACT, None, v, t1 + t2, **kw)
    first, i1 = rr.render(src, FRONT, K_EXACT, None, v, t1, **kw)
    second, i2 = rr.render(first, FRONT, K_EXACT, None, v, t2, **kw)
    assert not (i1["painted"] & i2["painted"]).any()                      # no pixel twice: at opacity 128 it would be blended twice
    assert ((i1["painted"] | i2["painted"]) == ib["painted"]).all()
    assert (second == both).all()
    if quad[0] == (10, 8):
        y, x = np.mgrid[0:H, 0:W]
        assert (ib["painted"] == ((x >= 10) & (x < 14) & (y >= 8) & (y < 12))).all()   # and no pixel of the union is missed
    else:
        # every pixel centre strictly inside the quadrilateral is painted
        p = np.asarray(quad, np.float64)[[0, 1, 3, 2]]
        y, x = np.mgrid[0:H, 0:W]
        inside = np.ones((H, W), bool)
        for (ax, ay), (bx, by) in zip(p, np.roll(p, -1, axis=0)):
            inside &= (bx - ax) * (y - ay) - (by - ay) * (x - ax) > 0
        assert inside.any() and (ib["painted"][inside]).all() and ib["painted"].sum() <= inside.sum() + 2 * (W + H)


POSES = [((0.4, -0.3, 0.2), (0.1, -0.05, 1.6)), ((-0.2, 0.5, -0.1), (-0.3, 0.1, 2.2)), ((2.6, 0.3, 0.2), (0.2, 0.1, 1.9))]
K_CAM = np.array([[30, 0, 19.3], [0, 31, 13.7], [0, 0, 1]], np.float32)


def test_order_of_triangles_and_instances_changes_nothing_off_the_fragile_pixels():
    v, t = cube()
    inst = [(np.array(r), np.array(tv), 0.5) for r, tv in POSES]
    src = frame()
    a, ia = rr.render(src, inst, K_CAM, None, v, t, colors=FACE_COLORS, flags=0)
    perm = np.random.RandomState(3).permutation(len(t))
    b, ib = rr.render(src, inst[::-1], K_CAM, None, v, t[perm], colors=FACE_COLORS[perm], flags=0)
    firm = ~(ia["fragile_depth"] | ib["fragile_depth"])
    assert ia["painted"].sum() > 100 and (ia["painted"] == ib["painted"]).all()
    assert (a[firm] == b[firm]).all() and firm.mean() > 0.999


@pytest.mark.parametrize("pose", POSES)
def test_a_closed_convex_cube_paints_the_same_with_and_without_culling(pose):
    v, t = cube()
    inst = [(np.array(pose[0]), np.array(pose[1]), 0.6)]
    src = frame()
    a, ia = rr.render(src, inst, K_CAM, None, v, t, colors=FACE_COLORS, flags=rr.CULL_BACK)
    b, ib = rr.render(src, inst, K_CAM, None, v, t, colors=FACE_COLORS, flags=0)
    assert ia["painted"].sum() > 50 and (ia["painted"] == ib["painted"]).all()
    firm = ~ib["fragile_depth"]
    assert (a[firm] == b[firm]).all()


def test_the_cube_is_made_of_outward_triangles_and_shows_its_near_face():
    v, t = cube()
    assert v.shape == (8, 3) and t.shape == (12, 3)
    c = v.mean(axis=0)
    for tri in t:
        a, b, d = v[tri]
        assert np.dot(np.cross(b - a, d - a), (a + b + d) / 3 - c) > 0
    # marker frame: z points out of the marker towards the camera. A pose that looks straight down on the marker (a half turn about x)
    # shows the face z = 1 (triangles 2, 3), never the face z = 0 that lies on the marker
    inst = [(np.array([np.pi, 0.0, 0.0]), np.array([0.0, 0.0, 3.0]), 1.0)]
    for flags in (rr.UNLIT, rr.UNLIT | rr.CULL_BACK):
        out, info = rr.render(np.zeros((H, W, 3), np.uint8), inst, K_CAM, None, v, t, colors=FACE_COLORS, flags=flags)
        cy, cx = int(round(float(K_CAM[1, 2]))), int(round(float(K_CAM[0, 2])))
        assert tuple(out[cy, cx]) == tuple(FACE_COLORS[2]) and info["owner"][cy, cx, 1] in (2, 3)
        assert not (out.reshape(-1, 3) == FACE_COLORS[0]).all(axis=1).any()


def test_lighting_scales_the_base_colour():
    v, t = cube()
    inst = [(np.array([np.pi, 0.0, 0.0]), np.array([0.0, 0.0, 3.0]), 1.0)]
    cy, cx = int(round(float(K_CAM[1, 2]))), int(round(float(K_CAM[0, 2])))
    black = np.zeros((H, W, 3), np.uint8)
    lit, _ = rr.render(black, inst, K_CAM, None, v, t, color=(100, 200, 50), ambient=64)          # the headlight meets the near face head on
    assert tuple(lit[cy, cx]) == (100, 200, 50)
    side, _ = rr.render(black, inst, K_CAM, None, v, t, color=(100, 200, 50), ambient=64, light=(1.0, 0.0, 0.0))   # ... a light from the side not at all
    assert tuple(side[cy, cx]) == tuple((np.array([100, 200, 50]) * 64 + 127) // 255)
    gray, _ = rr.render(np.zeros((H, W), np.uint8), inst, K_CAM, None, v, t, color=(100, 200, 50), ambient=64)
    assert gray[cy, cx] == rr.gray_of(100, 200, 50)


def test_opacity_zero_and_an_empty_mask_leave_the_frame():
    v, t = cube()
    inst = [(np.array(POSES[0][0]), np.array(POSES[0][1]), 0.6)]
    for cn in (1, 3):
        src = frame(cn)
        out, info = rr.render(src, inst, K_CAM, None, v, t, opacity=0)
        assert info["painted"].any() and (out == src).all()
        out, info = rr.render(src, inst, K_CAM, None, v, t, mask=np.zeros((H, W), np.uint8))
        assert info["painted"].any() and (out == src).all()
        half = np.zeros((H, W), np.uint8)
        half[:, : W // 2] = 1
        out, info = rr.render(src, inst, K_CAM, None, v, t, mask=half)
        assert (out[:, W // 2:] == src[:, W // 2:]).all() and (out[:, : W // 2] != src[:, : W // 2]).any()


@pytest.mark.parametrize("cn", [1, 3])
def test_a_fronto_parallel_quad_has_the_footprint_of_plane_compositing(cn):
    """A constant texture of TW x TH texels, one texel per pixel, its texel centres half a pixel off the pixel centres: compositing paints
    the box of texel centres (the outermost half texel is not shown), and the quad over that box covers the same pixel centres."""
    TW, TH, colour, opacity = 21, 13, (30, 220, 140), 200
    X0, Y0 = (5.5 - 8) / 16, (4.5 - 6) / 16                     # plane point of texel (0, 0): pixel (5.5, 4.5)
    N = np.array([[16, 0, -16 * X0], [0, 16, -16 * Y0], [0, 0, 1]], np.float64)
    src = frame(cn)
    tex = np.empty((TH, TW, cn), np.uint8)
    tex[:] = colour if cn == 3 else rr.gray_of(*colour)
    want, painted = cr.composite(src, tex if cn == 3 else tex[:, :, 0], N, K_EXACT, None, True, opacity)
    v = pixels([(5.5, 4.5), (5.5 + TW - 1, 4.5), (5.5, 4.5 + TH - 1), (5.5 + TW - 1, 4.5 + TH - 1)])
    got, info = rr.render(src, FRONT, K_EXACT, None, v, [(0, 1, 2), (3, 2, 1)], flags=rr.UNLIT, opacity=opacity, color=colour)
    assert painted.sum() == (TW - 1) * (TH - 1) and (info["painted"] == painted).all()
    assert (got == want).all()
