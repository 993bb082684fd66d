"""Mesh rendering on the device against tests/render_ref.py: byte for byte, no tolerance, on every pixel that is not fragile_depth.

Scenes come from a seeded generator (SCENES). A scene with a fragile vertex coordinate or a fragile shade is replaced by the next seed
(+1000), counted, and at most one scene in ten may be replaced; fragile_depth pixels are left out and may be at most 0.1 % of a case's
painted pixels. Both shares are printed. The references are computed once (built()) and shared.

The 2000-triangle sphere has 2004 projected coordinates, so a seed whose scene has none within 1e-3 of a half-integer is rare (about
one in 55, against about nine in ten for a cube scene): its first seed was searched ahead and is written down in SCENES, so that the draw
made here is firm like the others; the cap on replacements holds for it as for the rest.
Small shapes: frames of at most 130 x 33, one to three frames a case."""
import functools

import numpy as np
import pytest

from tests import render_ref as rr

pytestmark = pytest.mark.gpu

SENT = 0xA5
SIZES = [(1, 1), (70, 20), (130, 33), (64, 16)]
DIST5 = np.array([0.08, -0.05, 0.002, -0.001, 0.01], np.float32)
FACE_COLORS = np.repeat(np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [255, 0, 255], [0, 255, 255]], np.uint8), 2, axis=0)
K_EXACT = np.array([[16, 0, 40], [0, 16, 12], [0, 0, 1]], np.float32)


@pytest.fixture(scope="module")
def handle():
    from aruco_amd import capi

    h = capi.Handle(640, 480, max_batch=4)
    yield h
    h.close()


def camera(W, H):
    f = 1.1 * max(W, H, 16)
    return np.array([[f, 0, (W - 1) / 2 + 0.3], [0, f * 1.02, (H - 1) / 2 - 0.2], [0, 0, 1]], np.float32)


def marker_dtype():
    from aruco_amd import capi

    return capi.MARKER_DTYPE


def random_markers(rng, W, H, K, n, cap, size=None):
    """n posed markers of a W x H frame in a list of `cap`: facing the camera within half a radian, centres inside the frame"""
    m = np.zeros(cap, marker_dtype())
    px = max(min(W, H) * 0.45, 6.0) if size is None else size
    for i in range(n):
        z = rng.uniform(2.0, 4.0)
        u, v = rng.uniform(0.15, 0.85) * (W - 1), rng.uniform(0.15, 0.85) * (H - 1)
        m[i]["id"], m[i]["has_pose"], m[i]["ssize"] = i, 1, px * z / K[0, 0]
        m[i]["rvec"] = np.array([np.pi, 0, 0]) + rng.uniform(-0.5, 0.5, 3)
        m[i]["tvec"] = [(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z]
    return m


def exact_marker(cap=1):
    m = np.zeros(cap, marker_dtype())
    m[0]["has_pose"], m[0]["ssize"], m[0]["tvec"] = 1, 1.0, [0, 0, 1]
    return m


def pixels(pts):
    """object-frame vertices (z = 0) of pixel positions under K_EXACT and exact_marker()"""
    p = np.asarray(pts, np.float64)
    return np.stack([(p[:, 0] - 40) / 16, (p[:, 1] - 12) / 16, np.zeros(len(p))], axis=1).astype(np.float32)


def cube():
    from aruco_amd import capi

    v, t = capi.cube_mesh()
    return v, t, FACE_COLORS


def sphere2000():
    from aruco_amd import capi

    v, t = capi.uv_sphere_mesh(26, 40, center=(0.0, 0.0, 0.0))
    assert len(t) == 2000
    return v, t, np.random.RandomState(2).randint(0, 256, (2000, 3)).astype(np.uint8)


def checkerboard(n, H, W):
    y, x = np.mgrid[0:H, 0:W]
    return np.broadcast_to((((x // 3) + (y // 2)) & 1).astype(np.uint8), (n, H, W)).copy()


def source(n, W, H, cn, seed=7):
    return np.random.RandomState(seed + cn).randint(0, 256, (n, H, W) if cn == 1 else (n, H, W, 3)).astype(np.uint8)


# name -> how a seed makes the scene: dict(size, cn, markers [N][cap], counts, mesh (v, t, colours or None), style, K, dist, masks)
def _geometry(W, H, cn):
    def make(rng):
        K = camera(W, H)
        ms = np.stack([random_markers(rng, W, H, K, 2, 2), random_markers(rng, W, H, K, 1, 2)])
        return dict(size=(W, H), cn=cn, markers=ms, counts=[2, 1], mesh=cube(), K=K, dist=DIST5 if (W, H) == (70, 20) else None,
                    masks=checkerboard(2, H, W) if (W, H) == (130, 33) else None, style=dict(flags=1, opacity=255 if cn == 3 else 128))
    return make


def _counts(rng):
    K = camera(130, 33)
    ms = np.stack([random_markers(rng, 130, 33, K, 3, 3) for _ in range(3)])
    return dict(size=(130, 33), cn=3, markers=ms, counts=[2, 0, -1], mesh=cube(), K=K, style=dict(flags=1))


def _nopose(rng):
    K = camera(130, 33)
    ms = random_markers(rng, 130, 33, K, 3, 3)[None]
    ms[0, 1]["has_pose"] = 0
    return dict(size=(130, 33), cn=3, markers=ms, counts=[3], mesh=cube(), K=K, style=dict(flags=1, ambient=20))


def _one_marker(mesh, size=None, **style):
    def make(rng):
        K = camera(130, 33)
        return dict(size=(130, 33), cn=3, markers=random_markers(rng, 130, 33, K, 1, 1, size)[None], counts=[1], mesh=mesh(), K=K, style=style)
    return make


def _two_cubes(rng):
    """two cubes that overlap on screen at different depths: the second stands half a side beside the first and 1.5 sides behind it"""
    K = camera(130, 33)
    ms = random_markers(rng, 130, 33, K, 1, 2)[None]
    ms[0, 1] = ms[0, 0]
    ms[0, 1]["tvec"] += [0.5 * ms[0, 0]["ssize"], 0.1 * ms[0, 0]["ssize"], 1.5 * ms[0, 0]["ssize"]]
    ms[0, 1]["rvec"] += [0.2, -0.3, 0.1]
    return dict(size=(130, 33), cn=3, markers=ms[:, ::-1].copy(), counts=[2], mesh=cube(), K=K, style=dict(flags=0, opacity=128))


def _sphere(rng):
    """a sphere of 13 pixels inside the tile [64, 128) x [16, 32): without culling most of its 2000 triangles reach that tile's bin"""
    K = camera(130, 33)
    m = np.zeros(1, marker_dtype())
    z = rng.uniform(2.0, 4.0)
    m[0]["has_pose"], m[0]["ssize"] = 1, 13.0 * z / K[0, 0]
    m[0]["rvec"] = np.array([np.pi, 0, 0]) + rng.uniform(-0.5, 0.5, 3)
    m[0]["tvec"] = [(96 - K[0, 2]) / K[0, 0] * z, (24 - K[1, 2]) / K[1, 1] * z, z]
    return dict(size=(130, 33), cn=3, markers=m[None], counts=[1], mesh=sphere2000(), K=K, style=dict(flags=0))


def _exact(mesh, **style):
    def make(rng):
        return dict(size=(130, 33), cn=3, markers=exact_marker()[None], counts=[1], mesh=mesh, K=K_EXACT, style=dict(flags=2, **style))
    return make


QUAD = (pixels([(10, 8), (14, 8), (10, 12), (14, 12)]), np.array([(0, 1, 2), (3, 2, 1)], np.int32), None)
# one triangle with a vertex behind the camera (object z = -3 at tvec z = 1), one of no area, one good one
v_odd = np.concatenate([pixels([(20, 4), (60, 6), (30, 28), (70, 20), (90, 25), (100, 5)]), np.array([[0, 0, -3]], np.float32)])
ODD = (v_odd, np.array([(0, 1, 6), (3, 4, 4), (3, 5, 4), (0, 2, 1)], np.int32), np.array([[9, 9, 9], [50, 50, 50], [0, 0, 255], [255, 0, 0]], np.uint8))

SPHERE_SEED = 34   # searched ahead: the first seed from 0 whose sphere has no fragile coordinate (see the module's docstring)
SCENES = {"geometry-%dx%d-%d" % (w, h, cn): (_geometry(w, h, cn), 11 + 3 * i + cn) for i, (w, h) in enumerate(SIZES) for cn in (1, 3)}
SCENES.update({
    "counts": (_counts, 31), "nopose": (_nopose, 32),
    "triangle": (_one_marker(lambda: (np.array([[-0.5, -0.4, 0], [0.6, -0.2, 0.3], [0.1, 0.7, 0.1]], np.float32), np.array([[0, 1, 2]], np.int32), None),
                             flags=0, color=(200, 100, 50)), 33),
    "cube-culled": (_one_marker(cube, flags=1), 34), "cube-unculled": (_one_marker(cube, flags=0), 34),
    "two-cubes": (_two_cubes, 35),
    "partly-outside": (_one_marker(cube, size=60.0, flags=1), 36),
    "sphere-2000": (_sphere, SPHERE_SEED),
    "single-colour": (_one_marker(lambda: cube()[:2] + (None,), flags=1, color=(40, 90, 250)), 37),
    "unlit": (_one_marker(cube, flags=3), 37),
    "light-off-axis": (_one_marker(cube, flags=1, light=(0.5, -0.7, -0.6), ambient=30), 37),
    "exact-quad": (_exact(QUAD, opacity=128, color=(10, 250, 90)), 0),
    "exact-odd": (_exact(ODD), 0),
})


def reference(sc):
    """(the painted frames, the infos) of a scene"""
    W, H = sc["size"]
    src = source(len(sc["counts"]), W, H, sc["cn"])
    st = dict(sc["style"])
    scale = st.pop("scale", 1.0)
    v, t, c = sc["mesh"]
    res = [rr.render(src[f], rr.marker_instances(sc["markers"][f], sc["counts"][f], scale), sc["K"], sc.get("dist"), v, t, c,
                     mask=None if sc.get("masks") is None else sc["masks"][f], **st) for f in range(len(src))]
    return np.stack([r[0] for r in res]), [r[1] for r in res]


@functools.lru_cache(maxsize=None)
def built():
    """every scene with its reference, and the tally of the draws: name -> (scene, want, infos); (drawn, replaced)"""
    out, drawn, replaced = {}, 0, 0
    for name, (make, seed) in SCENES.items():
        while True:
            sc = make(np.random.RandomState(seed))
            want, infos = reference(sc)
            drawn += 1
            if not any(i["fragile_vertex"] or i["fragile_shade"] for i in infos):
                break
            replaced, seed = replaced + 1, seed + 1000
        out[name] = (sc, want, infos)
    print("scenes drawn %d, replaced for a fragile vertex or shade %d (%.1f %%)" % (drawn, replaced, 100.0 * replaced / drawn))
    assert replaced * 10 <= drawn, (replaced, drawn)
    return out


class Frames:
    """The frames of a call, tight or with rows of w * cn + 5 bytes and frames 7 bytes further apart, SENT in every byte that is no pixel."""

    def __init__(self, images, device, padded):
        self.n, self.h, self.w = images.shape[:3]
        self.cn = 1 if images.ndim == 3 else 3
        self.device = device
        self.row = self.w * self.cn + (5 if padded else 0)
        self.frame = self.row * self.h + (7 if padded else 0)
        buf = np.full(self.n * self.frame + 8, SENT, np.uint8)
        for f in range(self.n):
            for y in range(self.h):
                at = f * self.frame + y * self.row
                buf[at:at + self.w * self.cn] = images[f, y].reshape(-1)
        if device:
            import torch

            self.buf = torch.from_numpy(buf).cuda()
            self.ptr = self.buf.data_ptr()
        else:
            self.buf = buf
            self.ptr = buf.ctypes.data

    def split(self):
        """(the images, whether every other byte still holds the sentinel)"""
        b = self.buf.cpu().numpy().copy() if self.device else self.buf.copy()
        out = np.zeros((self.n, self.h, self.w * self.cn), np.uint8)
        for f in range(self.n):
            for y in range(self.h):
                at = f * self.frame + y * self.row
                out[f, y] = b[at:at + self.w * self.cn]
                b[at:at + self.w * self.cn] = SENT
        return (out if self.cn == 1 else out.reshape(self.n, self.h, self.w, 3)), bool((b == SENT).all())


def place(a, device):
    """(the array where the call reads it, its address)"""
    if a is None:
        return None, None
    a = np.ascontiguousarray(a)
    if device:
        import torch

        t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()
        return t, t.data_ptr()
    return a, a.ctypes.data


def run(handle, sc, frames_dev=False, markers_dev=False, mesh_dev=False, masks_dev=False, padded=False, flags_or=0, mesh=None):
    """arucohip_render_markers_batch on a scene; each argument on the host or on the device"""
    from aruco_amd import capi

    W, H = sc["size"]
    n = len(sc["counts"])
    fr = Frames(source(n, W, H, sc["cn"]), frames_dev, padded)
    keep_m, mptr = place(sc["markers"], markers_dev)
    keep_c, cptr = place(np.asarray(sc["counts"], np.int32), markers_dev)
    v, t, c = sc["mesh"] if mesh is None else mesh
    if mesh_dev:
        import torch

        dv, dt = torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(t, np.int32)).cuda()
        msh = capi.mesh(dv, dt, None if c is None else torch.from_numpy(np.ascontiguousarray(c, np.uint8)).cuda())
    else:
        msh = capi.mesh(v, t, c)
    keep_k, kptr = place(sc.get("masks"), masks_dev)
    st = dict(sc["style"])
    st["flags"] = st.get("flags", 1) | flags_or
    handle.render_markers_device(fr.ptr, n, W, H, sc["cn"], mptr, sc["markers"].shape[1], cptr, sc["K"], msh, capi.render_style(**st), sc.get("dist"),
                                 kptr, fr.row, fr.frame, int(frames_dev), int(markers_dev), int(masks_dev))
    handle.synchronize()
    del keep_m, keep_c, keep_k
    return fr.split()


def check(name, got, clean, want, infos, src):
    painted = sum(int(i["painted"].sum()) for i in infos)
    fragile = np.stack([i["fragile_depth"] for i in infos])
    share = fragile.sum() / max(painted, 1)
    print("%s: painted %d, fragile_depth %d (%.4f %%)" % (name, painted, fragile.sum(), 100 * share))
    assert clean, "a byte outside the images was written"
    assert share <= 1e-3
    assert (got[~fragile] == want[~fragile]).all(), np.argwhere((got != want).reshape(fragile.shape + (-1,)).any(axis=-1) & ~fragile)[:5]
    if painted and name not in ("geometry-1x1-1", "geometry-1x1-3"):
        assert (want != src).any()


@pytest.mark.parametrize("name", list(SCENES))
def test_scene_on_the_device_and_on_the_host(handle, name):
    """every scene twice: everything on the device with padded strides, and everything on the host with tight ones"""
    sc, want, infos = built()[name]
    src = source(len(sc["counts"]), sc["size"][0], sc["size"][1], sc["cn"])
    got, clean = run(handle, sc, True, True, True, True, padded=True)
    check(name + " device", got, clean, want, infos, src)
    got, clean = run(handle, sc)
    check(name + " host", got, clean, want, infos, src)


def test_the_scenes_cover_what_they_are_for():
    b = built()
    assert b["counts"][2][0]["painted"].any() and not b["counts"][2][1]["painted"].any() and not b["counts"][2][2]["painted"].any()
    assert len({int(o) for o in b["counts"][2][0]["owner"][..., 0].ravel()} - {-1}) == 2          # the third marker lies beyond counts[0] = 2
    assert {int(o) for o in b["nopose"][2][0]["owner"][..., 0].ravel()} - {-1} == {0, 1}            # two instances: the middle marker has no pose
    assert (b["cube-culled"][2][0]["painted"] == b["cube-unculled"][2][0]["painted"]).all()
    owners = b["two-cubes"][2][0]["owner"][..., 0]
    assert (owners == 0).sum() > 20 and (owners == 1).sum() > 20                                   # both cubes show; the far one comes first in the list
    p = b["partly-outside"][2][0]["painted"]
    assert p[0].any() or p[-1].any() or p[:, 0].any() or p[:, -1].any()
    sp = b["sphere-2000"][2][0]["painted"]
    ys, xs = np.nonzero(sp)
    assert sp.sum() > 80 and xs.min() >= 64 and xs.max() < 128 and ys.min() >= 16 and ys.max() < 32
    odd = {int(o) for o in b["exact-odd"][2][0]["owner"][..., 1].ravel()} - {-1}
    assert odd == {2, 3}                                                                           # behind the camera and zero area: absent
    def base_colours_only(name):
        sc, want, infos = b[name]
        px = want[0][infos[0]["painted"]].astype(np.int64)
        return bool((px[:, None, :] == FACE_COLORS[None].astype(np.int64)).all(axis=2).any(axis=1).all())

    assert base_colours_only("unlit") and not base_colours_only("cube-culled") and not base_colours_only("light-off-axis")
    y, x = np.mgrid[0:33, 0:130]
    assert (b["exact-quad"][2][0]["painted"] == ((x >= 10) & (x < 14) & (y >= 8) & (y < 12))).all()
    assert all(not i["fragile_depth"].any() and i["fragile_vertex"] == 0 for n in ("exact-quad", "exact-odd") for i in b[n][2])


def test_every_mix_of_host_and_device_arguments(handle):
    sc, want, infos = built()["geometry-130x33-3"]
    src = source(2, 130, 33, 3)
    for mix in range(1, 15):
        got, clean = run(handle, sc, bool(mix & 1), bool(mix & 2), bool(mix & 4), bool(mix & 8), padded=bool(mix & 1))
        check("mix %d" % mix, got, clean, want, infos, src)


def chunked_scene():
    """the three frames of "counts" in lists of 65535 slots, the largest cap: the records of one frame exceed the 64 MiB of a chunk, so
    every frame is a chunk of its own with its own part of the markers, counts, frames and masks"""
    sc = dict(built()["counts"][0])
    ms = np.zeros((3, 65535), marker_dtype())
    ms[:, :3] = sc["markers"]
    sc.update(markers=ms, counts=[2, 1, 2], masks=checkerboard(3, 33, 130))
    return sc


def test_frames_are_chunked_on_the_stream(handle):
    sc = chunked_scene()
    want, infos = reference(sc)
    assert not any(i["fragile_vertex"] or i["fragile_shade"] for i in infos) and all(i["painted"].any() for i in infos)
    src = source(3, 130, 33, 3)
    got, clean = run(handle, sc, True, True, True, True, padded=True)
    check("chunked device", got, clean, want, infos, src)
    got, clean = run(handle, sc)
    check("chunked host", got, clean, want, infos, src)


def test_int64_edge_functions_give_the_same_bytes(handle):
    for name in ("geometry-70x20-1", "two-cubes", "sphere-2000", "exact-quad"):
        sc, want, infos = built()[name]
        src = source(len(sc["counts"]), sc["size"][0], sc["size"][1], sc["cn"])
        got, clean = run(handle, sc, True, True, True, True, flags_or=4)
        check(name + " int64", got, clean, want, infos, src)


def test_boards_take_the_same_path(handle):
    """one instance per frame at the board's pose, scale in the pose's units; a frame without a pose stays as it was"""
    from aruco_amd import capi

    sc, _, _ = built()["counts"]
    K, (v, t, c) = sc["K"], sc["mesh"]
    boards = np.zeros(3, capi.BOARD_DTYPE)
    for f in range(3):
        boards[f] = (4, int(f != 1), sc["markers"][f, 0]["rvec"], sc["markers"][f, 0]["tvec"])
    scale = float(sc["markers"][0, 0]["ssize"])
    src = source(3, 130, 33, 3)
    res = [rr.render(src[f], rr.board_instances(boards[f], scale), K, None, v, t, c, flags=1) for f in range(3)]
    want, infos = np.stack([r[0] for r in res]), [r[1] for r in res]
    assert not any(i["fragile_vertex"] or i["fragile_shade"] for i in infos) and not infos[1]["painted"].any()
    host = src.copy()
    handle.render_boards(host, boards, K, capi.mesh(v, t, c), capi.render_style(scale=scale))
    check("boards host", host, True, want, infos, src)
    import torch

    dev, dboards = torch.from_numpy(src.copy()).cuda(), torch.from_numpy(boards.view(np.uint8).copy()).cuda()
    dmesh = capi.mesh(torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(c).cuda())
    handle.render_boards(dev, dboards, K, dmesh, capi.render_style(scale=scale))
    handle.synchronize()
    check("boards device", dev.cpu().numpy(), True, want, infos, src)


def test_a_device_mesh_with_an_index_past_the_vertices(handle):
    """that triangle is absent, everything else is there, and no error is reported"""
    sc, want, infos = built()["cube-unculled"]
    v, t, c = sc["mesh"]
    bad = np.concatenate([t[:5], np.array([[0, 1, len(v)]], np.int32), t[5:], np.array([[-1, 2, 3], [2 ** 30, 0, 1]], np.int32)])
    colours = np.concatenate([c[:5], [[1, 2, 3]], c[5:], [[4, 5, 6], [7, 8, 9]]]).astype(np.uint8)
    got, clean = run(handle, sc, True, True, True, True, mesh=(v, bad, colours))
    check("bad index", got, clean, want, infos, source(1, 130, 33, 3))


def test_refusals_name_what_is_wrong(handle):
    from aruco_amd import capi

    sc, _, _ = built()["cube-culled"]
    K, (v, t, c) = sc["K"], sc["mesh"]
    ms, one = sc["markers"], np.ones(1, np.int32)
    good = dict(frames=None, n=1, w=130, h=33, cn=3, mk=ms, cap=1, cnt=one, K=K, msh=capi.mesh(v, t, c), style={}, dist=None, masks=None, rs=None, fs=None)

    def err(code, word, **kw):
        a = dict(good)
        a.update(kw)
        frames = np.zeros((4, 33, 130 * 3 + 8), np.uint8) if a["frames"] is None or isinstance(a["frames"], int) else a["frames"]
        st = a["style"] if isinstance(a["style"], capi.Render) or a["style"] is None else capi.render_style(**a["style"])
        with pytest.raises(capi.ArucoHipError) as e:
            handle.render_markers_device(0 if isinstance(a["frames"], int) else frames.ctypes.data, a["n"], a["w"], a["h"], a["cn"],
                                         None if a["mk"] is None else a["mk"].ctypes.data, a["cap"], None if a["cnt"] is None else a["cnt"].ctypes.data,
                                         a["K"], a["msh"], st, a["dist"], a["masks"], a["rs"], a["fs"], 0, 0, 0)
        assert e.value.code == code and word in str(e.value), str(e.value)
        return frames

    I, U = capi.E_INVALID, capi.E_UNSUPPORTED
    err(I, "frames is NULL", frames=0)
    err(I, "markers / counts", mk=None)
    err(I, "markers / counts", cnt=None)
    err(I, "mesh is NULL", msh=None)
    err(I, "mesh->vertices", msh=capi.Mesh(None, t.ctypes.data, None, 8, 12, 0, 0))
    err(I, "mesh->vertices", msh=capi.Mesh(v.ctypes.data, None, None, 8, 12, 0, 0))
    err(I, "K is NULL", K=None)
    err(I, "channels", cn=2)
    err(I, "opacity", style=dict(opacity=256))
    err(I, "opacity", style=dict(opacity=-1))
    err(I, "ambient", style=dict(ambient=300))
    for s in (0.0, -1.0, float("inf"), float("nan")):
        err(I, "scale", style=dict(scale=s))
    err(I, "light", style=dict(light=(0, 0, 0)))
    err(I, "light", style=dict(light=(0, float("nan"), 1)))
    err(I, "nframes", n=0)
    err(I, "width / height", w=0)
    err(I, "width / height", h=0)
    err(I, "cap is below 1", cap=0)
    err(I, "nverts", msh=capi.Mesh(v.ctypes.data, t.ctypes.data, None, 0, 12, 0, 0))
    err(I, "nverts", msh=capi.Mesh(v.ctypes.data, t.ctypes.data, None, 65537, 12, 0, 0))
    err(I, "ntris", msh=capi.Mesh(v.ctypes.data, t.ctypes.data, None, 8, 0, 0, 0))
    err(I, "ntris", msh=capi.Mesh(v.ctypes.data, t.ctypes.data, None, 8, 16385, 0, 0))
    err(I, "ndist", dist=np.zeros(3, np.float32))
    err(I, "row_stride", rs=130 * 3 - 1)
    err(I, "frame_stride", n=2, fs=130 * 3 * 33 - 1)
    big = np.zeros(4 * 33 * (130 * 3 + 8) + 4096, np.uint8)
    inside = big[:4 * 33 * 398].reshape(4, 33, 398)
    for what, m in (("mesh->vertices", capi.Mesh(big.ctypes.data + 64, t.ctypes.data, None, 8, 12, 0, 0)),
                    ("mesh->triangles", capi.Mesh(v.ctypes.data, big.ctypes.data + 64, None, 8, 12, 0, 0)),
                    ("mesh->colors", capi.Mesh(v.ctypes.data, t.ctypes.data, big.ctypes.data + 64, 8, 12, 0, 0))):
        err(I, what + " overlaps", frames=inside, msh=m)
    err(I, "masks overlaps", frames=inside, masks=big.ctypes.data + 128)
    past = t.copy()
    past[7, 1] = 8
    err(I, "index outside", msh=capi.mesh(v, past, c))
    past[7, 1] = -1
    err(I, "index outside", msh=capi.mesh(v, past, c))
    err(U, "exceed the handle", w=641, rs=641 * 3, frames=np.zeros((1, 33, 641 * 3), np.uint8))
    err(U, "exceed the handle", h=481, frames=np.zeros((1, 481, 130 * 3), np.uint8), rs=130 * 3)
    err(U, "cap exceeds 65535", cap=65536)
    untouched = err(I, "channels", cn=4)
    assert not untouched.any()
    with pytest.raises(capi.ArucoHipError) as e:
        handle.render_boards_device(np.zeros((1, 33, 390), np.uint8).ctypes.data, 1, 130, 33, 3, np.zeros(1, capi.BOARD_DTYPE), None,
                                    capi.mesh(v, t, c), frames_on_device=0)
    assert e.value.code == I and "K is NULL" in str(e.value)


def test_rendering_leaves_detection_and_the_single_frame_graph_valid():
    """detect three times (the third call replays the captured graph), render into a 1080p host frame, detect again: the same bytes."""
    from aruco_amd import capi
    from aruco_amd.fixtures import load_case

    gray, doc = load_case("single")
    intr = doc["intrinsics"]
    h = capi.Handle(1920, 1080, max_batch=1, device=0)
    for _ in range(3):
        third = h.detect(gray, K=intr["K"], dist=intr["dist"], marker_size=1.0)
    assert len(third) == len(doc["markers"]) and third["has_pose"].any()
    frame = np.zeros((1, 1080, 1920, 3), np.uint8)
    v, t = capi.cube_mesh()
    h.render_markers(frame, third.reshape(1, -1), np.array([len(third)], np.int32), intr["K"], capi.mesh(v, t), dist=intr["dist"])
    assert frame.any()
    again = h.detect(gray, K=intr["K"], dist=intr["dist"], marker_size=1.0)
    assert again.tobytes() == third.tobytes()
    h.close()
