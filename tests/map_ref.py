"""Host model of marker mapping (arucohip_board_map*), written from the problem's statement and independently of the device code:
synthetic scenes with their truth, the rules that say which observations count, the start values (planar solutions from
tests/planar_ref, best edge per marker pair, spanning tree, frame poses) and a scipy.optimize.least_squares solve of the same cost
from those start values. Shared by test_map_cpu.py, test_gpu_map.py and test_gpu_map_shim.py.

Placements are always compared on corner positions (`obj`), never on rotation vectors: the marker on the cube face opposite the
reference sits at an angle near pi, where two equally good solves return rotation vectors of opposite sign."""
import numpy as np

from tests import pose_ref
from tests.planar_ref import brown_project, object_points, planar_poses, rodrigues, rodrigues_inv

SIZE = pose_ref.MARKER_SIZE
W, H = 640, 480
K = np.array([[600.0, 0.0, 320.0], [0.0, 600.0, 240.0], [0.0, 0.0, 1.0]])
DIST5 = np.array([-0.08, 0.03, 8e-4, -5e-4, 0.01])
DIST4 = DIST5[:4]
MAX_MARKERS, MAX_FRAME_MARKERS = 64, 16
FACING = np.radians(65.0)   # a marker is seen when its normal and the ray to the camera enclose less than this
TINY = np.finfo(np.float64).tiny


# ---------------------------------------------------------------------------------------------
# rigid transforms as (R, t)
# ---------------------------------------------------------------------------------------------
def compose(a, b):
    return a[0] @ b[0], a[0] @ b[1] + a[1]


def inverse(a):
    return a[0].T, -a[0].T @ a[1]


def small_transform(rng, rot=0.03, shift=0.002):
    return rodrigues(rng.normal(0.0, rot, 3)), rng.normal(0.0, shift, 3)


def corners_of(T, size=SIZE):
    """The four corners of a marker placed by T: [4][3]."""
    return object_points(size) @ T[0].T + T[1]


def relative_to_first(world):
    """Placements in the frame of marker 0."""
    inv0 = inverse(world[0])
    return [compose(inv0, T) for T in world]


def truth_obj(scene):
    return np.array([corners_of(T) for T in scene["T"]])


# ---------------------------------------------------------------------------------------------
# scenes: dict(ids, T (placements in the frame of marker 0), frames [(R, t) of marker 0's frame in the camera], show [per frame: the
# markers offered to the facing rule, None = all], facing (apply the facing rule), K, dist)
# ---------------------------------------------------------------------------------------------
def _look_at(rng, target, tilt, zr):
    """A camera pose that sees the point `target` of the board near the image centre: the board turned to face the camera and tilted by up
    to `tilt` about a random axis in its plane, the target zr metres away and up to 3 cm off the axis."""
    R = pose_ref.facing_rotation(rng, rng.uniform(0.0, tilt))
    c = np.array([rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03), rng.uniform(*zr)])
    return R, c - R @ target


def _turn_to(d, target):
    """The rotation about d x target that takes the unit vector d onto the unit vector target (not opposite to it)."""
    axis = np.cross(d, target)
    n = np.linalg.norm(axis)
    return np.eye(3) if n < 1e-12 else rodrigues(axis / n * np.arctan2(n, d @ target))


def cube(seed, nframes=24, side=0.08):
    """One marker on each face of a cube, each placement jittered by a seeded small rigid transform. Frame i looks at corner i % 8 of the
    cube, up to 8 degrees off and rolled at random, so that it shows the two or three faces that meet there. Marker 0 is the +z face,
    marker 5 the face opposite to it."""
    rng = np.random.default_rng(seed)
    x, y, z = np.eye(3)
    faces = [(x, y, z), (-z, y, x), (z, y, -x), (x, -z, y), (x, z, -y), (-x, y, -z)]   # (right, up, normal = right x up)
    world = []
    for r, u, n in faces:
        world.append(compose((np.stack([r, u, n], axis=1), side / 2.0 * n), small_transform(rng)))
    T = relative_to_first(world)
    frames = []
    for i in range(nframes):
        d = np.array([1.0 if i & 1 else -1.0, 1.0 if i & 2 else -1.0, 1.0 if i & 4 else -1.0]) / np.sqrt(3.0)
        off = rng.normal(size=3)
        Rw = rodrigues(off / np.linalg.norm(off) * rng.uniform(0.0, np.radians(8.0))) @ pose_ref.rot_z(rng.uniform(0.0, 2 * np.pi)) @ _turn_to(d, -z)
        tw = np.array([rng.uniform(-0.05, 0.05), rng.uniform(-0.04, 0.04), rng.uniform(0.35, 0.5)])
        frames.append(compose((Rw, tw), world[0]))
    return {"ids": np.arange(6, dtype=np.int32) + 20, "T": T, "frames": frames, "show": [None] * nframes, "facing": True, "K": K, "dist": DIST5}


def chain(seed=3, rounds=4):
    """Four panels in a row along x, each tilted 12 degrees further about y: a frame shows two neighbours, so the first and the last are
    never seen together and the tree from marker 0 is three edges deep."""
    rng = np.random.default_rng(seed)
    world = []
    for i in range(4):
        base = (rodrigues(np.array([0.0, np.radians(12.0) * i, 0.0])), np.array([0.07 * i, 0.0, 0.004 * i * i]))
        world.append(compose(base, small_transform(rng)))
    T = relative_to_first(world)
    windows = [(0, 1), (1, 2), (2, 3)]
    frames, show = [], []
    for _ in range(rounds):
        for w in windows:
            target = np.mean([T[m][1] for m in w], axis=0)
            frames.append(_look_at(rng, target, 0.35, (0.4, 0.55)))
            show.append(list(w))
    return {"ids": np.array([7, 3, 11, 5], np.int32), "T": T, "frames": frames, "show": show, "facing": True, "K": K, "dist": None}


def pair(seed=5, nframes=2, turned=False):
    """Two markers 8 cm apart in nearly one plane. turned: the second one turned 180 degrees about its x axis, a marker printed on glass and
    seen from behind (the facing rule is waived: no opaque marker can be seen together with one turned away from it)."""
    rng = np.random.default_rng(seed)
    second = compose((rodrigues(np.array([np.pi if turned else 0.0, 0.0, 0.0])), np.array([0.08, 0.005, 0.0])), small_transform(rng, 0.05))
    T = [(np.eye(3), np.zeros(3)), second]
    frames = [_look_at(rng, np.array([0.04, 0.0, 0.0]), 0.6, (0.35, 0.5)) for _ in range(nframes)]
    return {"ids": np.array([40, 41], np.int32), "T": T, "frames": frames, "show": [None] * nframes, "facing": not turned, "K": K, "dist": DIST4}


def grid(nm, nframes=3, seed=9, windows=False):
    """nm markers on a slightly bent sheet (rows of 8, every row tilted a little more). windows: frame i shows rows i and i + 1 (sixteen
    markers, every marker in some frame, neighbouring frames share a row); else every frame shows all of them."""
    rng = np.random.default_rng(seed)
    world = []
    for i in range(nm):
        r, c = divmod(i, 8)
        world.append(compose((rodrigues(np.array([0.05 * r, 0.0, 0.0])), np.array([0.06 * c, 0.06 * r, 0.002 * r * r])), small_transform(rng, 0.01, 0.0005)))
    T = relative_to_first(world)
    if windows:
        show = [[m for m in range(nm) if m // 8 in (i, i + 1)] for i in range((nm + 7) // 8 - 1)]
    else:
        show = [list(range(nm))] * nframes
    frames = [_look_at(rng, np.mean([T[m][1] for m in s], axis=0), 0.4, (1.1, 1.3)) for s in show]
    return {"ids": np.arange(nm, dtype=np.int32) + 200, "T": T, "frames": frames, "show": show, "facing": True,
            "K": np.array([[1500.0, 0.0, 320.0], [0.0, 1500.0, 240.0], [0.0, 0.0, 1.0]]), "dist": None}


def observe(scene, noise=0.0, seed=0):
    """The scene's observations as the C ABI takes them: (frame int32 [n], id int32 [n], corners float32 [n][8]), frames in order, markers in
    board order. Projection in float64, optional Gaussian noise, rounded to float32."""
    rng = np.random.default_rng(seed)
    fr, ids, cs = [], [], []
    for f, (Rf, tf) in enumerate(scene["frames"]):
        for m, Tm in enumerate(scene["T"]):
            if scene["show"][f] is not None and m not in scene["show"][f]:
                continue
            Rc, tc = compose((Rf, tf), Tm)
            if scene["facing"]:
                ray = -tc / np.linalg.norm(tc)
                if not (tc[2] > 0 and np.arccos(np.clip(Rc[:, 2] @ ray, -1.0, 1.0)) < FACING):
                    continue
            px = brown_project(object_points(SIZE), Rc, tc, scene["K"], scene["dist"])
            if noise > 0:
                px = px + rng.normal(0.0, noise, px.shape)
            fr.append(f), ids.append(int(scene["ids"][m])), cs.append(px.reshape(8))
    return np.array(fr, np.int32), np.array(ids, np.int32), np.array(cs, np.float32).reshape(-1, 8)


# ---------------------------------------------------------------------------------------------
# which observations count
# ---------------------------------------------------------------------------------------------
def perimeter(c):
    q = np.asarray(c, np.float64).reshape(4, 2)
    return float(np.sum(np.linalg.norm(q - np.roll(q, -1, axis=0), axis=1)))


def select(obs, nframes, board_ids, Kc, dist, size=SIZE, min_markers=2):
    """Per frame the list of (board index, corners float64 [4][2], planar dict) that count, in detection order, and used [nframes]."""
    fr, ids, cs = obs
    index = {}
    for k, i in enumerate(board_ids):
        index.setdefault(int(i), k)
    per_frame, used = [], np.zeros(nframes, bool)
    for f in range(nframes):
        cand, seen = [], set()
        for j in np.nonzero(fr == f)[0]:
            b = index.get(int(ids[j]))
            if b is None or b in seen:
                continue
            seen.add(b)
            cand.append((b, np.asarray(cs[j], np.float64).reshape(4, 2)))
        listed = len(cand)
        if listed > MAX_FRAME_MARKERS:
            order = sorted(range(listed), key=lambda k: (-perimeter(cand[k][1]), k))[:MAX_FRAME_MARKERS]
            cand = [cand[k] for k in sorted(order)]
        kept = []
        for b, c in cand:
            pp = planar_poses(c, Kc, dist, size)
            if pp is not None:
                kept.append((b, c, pp))
        per_frame.append(kept)
        used[f] = listed >= max(min_markers, 2) and len(kept) >= 2
    return per_frame, used


# ---------------------------------------------------------------------------------------------
# start values
# ---------------------------------------------------------------------------------------------
def start_values(per_frame, used, nboard):
    """dict(T [nboard] of (R, t) or None, mapped [nboard], frames {f: (R, t)}, used (frames of unconnected markers removed), depth [nboard]
    tree depth); None when marker 0 is in no used frame."""
    used = used.copy()
    q = [{b: pp["rms"][1] / max(pp["rms"][0], TINY) for b, _, pp in kept} for kept in per_frame]
    pose = [{b: (pp["R"][0], pp["tvec"][0]) for b, _, pp in kept} for kept in per_frame]
    if not any(used[f] and 0 in q[f] for f in range(len(per_frame))):
        return None
    edge = {}
    for f in range(len(per_frame)):
        if not used[f]:
            continue
        for a in q[f]:
            for b in q[f]:
                if a != b:
                    s = min(q[f][a], q[f][b])
                    if (a, b) not in edge or s > edge[(a, b)][0]:
                        edge[(a, b)] = (s, f)
    T = [None] * nboard
    T[0] = (np.eye(3), np.zeros(3))
    depth = [-1] * nboard
    depth[0] = 0
    while True:
        best = None
        for b in range(nboard):
            if T[b] is not None:
                continue
            mine = None
            for a in range(nboard):
                if T[a] is not None and (a, b) in edge and (mine is None or edge[(a, b)][0] > mine[0]):
                    mine = (edge[(a, b)][0], a)
            if mine is not None and (best is None or mine[0] > best[0]):
                best = (mine[0], mine[1], b)
        if best is None:
            break
        _, a, b = best
        f = edge[(a, b)][1]
        T[b] = compose(T[a], compose(inverse(pose[f][a]), pose[f][b]))
        depth[b] = depth[a] + 1
    mapped = np.array([t is not None for t in T])
    frames = {}
    for f in range(len(per_frame)):
        if not used[f]:
            continue
        best = None
        for b, _, _ in per_frame[f]:
            if mapped[b] and (best is None or q[f][b] > q[f][best]):
                best = b
        if best is None:
            used[f] = False
        else:
            frames[f] = compose(pose[f][best], inverse(T[best]))
    return {"T": T, "mapped": mapped, "frames": frames, "used": used, "depth": depth}


# ---------------------------------------------------------------------------------------------
# the cost and its scipy solve
# ---------------------------------------------------------------------------------------------
def _rodrigues_many(r):
    th = np.linalg.norm(r, axis=1)
    safe = np.maximum(th, 1e-300)
    k = r / safe[:, None]
    Kx = np.zeros((len(r), 3, 3))
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0] = -k[:, 2], k[:, 1], k[:, 2]
    Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -k[:, 0], -k[:, 1], k[:, 0]
    return np.eye(3) + np.sin(th)[:, None, None] * Kx + (1 - np.cos(th))[:, None, None] * (Kx @ Kx)


class Problem:
    """The observations of the used frames and mapped markers; x = [rvec, tvec of the mapped markers but 0 | rvec, tvec of the used frames]."""

    def __init__(self, per_frame, used, mapped, Kc, dist, size=SIZE):
        self.K = np.asarray(Kc, np.float64).reshape(3, 3)
        self.d = np.zeros(5)
        if dist is not None:
            self.d[:len(dist)] = np.asarray(dist, np.float64)
        self.P = object_points(size)
        self.markers = [m for m in range(len(mapped)) if mapped[m] and m > 0]
        self.frames = [f for f in range(len(per_frame)) if used[f]]
        mi = {m: k for k, m in enumerate(self.markers)}
        om, of, px, self.board = [], [], [], []
        for k, f in enumerate(self.frames):
            for b, c, _ in per_frame[f]:
                om.append(mi.get(b, -1)), of.append(k), px.append(np.asarray(np.float32(c), np.float64)), self.board.append(b)
        self.om, self.of, self.px = np.array(om), np.array(of), np.array(px)
        self.board = np.array(self.board)

    def pack(self, T, frames):
        x = []
        for m in self.markers:
            x += [rodrigues_inv(T[m][0]), T[m][1]]
        for f in self.frames:
            x += [rodrigues_inv(frames[f][0]), frames[f][1]]
        return np.concatenate(x) if x else np.zeros(0)

    def unpack(self, x):
        nm = len(self.markers)
        pm = np.concatenate([np.zeros((1, 6)), x[:6 * nm].reshape(nm, 6)])   # row 0: marker 0, the identity
        return pm, x[6 * nm:].reshape(len(self.frames), 6)

    def residuals(self, x):
        pm, pf = self.unpack(x)
        Rm, Rf = _rodrigues_many(pm[:, :3]), _rodrigues_many(pf[:, :3])
        om = self.om + 1
        X = np.einsum("nij,kj->nki", Rm[om], self.P) + pm[om, None, 3:]
        Xc = np.einsum("nij,nkj->nki", Rf[self.of], X) + pf[self.of, None, 3:]
        xn, yn = Xc[..., 0] / Xc[..., 2], Xc[..., 1] / Xc[..., 2]
        r2 = xn * xn + yn * yn
        d = self.d
        rad = 1 + d[0] * r2 + d[1] * r2 ** 2 + d[4] * r2 ** 3
        xd = xn * rad + 2 * d[2] * xn * yn + d[3] * (r2 + 2 * xn * xn)
        yd = yn * rad + d[2] * (r2 + 2 * yn * yn) + 2 * d[3] * xn * yn
        u, v = self.K[0, 0] * xd + self.K[0, 2], self.K[1, 1] * yd + self.K[1, 2]
        return np.stack([u - self.px[..., 0], v - self.px[..., 1]], axis=-1)

    def solve(self, x0):
        from scipy.optimize import least_squares

        res = least_squares(lambda x: self.residuals(x).ravel(), x0, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=400 * (len(x0) + 1))
        return res.x

    def result(self, x, nboard, nframes, size=SIZE):
        pm, pf = self.unpack(x)
        obj = np.zeros((nboard, 4, 3))
        mapped = np.zeros(nboard, bool)
        for k, m in enumerate([0] + self.markers):
            obj[m] = corners_of((rodrigues(pm[k, :3]), pm[k, 3:]), size)
            mapped[m] = True
        r = self.residuals(x)
        e2 = np.sum(r * r, axis=(1, 2))
        marker_rms = np.zeros(nboard)
        for m in range(nboard):
            if mapped[m] and np.any(self.board == m):
                marker_rms[m] = np.sqrt(np.sum(e2[self.board == m]) / (4 * np.sum(self.board == m)))
        fr, ft = np.zeros((nframes, 3)), np.zeros((nframes, 3))
        for k, f in enumerate(self.frames):
            fr[f], ft[f] = pf[k, :3], pf[k, 3:]
        return {"obj": obj, "mapped": mapped, "rms": float(np.sqrt(np.sum(e2) / (4 * len(e2)))), "marker_rms": marker_rms, "frame_rvecs": fr,
                "frame_tvecs": ft, "x": x}


def reference(obs, nframes, board_ids, Kc, dist, size=SIZE, min_markers=2, truth=None):
    """The whole reference: selection, start values, scipy solve. dict(obj, mapped, used, rms, marker_rms, frame_rvecs, frame_tvecs, depth,
    start_obj); with truth = (T, frames) of a scene also truth_obj_solved: the solve started at the truth. None where the call must fail."""
    nboard = len(board_ids)
    per_frame, used = select(obs, nframes, board_ids, Kc, dist, size, min_markers)
    sv = start_values(per_frame, used, nboard)
    if sv is None or sv["mapped"].sum() < 2:
        return None
    prob = Problem(per_frame, sv["used"], sv["mapped"], Kc, dist, size)
    x0 = prob.pack(sv["T"], sv["frames"])
    out = prob.result(prob.solve(x0), nboard, nframes, size)
    out["used"], out["depth"] = sv["used"], sv["depth"]
    out["start_obj"] = prob.result(x0, nboard, nframes, size)["obj"]
    out["problem"] = prob
    if truth is not None:
        xt = prob.pack(truth[0], {f: truth[1][f] for f in prob.frames})
        out["truth_solved"] = prob.result(prob.solve(xt), nboard, nframes, size)
    return out


def island(c):
    """The chain's observations with panel 2 taken out of the frames it shares with panel 1: panels 2 and 3 still see each other, in frames
    that show two listed markers, but nothing connects them to panel 0. Returns (obs, the frames that show the island)."""
    fr, ids, cs = c["obs"]
    board = c["scene"]["ids"]
    shared = [f for f, s in enumerate(c["scene"]["show"]) if 1 in s and 2 in s]
    keep = ~((ids == board[2]) & np.isin(fr, shared))
    return (fr[keep], ids[keep], cs[keep]), np.array([f for f, s in enumerate(c["scene"]["show"]) if 3 in s])


_cache = {}


def case(name, noise=0.0, seed=0):
    """A scene with its observations and reference, computed once per process: dict(scene, obs, nframes, ref)."""
    key = (name, noise, seed)
    if key not in _cache:
        scene = {"cube": lambda: cube(100 + seed), "chain": chain, "pair": pair, "pair180": lambda: pair(turned=True)}[name]()
        obs = observe(scene, noise, 1000 + seed)
        n = len(scene["frames"])
        ref = reference(obs, n, scene["ids"], scene["K"], scene["dist"], truth=(scene["T"], scene["frames"]))
        _cache[key] = {"scene": scene, "obs": obs, "nframes": n, "ref": ref}
    return _cache[key]


# the cases of the GPU tests: (scene, noise, seed)
EXACT_CASES = [("cube", 0.0, 0), ("chain", 0.0, 0), ("pair", 0.0, 0), ("pair180", 0.0, 0)]
NOISY_CASES = [("cube", pose_ref.NOISE, s) for s in (1, 2, 3)]


def obj_dev(a, b, mask=None):
    """Largest corner distance in metres between two sets of object points (over the markers of mask)."""
    a, b = np.asarray(a, np.float64).reshape(-1, 4, 3), np.asarray(b, np.float64).reshape(-1, 4, 3)
    d = np.linalg.norm(a - b, axis=2)
    return float(np.max(d if mask is None else d[np.asarray(mask, bool)]))
