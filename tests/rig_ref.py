"""Float64 host model of the camera rig calls (arucohip_rig_calibrate*, arucohip_rig_pose*), written from the rules of include/arucohip.h and
not from the device code: which observations count, the start values (pair scores, the spanning tree from camera 0, the instants' poses)
and a scipy.optimize.least_squares solve of the same cost from those start values. Shared by test_rig_cpu.py, test_gpu_rig.py.

A rig is ncams cameras; camera c has fixed intrinsics and the transform rig -> camera T_c = (R_c, t_c), X_c = R_c X_rig + t_c; camera 0 is the
rig frame. View v = instant * ncams + camera. The cost: over every counted view and every corner of every member marker in it, the squared
pixel residual of project(K_c, dist_c, R_c (R_t X + t_t) + t_c) - x, (R_t, t_t) the board in the rig frame at instant t.

Scenes: cameras 0.25 m apart on a line, toed in by 0.08 rad per camera (or on a ring, looking inward, for the 16-camera case), each with its
own K near 600 px at 640 x 480 and ndist 5, 4, 0 in turn; a 3 x 2 board of 0.05 m markers 0.7 - 1.0 m away; show[t][c] lists the board
markers view (t, c) sees, so that chains and islands can be made."""
import numpy as np

from tests import board3d_ref, pose_ref
from tests.map_ref import compose, inverse
from tests.planar_ref import brown_project, object_points, rodrigues, rodrigues_inv

W, H = 640, 480
MARKER_SIZE = pose_ref.MARKER_SIZE
BASELINE, TOE_IN = 0.25, 0.08
DIST5 = np.array([-0.08, 0.03, 8e-4, -5e-4, 0.01])
NDIST = (5, 4, 0)
MAX_CAMERAS, MAX_BOARD = 16, 128
Z_RANGE = (0.7, 1.0)
IDENTITY = (np.eye(3), np.zeros(3))


def rot_y(a):
    return np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])


# ---------------------------------------------------------------------------------------------
# boards and scenes
# ---------------------------------------------------------------------------------------------
def grid_board(cols=3, rows=2, size=MARKER_SIZE, gap=0.01, first_id=10):
    """(ids [n], obj [n,4,3] float32, metres) of a centred cols x rows grid in z = 0, the corners in the order of Marker::getObjectPoints."""
    P = object_points(size)
    pitch = size + gap
    obj = []
    for r in range(rows):
        for c in range(cols):
            obj.append(P + np.array([(c - (cols - 1) / 2.0) * pitch, ((rows - 1) / 2.0 - r) * pitch, 0.0]))
    return np.arange(first_id, first_id + cols * rows, dtype=np.int32), np.array(obj).astype(np.float32)


def make_cameras(ncams, seed, ring=False):
    """List of dicts K (float32-exact), dist (None, 4 or 5 float32-exact coefficients), T = (R_c, t_c) rig -> camera, Q / p the camera's
    orientation and position in the rig frame. Line: camera c at x = 0.25 c, turned TOE_IN c towards the others. Ring: the cameras on a
    circle 0.85 m in radius, looking at its centre."""
    rng = np.random.default_rng(seed)
    cams = []
    for c in range(ncams):
        K = np.array([[600.0 + rng.uniform(-15, 15), 0.0, 320.0 + rng.uniform(-8, 8)], [0.0, 600.0 + rng.uniform(-15, 15), 240.0 + rng.uniform(-8, 8)],
                      [0.0, 0.0, 1.0]]).astype(np.float32).astype(np.float64)
        nd = NDIST[c % 3]
        dist = (DIST5[:nd] * (1.0 + 0.05 * (c % 5))).astype(np.float32).astype(np.float64) if nd else None
        if ring:
            phi, rad = 2 * np.pi * c / ncams, 0.85
            Q, p = rot_y(-phi), np.array([rad * np.sin(phi), 0.0, rad - rad * np.cos(phi)])
        else:
            Q, p = rot_y(-TOE_IN * c), np.array([BASELINE * c, 0.0, 0.0])
        cams.append({"K": K, "dist": dist, "T": (Q.T, -Q.T @ p), "Q": Q, "p": p})
    return cams


def make_scene(ncams, show, seed, board=None, ring=False, tilt=0.4):
    """show[t][c]: the board markers (indices) view (t, c) sees, empty for none. The board of instant t stands in front of the cameras that
    see it, 0.7 - 1.0 m away along their mean viewing direction, facing them, tilted by up to `tilt`."""
    rng = np.random.default_rng(seed)
    board = grid_board() if board is None else board
    cams = make_cameras(ncams, seed + 1, ring)
    poses = []
    for t, row in enumerate(show):
        seen = [c for c in range(ncams) if len(row[c])] or [0]
        f = np.mean([cams[c]["Q"][:, 2] for c in seen], axis=0)
        Q = rot_y(np.arctan2(f[0], f[2]))
        centre = np.mean([cams[c]["p"] for c in seen], axis=0)
        R = Q @ pose_ref.facing_rotation(rng, rng.uniform(0.0, tilt))
        poses.append((R, centre + Q @ np.array([rng.uniform(-0.04, 0.04), rng.uniform(-0.04, 0.04), rng.uniform(*Z_RANGE)])))
    return {"ncams": ncams, "ninstants": len(show), "cams": cams, "ids": board[0], "obj": board[1], "show": [[tuple(s) for s in row] for row in show],
            "poses": poses}


def everyone(ncams, ninstants, nboard=6):
    return [[tuple(range(nboard))] * ncams for _ in range(ninstants)]


def project(cam, pose, X):
    """pixels of board points X [n,3] at board pose `pose` (rig frame) through camera `cam`"""
    T = compose(cam["T"], pose)
    return brown_project(np.asarray(X, np.float64).reshape(-1, 3), T[0], T[1], cam["K"], cam["dist"])


def observe(scene, noise=0.0, seed=0):
    """The scene's observations as the C ABI takes them: (view int32 [n], id int32 [n], corners float32 [n][8]), views in order, markers in
    board order. Projection in float64, optional Gaussian noise, rounded to float32."""
    rng = np.random.default_rng(seed)
    nc = scene["ncams"]
    vs, ids, cs = [], [], []
    for t, row in enumerate(scene["show"]):
        for c in range(nc):
            for m in row[c]:
                px = project(scene["cams"][c], scene["poses"][t], scene["obj"][m])
                if noise > 0:
                    px = px + rng.normal(0.0, noise, px.shape)
                vs.append(t * nc + c), ids.append(scene["ids"][m]), cs.append(px.reshape(8))
    return (np.array(vs, np.int32), np.array(ids, np.int32), np.array(cs, np.float64).reshape(-1, 8).astype(np.float32))


def cam_dicts(scene, truth=False):
    """the cameras as Handle.rig_calibrate / rig_pose take them; truth: with the true transforms, calibrated"""
    out = []
    for cam in scene["cams"]:
        d = {"K": cam["K"], "dist": cam["dist"]}
        if truth:
            d.update(calibrated=True, rvec=rodrigues_inv(cam["T"][0]), tvec=cam["T"][1])
        out.append(d)
    return out


# ---------------------------------------------------------------------------------------------
# which observations count, start values
# ---------------------------------------------------------------------------------------------
def select(obs, cams, board_ids, obj, ninstants, min_markers=1):
    """Per view dict(members [(board index, corners float64 [4,2])] in detection order, the first of a repeated id; n; V = (R, t) the
    single-camera pose or None; counted)."""
    vs, ids, cs = obs
    nc = len(cams)
    index = {}
    for j, b in enumerate(board_ids):
        index.setdefault(int(b), j)
    views = [{"members": [], "seen": set()} for _ in range(ninstants * nc)]
    for v, i, c in zip(vs, ids, cs):
        if not 0 <= v < len(views) or int(i) not in index or index[int(i)] in views[v]["seen"]:
            continue
        views[v]["seen"].add(index[int(i)])
        views[v]["members"].append((index[int(i)], np.asarray(np.float32(c), np.float64).reshape(4, 2)))
    obj = np.asarray(obj, np.float64).reshape(-1, 4, 3)
    for v, view in enumerate(views):
        view["n"] = len(view["members"])
        view["V"] = None
        if view["n"] >= 1:
            cam = cams[v % nc]
            X = np.concatenate([obj[b] for b, _ in view["members"]])
            x = np.concatenate([c for _, c in view["members"]])
            s = board3d_ref.solve(X, x, cam["K"], cam["dist"])
            if s is not None and np.all(np.isfinite(s["rvec"])) and np.all(np.isfinite(s["tvec"])):
                view["V"] = (rodrigues(s["rvec"]), np.asarray(s["tvec"], np.float64))
        view["counted"] = view["n"] >= min_markers and view["V"] is not None
    return views


def instant_start(views, t, nc, T, calibrated):
    """(number of counted views of calibrated cameras, the instant's start pose T_c^-1 V_tc from the one with the most member markers, ties
    to the lower camera)"""
    act = [c for c in range(nc) if views[t * nc + c]["counted"] and calibrated[c]]
    if not act:
        return 0, None
    best = max(act, key=lambda c: (views[t * nc + c]["n"], -c))
    return len(act), compose(inverse(T[best]), views[t * nc + best]["V"])


def start_values(views, nc, ninstants):
    """dict(T [nc] of (R, t), calibrated [nc], used [ninstants], poses {t: (R, t)}, depth [nc]); None when no eligible instant shows camera 0
    or no camera besides camera 0 is reached."""
    counted = np.array([v["counted"] for v in views]).reshape(ninstants, nc)
    n = np.array([v["n"] for v in views]).reshape(ninstants, nc)
    eligible = counted.sum(axis=1) >= 2
    if not np.any(eligible & counted[:, 0]):
        return None
    score = -np.ones((nc, nc), int)
    at = -np.ones((nc, nc), int)
    for a in range(nc):
        for b in range(nc):
            for t in range(ninstants):
                if a != b and eligible[t] and counted[t, a] and counted[t, b] and min(n[t, a], n[t, b]) > score[a, b]:
                    score[a, b], at[a, b] = min(n[t, a], n[t, b]), t
    T = [IDENTITY] + [None] * (nc - 1)
    reached, depth = [True] + [False] * (nc - 1), [0] * nc
    while True:
        cand = []
        for b in range(nc):
            if reached[b]:
                continue
            edges = [(score[a, b], -a) for a in range(nc) if reached[a] and at[a, b] >= 0]
            if edges:
                s, na = max(edges)
                cand.append((s, -b, -na))
        if not cand:
            break
        _, nb, a = max(cand)
        b = -nb
        t = at[a, b]
        T[b] = compose(views[t * nc + b]["V"], compose(inverse(views[t * nc + a]["V"]), T[a]))
        reached[b], depth[b] = True, depth[a] + 1
    if sum(reached) < 2:
        return None
    used, poses = np.zeros(ninstants, bool), {}
    for t in range(ninstants):
        cnt, p = instant_start(views, t, nc, T, reached)
        if cnt >= 2:
            used[t], poses[t] = True, p
    return {"T": T, "calibrated": np.array(reached), "used": used, "poses": poses, "depth": depth}


# ---------------------------------------------------------------------------------------------
# the cost and its scipy solve
# ---------------------------------------------------------------------------------------------
def _rodrigues_many(r):
    th = np.linalg.norm(r, axis=1)
    k = r / np.maximum(th, 1e-300)[:, None]
    Kx = np.zeros((len(r), 3, 3))
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0] = -k[:, 2], k[:, 1], k[:, 2]
    Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -k[:, 0], -k[:, 1], k[:, 0]
    return np.eye(3) + np.sin(th)[:, None, None] * Kx + (1 - np.cos(th))[:, None, None] * (Kx @ Kx)


class Problem:
    """The points of the views that take part. free_cams: x = [rvec, tvec of the calibrated cameras but 0 | rvec, tvec of the instants];
    else the cameras are fixed at T and x holds the instants only."""

    def __init__(self, views, cams, obj, nc, instants, calibrated, T=None, free_cams=True):
        obj = np.asarray(obj, np.float64).reshape(-1, 4, 3)
        self.nc, self.free_cams = nc, free_cams
        self.cams = [c for c in range(1, nc) if calibrated[c]] if free_cams else []
        self.instants = list(instants)
        ci = {c: k + 1 for k, c in enumerate(self.cams)}
        self.fixed = None if free_cams else np.array([np.concatenate([rodrigues_inv(T[c][0]), T[c][1]]) if calibrated[c] else np.zeros(6) for c in range(nc)])
        pc, pt, X, px, intr, view = [], [], [], [], [], []
        for k, t in enumerate(self.instants):
            for c in range(nc):
                vw = views[t * nc + c]
                if not (vw["counted"] and calibrated[c]):
                    continue
                cam = cams[c]
                d = np.zeros(5)
                if cam["dist"] is not None:
                    d[:len(cam["dist"])] = cam["dist"]
                for b, crn in vw["members"]:
                    for q in range(4):
                        pc.append(ci.get(c, 0) if free_cams else c), pt.append(k), X.append(obj[b, q]), px.append(crn[q]), view.append(t * nc + c)
                        intr.append([cam["K"][0, 0], cam["K"][1, 1], cam["K"][0, 2], cam["K"][1, 2], *d])
        self.pc, self.pt, self.X, self.px = np.array(pc), np.array(pt), np.array(X), np.array(px)
        self.intr, self.view = np.array(intr), np.array(view)

    def pack(self, T, poses):
        x = [np.concatenate([rodrigues_inv(T[c][0]), T[c][1]]) for c in self.cams]
        x += [np.concatenate([rodrigues_inv(poses[t][0]), poses[t][1]]) for t in self.instants]
        return np.concatenate(x) if x else np.zeros(0)

    def unpack(self, x):
        n = len(self.cams)
        pc = np.concatenate([np.zeros((1, 6)), x[:6 * n].reshape(n, 6)]) if self.free_cams else self.fixed
        return pc, x[6 * n:].reshape(len(self.instants), 6)

    def residuals(self, x):
        pc, pt = self.unpack(x)
        Rc, Rt = _rodrigues_many(pc[:, :3]), _rodrigues_many(pt[:, :3])
        P = np.einsum("nij,nj->ni", Rt[self.pt], self.X) + pt[self.pt, 3:]
        Xc = np.einsum("nij,nj->ni", Rc[self.pc], P) + pc[self.pc, 3:]
        xn, yn = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
        r2 = xn * xn + yn * yn
        i = self.intr
        rad = 1 + i[:, 4] * r2 + i[:, 5] * r2 ** 2 + i[:, 8] * r2 ** 3
        xd = xn * rad + 2 * i[:, 6] * xn * yn + i[:, 7] * (r2 + 2 * xn * xn)
        yd = yn * rad + i[:, 6] * (r2 + 2 * yn * yn) + 2 * i[:, 7] * xn * yn
        return np.stack([i[:, 0] * xd + i[:, 2] - self.px[:, 0], i[:, 1] * yd + i[:, 3] - self.px[:, 1]], axis=-1)

    def sparsity(self):
        """which unknowns a residual depends on: its camera's six (none for camera 0 or fixed cameras) and its instant's six"""
        from scipy.sparse import coo_matrix

        n, npts = len(self.cams), len(self.pt)
        rows, cols = [], []
        for blk, on in ((6 * (self.pc - 1), self.pc > 0 if self.free_cams else np.zeros(npts, bool)), (6 * n + 6 * self.pt, np.ones(npts, bool))):
            pts = np.nonzero(on)[0]
            for res in range(2):
                for k in range(6):
                    rows.append(2 * pts + res), cols.append(blk[pts] + k)
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        return coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(2 * npts, 6 * n + 6 * len(self.instants))).tocsr()

    def solve(self, x0, method="lm", sparse=False):
        """sparse: trf with the Jacobian's sparsity, for problems too large for a dense numeric Jacobian"""
        from scipy.optimize import least_squares

        kw = dict(xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=400 * (len(x0) + 1))
        if method == "trf":
            kw.update(jac="3-point", x_scale="jac", max_nfev=400)
        if sparse:
            kw.update(jac_sparsity=self.sparsity(), tr_solver="lsmr")
        return least_squares(lambda x: self.residuals(x).ravel(), x0, method=method, **kw).x

    def rms(self, x):
        r = self.residuals(x)
        return float(np.sqrt(np.sum(r * r) / len(r)))

    def camera_rms(self, x):
        e2 = np.sum(self.residuals(x) ** 2, axis=1)
        cam = self.view % self.nc
        return np.array([np.sqrt(e2[cam == c].sum() / max((cam == c).sum(), 1)) for c in range(self.nc)])

    def transforms(self, x):
        """([(R, t)] for camera 0 and the free cameras in order (or every camera when they are fixed), {t: (R, t)})"""
        pc, pt = self.unpack(x)
        return [(rodrigues(p[:3]), p[3:]) for p in pc], {t: (rodrigues(p[:3]), p[3:]) for t, p in zip(self.instants, pt)}


def reference(obs, cams, board_ids, obj, ninstants, min_markers=1, truth=None):
    """The whole calibration reference: selection, start values, scipy solve. dict(T [nc] (zeros-transform None for a camera that is not
    calibrated), calibrated, used, poses, rms, camera_rms, start_T, views, problem, x); with truth = (T, poses) also truth_T / truth_rms:
    a second, independent solve (trf) started at the truth. None where the call must fail."""
    nc = len(cams)
    views = select(obs, cams, board_ids, obj, ninstants, min_markers)
    sv = start_values(views, nc, ninstants)
    if sv is None:
        return None
    inst = [t for t in range(ninstants) if sv["used"][t]]
    prob = Problem(views, cams, obj, nc, inst, sv["calibrated"])
    x = prob.solve(prob.pack(sv["T"], sv["poses"]))

    def spread(x):
        Tc, poses = prob.transforms(x)
        T = [None] * nc
        for c, Tk in zip([0] + prob.cams, Tc):
            T[c] = Tk
        return T, poses

    T, poses = spread(x)
    out = {"T": T, "calibrated": sv["calibrated"], "used": sv["used"], "poses": poses, "rms": prob.rms(x), "camera_rms": prob.camera_rms(x),
           "start_T": sv["T"], "start_poses": sv["poses"], "depth": sv["depth"], "views": views, "problem": prob, "x": x}
    if truth is not None:
        xt = prob.solve(prob.pack(truth[0], {t: truth[1][t] for t in inst}), method="trf")
        out["truth_T"], out["truth_rms"] = spread(xt)[0], prob.rms(xt)
    return out


def pose_reference(obs, cams, T, calibrated, board_ids, obj, ninstants, min_markers=1):
    """The rig pose reference: per instant None (no counted view of a calibrated camera) or dict(pose (R, t) the scipy minimum of the joint
    cost from the start, start, views_used, n_markers)."""
    nc = len(cams)
    views = select(obs, cams, board_ids, obj, ninstants, min_markers)
    out = []
    for t in range(ninstants):
        cnt, start = instant_start(views, t, nc, T, calibrated)
        if cnt < 1:
            out.append(None)
            continue
        prob = Problem(views, cams, obj, nc, [t], calibrated, T=T, free_cams=False)
        x = prob.solve(prob.pack(T, {t: start}))
        out.append({"pose": prob.transforms(x)[1][t], "start": start, "views_used": cnt,
                    "n_markers": sum(views[t * nc + c]["n"] for c in range(nc) if views[t * nc + c]["counted"] and calibrated[c])})
    return out


# ---------------------------------------------------------------------------------------------
# measures
# ---------------------------------------------------------------------------------------------
def cam_dev(Ta, Tb, obj, cams=None):
    """Largest distance in metres between the board's points, taken 1 m in front of the rig, pushed through two sets of camera transforms."""
    P = np.asarray(obj, np.float64).reshape(-1, 3) + np.array([0.0, 0.0, 1.0])
    worst = 0.0
    for c in (range(len(Ta)) if cams is None else cams):
        if Ta[c] is None or Tb[c] is None:
            continue
        worst = max(worst, float(np.max(np.linalg.norm((P @ Ta[c][0].T + Ta[c][1]) - (P @ Tb[c][0].T + Tb[c][1]), axis=1))))
    return worst


def board_dev(pa, pb, obj):
    """Largest distance in metres between the board's points in the rig frame at two poses."""
    X = np.asarray(obj, np.float64).reshape(-1, 3)
    return float(np.max(np.linalg.norm((X @ pa[0].T + pa[1]) - (X @ pb[0].T + pb[1]), axis=1)))


def device_T(r):
    """[(R, t) or None] of Handle.rig_calibrate's result"""
    return [(rodrigues(rv), tv) if cal else None for rv, tv, cal in zip(r["rvecs"], r["tvecs"], r["calibrated"])]


# ---------------------------------------------------------------------------------------------
# the cases of the tests
# ---------------------------------------------------------------------------------------------
def _chain_show():
    return [[tuple(range(6)) if c in ((0, 1) if t % 2 == 0 else (1, 2)) else () for c in range(3)] for t in range(6)]


def _island_show():
    return [[tuple(range(6)) if (c < 2) == (t < 4) else () for c in range(3)] for t in range(6)]


def _ring_show(nc=16, ninstants=32):
    return [[tuple(range(6)) if c in (t % nc, (t + 1) % nc) else () for c in range(nc)] for t in range(ninstants)]


SCENES = {
    "three": lambda seed: make_scene(3, everyone(3, 8), 500 + seed),
    "pair1": lambda seed: make_scene(2, [[(2,), (3,)]], 510 + seed),
    "pair2": lambda seed: make_scene(2, everyone(2, 2), 520 + seed),
    "chain": lambda seed: make_scene(3, _chain_show(), 530 + seed),
    "island": lambda seed: make_scene(3, _island_show(), 540 + seed),
    "ring16": lambda seed: make_scene(16, _ring_show(), 550 + seed, ring=True),
    "full128": lambda seed: make_scene(2, everyone(2, 2, 128), 560 + seed, board=grid_board(16, 8, 0.012, 0.003, 100)),
}
_cache = {}


def case(name, noise=0.0, seed=0, solve=True):
    """A scene with its observations and (solve) its reference, computed once per process: dict(scene, obs, ref)."""
    key = (name, noise, seed, solve)
    if key not in _cache:
        sc = SCENES[name](seed)
        obs = observe(sc, noise, 1000 + seed)
        ref = None
        if solve:
            ref = reference(obs, sc["cams"], sc["ids"], sc["obj"], sc["ninstants"], truth=([c["T"] for c in sc["cams"]], sc["poses"]))
        _cache[key] = {"scene": sc, "obs": obs, "ref": ref}
    return _cache[key]


def truth_T(scene):
    return [c["T"] for c in scene["cams"]]
