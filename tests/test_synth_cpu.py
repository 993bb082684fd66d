"""The synthetic stream's layout sampler skips work (an occupied-centre test before the geometry, the bounds test before the quiet-zone
homography, broadcast occupancy masks) without changing what it draws: against the plain rejection sampler below, the same markers at the
same float64 corners and the random state in the same place after every frame. The bench's inputs depend on that."""
import math

import numpy as np
import torch

from aruco_amd import synth


def plain_poly_mask(shape, quad, scale):
    h, w = shape
    q = np.asarray(quad, float) / scale
    x0 = int(max(0, math.floor(q[:, 0].min()) - 1)); x1 = int(min(w, math.ceil(q[:, 0].max()) + 2))
    y0 = int(max(0, math.floor(q[:, 1].min()) - 1)); y1 = int(min(h, math.ceil(q[:, 1].max()) + 2))
    if x1 <= x0 or y1 <= y0:
        return 0, 0, 0, 0, np.zeros((0, 0), bool)
    ys, xs = np.mgrid[y0:y1, x0:x1]
    m = np.ones((y1 - y0, x1 - x0), bool)
    sign = 0
    for i in range(4):
        ax, ay = q[i]
        bx, by = q[(i + 1) % 4]
        cr = (bx - ax) * (ys + 0.5 - ay) - (by - ay) * (xs + 0.5 - ax)
        if sign == 0:
            c = (q[:, 0].mean() - ax) * (by - ay) - (q[:, 1].mean() - ay) * (bx - ax)
            sign = -1 if c > 0 else 1
        m &= (cr * sign) >= 0
    return y0, y1, x0, x1, m


def plain_frame_layout(rng, width, height, n_markers=20, side_range=(90, 220), margin=60, jitter=0.08, quiet=1, cells=7, id_pool=1024):
    """every attempt draws, builds its quads and runs every test in turn"""
    ids = rng.choice(id_pool, size=n_markers, replace=False)
    sc = 4
    occ = np.zeros(((height + sc - 1) // sc, (width + sc - 1) // sc), bool)
    out = []
    for mid in ids:
        for attempt in range(200):
            hi = side_range[1] - (side_range[1] - side_range[0]) * min(attempt / 60.0, 0.95)
            s = rng.uniform(side_range[0], max(hi, side_range[0] + 1))
            th = rng.uniform(0, 2 * math.pi)
            c, sn = abs(math.cos(th)), abs(math.sin(th))
            if s * max(c, sn) < 86:
                continue
            cx = rng.uniform(margin, width - margin)
            cy = rng.uniform(margin, height - margin)
            R = np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
            base = np.array([[-0.5, -0.5], [0.5, -0.5], [0.5, 0.5], [-0.5, 0.5]]) * s
            base = base + rng.uniform(-jitter, jitter, size=(4, 2)) * s
            quad = base @ R.T + np.array([cx, cy])
            Hm = synth._homography([(0, 0), (cells, 0), (cells, cells), (0, cells)], [tuple(p) for p in quad])
            qq = []
            for (u, v) in [(-quiet, -quiet), (cells + quiet, -quiet), (cells + quiet, cells + quiet), (-quiet, cells + quiet)]:
                p = Hm @ np.array([u, v, 1.0])
                qq.append(p[:2] / p[2])
            qq = np.array(qq)
            if quad[:, 0].min() < margin or quad[:, 0].max() > width - margin or quad[:, 1].min() < margin or \
                    quad[:, 1].max() > height - margin:
                continue
            if qq[:, 0].min() < 2 or qq[:, 0].max() > width - 3 or qq[:, 1].min() < 2 or qq[:, 1].max() > height - 3:
                continue
            d = np.roll(qq, -1, axis=0) - qq
            cr = d[:, 0] * np.roll(d, -1, axis=0)[:, 1] - d[:, 1] * np.roll(d, -1, axis=0)[:, 0]
            if not (np.all(cr > 0) or np.all(cr < 0)):
                continue
            ctr = qq.mean(axis=0)
            grown = ctr + (qq - ctr) * (1 + 10.0 / s)
            y0, y1, x0, x1, m = plain_poly_mask(occ.shape, grown, sc)
            if (m & occ[y0:y1, x0:x1]).any():
                continue
            occ[y0:y1, x0:x1] |= m
            out.append({"id": int(mid), "quad": quad, "quad_q": qq})
            break
    return out


def _same_layouts(n_frames, width, height, seed, **kw):
    a, b = np.random.RandomState(seed), np.random.RandomState(seed)
    for _ in range(n_frames):
        la, lb = plain_frame_layout(a, width, height, **kw), synth.frame_layout(b, width, height, **kw)
        assert [m["id"] for m in la] == [m["id"] for m in lb]
        for p, q in zip(la, lb):
            assert p["quad"].tobytes() == q["quad"].tobytes() and p["quad_q"].tobytes() == q["quad_q"].tobytes()
        sa, sb = a.get_state(), b.get_state()
        assert sa[1].tobytes() == sb[1].tobytes() and sa[2:] == sb[2:]


def test_layout_of_the_bench_stream_equals_the_plain_sampler():
    # make_stream's arguments at 1080p (the bench's stream, seed 4711) and at a quarter of the area with few markers
    _same_layouts(24, 1920, 1080, 4711, n_markers=20, side_range=(90.0, 220.0), margin=60)
    _same_layouts(8, 960, 540, 3, n_markers=5, side_range=(45.0, 110.0), margin=30)


def test_layout_of_hrm_frames_equals_the_plain_sampler():
    # make_hrm_frame's arguments: 1280x720, larger markers, 6x6 cells
    s = 1280 / 1920.0
    _same_layouts(4, 1280, 720, 7, n_markers=10, side_range=(110 * s * 1.5, 220 * s * 1.5), margin=int(60 * s), cells=6, id_pool=12)


def test_stream_frames_render_from_their_layouts():
    # what make_stream returns is the frames it rendered for those layouts, on the same draws
    frames, truth = synth.make_stream(2, width=960, height=540, seed=3, n_markers=5)
    rng = np.random.RandomState(3)
    for f in range(2):
        lay = plain_frame_layout(rng, 960, 540, n_markers=5, side_range=(45.0, 110.0), margin=30)
        assert [m["id"] for m in lay] == [m["id"] for m in truth[f]]
        assert torch.equal(synth.render_frame(lay, 960, 540, rng), frames[f])
