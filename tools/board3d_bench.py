#!/usr/bin/env python3
"""What arucohip_board_detect_batch costs on a planar board, on a folded one and on a planar board written out of z = 0.

One process, one case (run it per library for an A/B: ARUCOHIP_LIB names a variant build):
  --case planar : --frames device-resident 4K frames of the bench's board stream (synth.make_board_stream as bench.py --config 4 sets it
                  up; --distinct frames are rendered and repeated). The planar start, the path every board took before boards out of a
                  plane were posed.
  --case fold   : 1280 x 720, the board's 24 markers as two panels of 12 placed at +-45 degrees about a common hinge with
                  arucohip_board_place (a 90 degree fold that opens towards the camera), 8 rendered views repeated: the DLT start.
  --case lifted : 1280 x 720, 8 views of the planar board, its configuration moved by a rigid transform with arucohip_board_place: the
                  tilted-plane start.
detect_batch once (untimed), then --warmup + --runs calls of board_detect_batch, each between two events on the handle's stream, boards and
prob returned to the host. Prints one JSON line: the median, the runs, and how many members and poses the frames gave."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from aruco_amd import capi, synth
from aruco_amd.fixtures import load_case

ap = argparse.ArgumentParser()
ap.add_argument("--case", choices=("planar", "fold", "lifted"), default="planar")
ap.add_argument("--frames", type=int, default=1024)
ap.add_argument("--distinct", type=int, default=128)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
a = ap.parse_args()
assert torch.cuda.is_available(), "board3d_bench.py needs a GPU"
UNIT, SIZE, CAP, N = 0.039 / 100.0, 0.039, 64, a.frames
_, doc = load_case("board")
board = doc["board_conf"]
ids, obj = [int(i) for i in board["ids"]], np.asarray(board["obj"], np.float64).reshape(-1, 4, 3)
W, H = (3840, 2160) if a.case == "planar" else (1280, 720)
K = np.array(doc["intrinsics"]["K"], np.float32).reshape(3, 3)   # CameraParameters::resize rule, as bench.py
K[0, 0] *= np.float32(W / 640.0); K[0, 2] *= np.float32(W / 640.0)
K[1, 1] *= np.float32(H / 480.0); K[1, 2] *= np.float32(H / 480.0)


def render_panels(panels, rvec, tvec, rng, pad=40.0):
    """synth.render_board for panels that are not in one plane: per panel (ids, placed obj, placed sheet) a white sheet, then its markers."""
    img = torch.full((H, W), float(rng.uniform(90, 130)), dtype=torch.float32, device="cuda")
    white = rng.uniform(215, 240)
    Kd = K.astype(np.float64)
    for pid, pobj, sheet in panels:
        synth._paint_quad(img, synth.project(Kd, rvec, tvec, sheet * UNIT), np.full((1, 1), white, np.float32), 1, 0)
        for mid, o in zip(pid, pobj):
            synth._paint_quad(img, synth.project(Kd, rvec, tvec, o * UNIT), synth._marker_table(int(mid), 0, rng.uniform(15, 40), white), 7, 0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(int(rng.randint(0, 2 ** 31 - 1)))
    img = img + torch.randn(img.shape, generator=gen, device="cuda") * 1.5
    return img.round().clamp(0, 255).to(torch.uint8)


if a.case == "planar":
    D = min(a.distinct, N)
    distinct, _ = synth.make_board_stream(D, ids, obj, K.reshape(-1), width=W, height=H, seed=4711, device="cuda")
    use_obj = obj
elif a.case == "lifted":
    D = 8
    distinct, _ = synth.make_board_stream(D, ids, obj, K.reshape(-1), width=W, height=H, seed=4711, device="cuda")
    # the same board, its file written in another frame: p -> R p + t in board units
    use_obj = capi.board_place(obj, [0.3, -0.5, 0.2], [250.0, -120.0, 640.0]).astype(np.float64)
else:
    D = 8
    ctr = (obj.reshape(-1, 3).min(axis=0) + obj.reshape(-1, 3).max(axis=0)) / 2
    order = np.argsort([o[:, 0].mean() for o in obj], kind="stable")   # the board's left and right halves by marker centre
    halves = [np.sort(order[:len(ids) // 2]), np.sort(order[len(ids) // 2:])]
    panels, use_obj = [], np.zeros_like(obj)
    for side, idx in enumerate(halves):
        p = obj[idx] - ctr
        lo, hi = p.reshape(-1, 3).min(axis=0), p.reshape(-1, 3).max(axis=0)
        hinge = np.array([hi[0] + 60.0, 0, 0]) if side == 0 else np.array([lo[0] - 60.0, 0, 0])   # 60 board units of sheet beside the hinge
        rv = np.array([0.0, -np.pi / 4 if side == 0 else np.pi / 4, 0.0])
        Rm = synth._rodrigues(rv)
        tv = -Rm @ hinge
        sheet = np.array([[[lo[0] - 40, lo[1] - 40, 0], [hi[0] + 40, lo[1] - 40, 0], [hi[0] + 40, hi[1] + 40, 0], [lo[0] - 40, hi[1] + 40, 0]]])
        placed = capi.board_place(p, rv, tv).astype(np.float64)
        use_obj[idx] = placed
        panels.append(([ids[i] for i in idx], placed, capi.board_place(sheet, rv, tv).astype(np.float64)[0]))
    rng = np.random.RandomState(4711)
    distinct = torch.empty((D, H, W), dtype=torch.uint8, device="cuda")
    for f in range(D):
        rvec = rng.uniform(-0.2, 0.2, 3)
        tvec = np.array([rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), rng.uniform(0.6, 0.7)])
        distinct[f] = render_panels(panels, rvec, tvec, rng)
frames = distinct.repeat((N + D - 1) // D, 1, 1)[:N].contiguous()
del distinct
torch.cuda.synchronize()
h = capi.Handle(W, H, max_batch=N)
stream = torch.cuda.ExternalStream(h.get_stream())
out = torch.zeros((N, CAP * 96), dtype=torch.uint8, device="cuda")
cnt = torch.zeros(N, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
h.detect_batch_device(frames.data_ptr(), N, W, H, out.data_ptr(), CAP, cnt.data_ptr(), K=K, marker_size=SIZE)
h.batch_status()

times, boards = [], None
for i in range(a.warmup + a.runs):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    boards = h.board_detect_batch(N, ids, use_obj, board["info_type"], K, [0.0] * 5, SIZE)
    e1.record(stream)
    e1.synchronize()
    if i >= a.warmup:
        times.append(e0.elapsed_time(e1))
print(json.dumps({"case": a.case, "library": capi.load().arucohip_build_info().decode(), "frames": N, "distinct_frames": D, "width": W, "height": H,
                  "runs": a.runs, "board_detect_batch_ms": round(float(np.median(times)), 3), "runs_ms": [round(t, 3) for t in times],
                  "min_ms": round(min(times), 3), "max_ms": round(max(times), 3),
                  "members_per_frame": round(float(np.mean([b["n_markers"] for b in boards])), 2),
                  "frames_with_pose": int(sum(b["has_pose"] for b in boards))}))
h.close()
