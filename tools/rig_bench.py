#!/usr/bin/env python3
"""What arucohip_rig_pose_batch and arucohip_rig_calibrate_batch cost on an eight-camera batch, next to arucohip_board_detect_batch on the
same batch (the one-camera-at-a-time answer the rig pose replaces).

--frames device-resident 1080p frames of the bench's 24-marker board: --instants distinct instants of eight cameras are rendered (camera c
looks at the board of instant t through its own small rigid transform, so the views of an instant belong to one rig) and repeated; frame
f is view f = instant * 8 + camera. detect_batch once (untimed), then for each of the three calls --warmup + --runs calls with the host
clock around the synchronous call. Prints one JSON line: medians, runs, accepted steps, how far the calibrated transforms are from the
ones the frames were drawn with. --dump FILE.npz: the detections (view, id, corners) and the rig, for the host model's scipy solve."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from aruco_amd import capi, synth
from aruco_amd.fixtures import load_case

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=1024)
ap.add_argument("--instants", type=int, default=8)
ap.add_argument("--runs", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--dump", default="")
a = ap.parse_args()
assert torch.cuda.is_available(), "rig_bench.py needs a GPU"
NC, UNIT, SIZE, CAP, N, W, H = 8, 0.039 / 100.0, 0.039, 64, a.frames, 1920, 1080
assert N % NC == 0
_, doc = load_case("board")
board = doc["board_conf"]
ids, obj = [int(i) for i in board["ids"]], np.asarray(board["obj"], np.float64).reshape(-1, 4, 3)
K = np.array(doc["intrinsics"]["K"], np.float32).reshape(3, 3)   # CameraParameters::resize rule, as bench.py
K[0, 0] *= np.float32(W / 640.0); K[0, 2] *= np.float32(W / 640.0)
K[1, 1] *= np.float32(H / 480.0); K[1, 2] *= np.float32(H / 480.0)

# the rig the frames are drawn with: the board fills most of the image, so the cameras stand close together
rig = [(np.zeros(3), np.zeros(3))] + [(np.array([0.0, 0.012 * (c - 3.5), 0.004 * c]), np.array([0.006 * c - 0.02, 0.003 * (c % 3), 0.002 * c])) for c in range(1, NC)]
rng = np.random.RandomState(4711)
D = a.instants * NC
distinct = torch.empty((D, H, W), dtype=torch.uint8, device="cuda")
for t in range(a.instants):
    rv, tv = rng.uniform(-0.2, 0.2, 3), np.array([rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), rng.uniform(0.52, 0.60)])
    Rt = synth._rodrigues(rv)
    for c, (rc, tc) in enumerate(rig):
        Rc = synth._rodrigues(rc)
        R = Rc @ Rt
        # rotation matrix -> vector for synth.render_board
        ang = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
        ax = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
        rvec = ax / max(np.linalg.norm(ax), 1e-300) * ang
        distinct[t * NC + c], _ = synth.render_board(ids, obj, K.astype(np.float64), rvec, Rc @ tv + tc, W, H, rng, device="cuda", unit=UNIT)
frames = distinct.repeat((N + D - 1) // D, 1, 1)[:N].contiguous()
del distinct
torch.cuda.synchronize()
h = capi.Handle(W, H, max_batch=N)
out = torch.zeros((N, CAP * 96), dtype=torch.uint8, device="cuda")
cnt = torch.zeros(N, dtype=torch.int32, device="cuda")
h.detect_batch_device(frames.data_ptr(), N, W, H, out.data_ptr(), CAP, cnt.data_ptr(), K=K, marker_size=SIZE)
h.batch_status()
torch.cuda.synchronize()
cams = [{"K": K, "dist": None} for _ in range(NC)]


def timed(fn):
    times, res = [], None
    for i in range(a.warmup + a.runs):
        t0 = time.perf_counter()
        res = fn()
        t1 = time.perf_counter()
        if i >= a.warmup:
            times.append((t1 - t0) * 1e3)
    return res, {"median_ms": round(float(np.median(times)), 3), "min_ms": round(min(times), 3), "max_ms": round(max(times), 3)}


boards, t_board = timed(lambda: h.board_detect_batch(N, ids, obj, board["info_type"], K, None, SIZE))
calib, t_calib = timed(lambda: h.rig_calibrate_batch(N, cams, ids, obj, board["info_type"], marker_size=SIZE))
poses, t_pose = timed(lambda: h.rig_pose_batch(N, calib["cams"], ids, obj, board["info_type"], marker_size=SIZE))
P = obj.reshape(-1, 3) * UNIT + np.array([0.0, 0.0, 0.55])
dev = max(float(np.max(np.linalg.norm((P @ synth._rodrigues(calib["rvecs"][c]).T + calib["tvecs"][c]) - (P @ synth._rodrigues(rig[c][0]).T + rig[c][1]), axis=1)))
          for c in range(NC))
if a.dump:
    mk = np.frombuffer(out.cpu().numpy().tobytes(), capi.MARKER_DTYPE).reshape(N, CAP)
    n = cnt.cpu().numpy()
    view = np.concatenate([np.full(max(int(n[f]), 0), f, np.int32) for f in range(N)])
    np.savez(a.dump, view=view, id=np.concatenate([mk[f, :max(int(n[f]), 0)]["id"] for f in range(N)]).astype(np.int32),
             corners=np.concatenate([mk[f, :max(int(n[f]), 0)]["corners"] for f in range(N)]).astype(np.float32).reshape(-1, 8), K=K, ids=np.array(ids, np.int32),
             obj=(obj * UNIT).astype(np.float32), rvecs=calib["rvecs"], tvecs=calib["tvecs"], rms=calib["rms"], rig_r=np.array([r for r, _ in rig]),
             rig_t=np.array([t for _, t in rig]))
print(json.dumps({"library": capi.load().arucohip_build_info().decode(), "frames": N, "cameras": NC, "instants": N // NC, "distinct_instants": a.instants,
                  "width": W, "height": H, "runs": a.runs, "board_detect_batch": t_board, "rig_pose_batch": t_pose, "rig_calibrate_batch": t_calib,
                  "calibrate_steps": calib["iterations"], "calibrate_rms_px": round(calib["rms"], 4), "calibrated": int(calib["calibrated"].sum()),
                  "instants_used": int(calib["used"].sum()), "against_the_drawing_m": dev,
                  "members_per_frame": round(float(np.mean([b["n_markers"] for b in boards])), 2),
                  "instants_with_pose": int(sum(p["has_pose"] for p in poses)), "views_per_instant": round(float(np.mean([p["views_used"] for p in poses])), 2)}))
h.close()
