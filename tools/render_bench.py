#!/usr/bin/env python3
"""What mesh rendering costs ("Mesh rendering"). One process, N device-resident three-channel frames of 1920 x 1080 of
synth.make_stream with the bench's 20 markers each, posed by one arucohip_detect_batch with the bench's camera (markers and counts stay
on the device). Warmed, alternating, event-timed legs (the median of --runs per leg), as tools/ingest_bench.py alternates its legs:

  cube           arucohip_render_markers_batch, the 12-triangle cube, scale 1
  sphere         ... a 960-triangle sphere (uv_sphere_mesh(21, 24)), scale 1
  cube_int64 / sphere_int64   the same with ARUCOHIP_RENDER_EDGES_INT64: the edge functions in int64 instead of double
  draw_cube      arucohip_draw_markers_batch with ARUCOHIP_DRAW_CUBE on the same frames: the wireframe overlay, a familiar yardstick

Every leg paints over what the one before left: the work of a render call does not depend on the bytes of the frames. After the timed
legs, one further call per mesh with arucohip_enable_timing gives the build kernels' (instances, vertices, triangles) and the raster
kernel's own event times. Prints one JSON line with arucohip_build_info()."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from aruco_amd import capi, synth

W, H, CAP = 1920, 1080, 64
K = [1400, 0, 960, 0, 1400, 540, 0, 0, 1]
DIST = [-0.10, 0.02, 1e-3, -5e-4, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "render_bench.py needs a GPU"
    N = a.frames
    grey, _ = synth.make_stream(N, seed=4711, device="cuda")
    h = capi.Handle(W, H, max_batch=N)
    stream = torch.cuda.ExternalStream(h.get_stream())
    out = torch.zeros((N, CAP * capi.MARKER_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(N, dtype=torch.int32, device="cuda")
    h.detect_batch_device(grey.data_ptr(), N, W, H, out.data_ptr(), CAP, cnt.data_ptr(), K=K, dist=DIST, marker_size=0.05)
    h.synchronize()
    markers = out.cpu().numpy().view(capi.MARKER_DTYPE).reshape(N, CAP)
    counts = cnt.cpu().numpy()
    posed = int(sum(markers[f, :max(counts[f], 0)]["has_pose"].sum() for f in range(N)))
    frames = grey[..., None].expand(N, H, W, 3).contiguous()
    del grey
    meshes = {}
    for name, (v, t) in (("cube", capi.cube_mesh()), ("sphere", capi.uv_sphere_mesh(21, 24))):
        meshes[name] = (capi.mesh(torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda()), len(t))
    assert meshes["cube"][1] == 12 and meshes["sphere"][1] == 960
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def render(name, flags=capi.RENDER_CULL_BACK):
        h.render_markers_device(frames.data_ptr(), N, W, H, 3, out.data_ptr(), CAP, cnt.data_ptr(), K, meshes[name][0], capi.render_style(flags=flags), DIST)

    def draw_cube():
        h.draw_markers(frames, out, cnt, K=K, dist=DIST, flags=capi.DRAW_CUBE)

    legs = {"cube": lambda: render("cube"), "sphere": lambda: render("sphere"),
            "cube_int64": lambda: render("cube", capi.RENDER_CULL_BACK | capi.RENDER_EDGES_INT64),
            "sphere_int64": lambda: render("sphere", capi.RENDER_CULL_BACK | capi.RENDER_EDGES_INT64), "draw_cube": draw_cube}
    times = {k: [] for k in legs}
    for i in range(a.warmup + a.runs):
        for k, fn in legs.items():   # alternating: every leg sees the same drift of the machine
            ms = timed(fn)
            if i >= a.warmup:
                times[k].append(ms)
    res = {"frames": N, "width": W, "height": H, "channels": 3, "cap": CAP, "posed_markers": posed, "runs": a.runs, "warmup": a.warmup,
           "build_info": capi.build_info(), "device": torch.cuda.get_device_name(0), "legs": {}}
    for k, v in times.items():
        ms = float(np.median(v))
        res["legs"][k] = {"ms_per_batch": round(ms, 3), "frames_per_s": round(N / ms * 1e3, 1), "runs_ms": [round(t, 3) for t in v]}
    # the kernels' own times: one more call per mesh between events, averaged over --runs calls
    for name in meshes:
        for flags, key in ((capi.RENDER_CULL_BACK, name), (capi.RENDER_CULL_BACK | capi.RENDER_EDGES_INT64, name + "_int64")):
            h.enable_timing(True)
            for _ in range(a.runs):
                render(name, flags)
            calls, build, raster = h.render_times()
            h.enable_timing(False)
            res["legs"][key].update({"build_kernels_ms": round(build, 3), "raster_kernel_ms": round(raster, 3), "timed_calls": calls})
    print(json.dumps(res))
    h.close()


if __name__ == "__main__":
    main()
