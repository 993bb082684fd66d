"""What plane rectification costs on the device: a 1920x1080 -> 1920x1080 window over 1024 device-resident one-channel frames with 1024
different maps (arucohip_board_rectify_batch, ndist 0 and 5), beside two yardsticks on the same frames in the same process:
arucohip_undistort's remap (one cached map, fixed-point positions read from memory) and a plain device-to-device copy. Every leg is
warmed up, then timed over --calls calls between two events on the handle's stream. Prints one JSON line per leg: ms per call over the
whole batch, the bytes the algorithm needs (every source byte read once, every destination byte written once, the map bytes) and the
GB/s those bytes give. Measured, not gated: DESIGN.md "Plane rectification" records a run.

    python tools/rectify_rate.py [--frames 1024] [--calls 20] [--limit 240]
"""
import argparse
import json
import os
import signal
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--limit", type=int, default=240, help="seconds after which the run gives up")
    args = ap.parse_args()

    def give_up(*_):
        raise SystemExit("rectify_rate: no result within %d s" % args.limit)

    signal.signal(signal.SIGALRM, give_up)
    signal.alarm(args.limit)

    import torch

    from aruco_amd import capi

    assert torch.cuda.is_available(), "rectify_rate needs a GPU"
    n, W, H = args.frames, args.width, args.height
    chunk = 64                                    # arucohip_undistort takes at most max_batch frames per call
    h = capi.Handle(W, H, max_batch=chunk)
    stream = torch.cuda.Stream()                  # the handle's work, the copy and the events share one stream
    h.set_stream(stream.cuda_stream)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4711)
    frames = torch.randint(0, 256, (n, H, W), dtype=torch.uint8, device="cuda", generator=gen)
    dst = torch.empty_like(frames)
    K = np.array([[1400, 0, W / 2], [0, 1400, H / 2], [0, 0, 1]], np.float32)
    dist5 = np.array([0.08, -0.12, 0.0011, -0.0017, 0.03], np.float32)
    # a board about 0.7 m away, turned a little differently in every frame; the window: the frame's own size at a scale that keeps the
    # source footprint about the frame (1 output pixel = 0.5 mm = one source pixel at that distance)
    rng = np.random.RandomState(7)
    boards = np.zeros(n, capi.BOARD_DTYPE)
    for f in range(n):
        boards[f] = (4, 1, rng.uniform(-0.3, 0.3, 3), (rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), rng.uniform(0.65, 0.75)))
    dboards = torch.from_numpy(boards.view(np.uint8).copy()).cuda()
    win = capi.Rectify(W, H, -W / 2 * 0.0005, -H / 2 * 0.0005, 0.0005, 0.0, 0.0, 0.0005)

    def rectify(dist):
        h.board_rectify_device(frames.data_ptr(), n, W, H, 1, dboards, K, win, dst.data_ptr(), dist)

    def undistort():
        for f0 in range(0, n, chunk):
            m = min(chunk, n - f0)
            h._chk(h.L.arucohip_undistort(h.h, frames.data_ptr() + f0 * W * H, m, W, H, W, W * H, 1, 1, K.ctypes.data, dist5.ctypes.data, 5,
                                          dst.data_ptr() + f0 * W * H, 1))

    def copy():
        dst.copy_(frames)

    image = n * W * H
    legs = [("rectify_ndist0", lambda: rectify(None), 2 * image + n * 76), ("rectify_ndist5", lambda: rectify(dist5), 2 * image + n * 76),
            ("undistort_remap", undistort, 2 * image + W * H * 6), ("copy_d2d", copy, 2 * image)]
    torch.cuda.synchronize()
    for name, fn, nbytes in legs:
        with torch.cuda.stream(stream):
            fn(), fn()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            for _ in range(args.calls):
                fn()
            t1.record(stream)
            t1.synchronize()
        ms = t0.elapsed_time(t1) / args.calls
        print(json.dumps({"leg": name, "frames": n, "size": [W, H], "calls": args.calls, "ms_per_call": round(ms, 3), "bytes": nbytes,
                          "GBps": round(nbytes / ms / 1e6, 1), "covered": float((dst[::max(n // 8, 1)] != 0).float().mean()) if name.startswith("rectify") else None}),
              flush=True)
    signal.alarm(0)
    h.close()


if __name__ == "__main__":
    main()
