"""What plane compositing costs on the device: 1024 device-resident 1920x1080 one-channel frames with 1024 poses and one 1024x1024
texture that covers roughly a quarter of each frame (arucohip_board_composite_batch; opacity 255 and 128, ndist 0 and 5, with and without
masks), beside two yardsticks on the same frames in the same process: arucohip_board_rectify_batch (a 1920x1080 window, ndist 5) and a
plain device-to-device copy. Every leg is warmed up, then timed over --calls calls between two events on the handle's stream. Prints one
JSON line per leg: ms per call over the whole batch, the share of the frames' pixels that was painted, the bytes the algorithm needs
(every painted byte written once and, below opacity 255, read once; every mask byte read once; the texture and the maps once) and the
GB/s those bytes give. Measured, not gated: DESIGN.md "Plane compositing" records a run.

    python tools/composite_rate.py [--frames 1024] [--calls 20] [--limit 240]
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
    ap.add_argument("--texture", type=int, default=1024, help="side of the square texture")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--limit", type=int, default=240, help="seconds after which the run gives up")
    args = ap.parse_args()

    def give_up(*_):
        raise SystemExit("composite_rate: no result within %d s" % args.limit)

    signal.signal(signal.SIGALRM, give_up)
    signal.alarm(args.limit)

    import torch

    from aruco_amd import capi

    assert torch.cuda.is_available(), "composite_rate needs a GPU"
    n, W, H, T = args.frames, args.width, args.height, args.texture
    h = capi.Handle(W, H, max_batch=1)
    stream = torch.cuda.Stream()                  # the handle's work, the copy and the events share one stream
    h.set_stream(stream.cuda_stream)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4711)
    pristine = torch.randint(0, 256, (n, H, W), dtype=torch.uint8, device="cuda", generator=gen)
    frames = pristine.clone()
    dst = torch.empty_like(frames)
    tex = torch.randint(0, 256, (T, T), dtype=torch.uint8, device="cuda", generator=gen)
    masks = torch.ones((n, H, W), dtype=torch.uint8, device="cuda")
    masks[:, H // 3:H // 2, W // 3:W // 2] = 0     # an occluder over a part of the board
    K = np.array([[1400, 0, W / 2], [0, 1400, H / 2], [0, 0, 1]], np.float32)
    dist5 = np.array([0.08, -0.12, 0.0011, -0.0017, 0.03], np.float32)
    # a board about 0.7 m away, turned a little differently in every frame (tools/rectify_rate.py's poses). A frame pixel is 0.5 mm there;
    # the texture spans 0.36 m, about 720 x 720 frame pixels: a quarter of the frame
    rng = np.random.RandomState(7)
    boards = np.zeros(n, capi.BOARD_DTYPE)
    for f in range(n):
        boards[f] = (4, 1, rng.uniform(-0.3, 0.3, 3), (rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), rng.uniform(0.65, 0.75)))
    dboards = torch.from_numpy(boards.view(np.uint8).copy()).cuda()
    step = 0.36 / T
    win = capi.Rectify(T, T, -T / 2 * step, -T / 2 * step, step, 0.0, 0.0, step)
    view = capi.Rectify(W, H, -W / 2 * 0.0005, -H / 2 * 0.0005, 0.0005, 0.0, 0.0, 0.0005)

    def composite(opacity, dist, masked):
        h.board_composite_device(frames.data_ptr(), n, W, H, 1, dboards, K, win, capi.texture(tex, opacity), dist, masks.data_ptr() if masked else None)

    def rectify():
        h.board_rectify_device(frames.data_ptr(), n, W, H, 1, dboards, K, view, dst.data_ptr(), dist5)

    def copy():
        dst.copy_(frames)

    image = n * W * H
    legs = [("composite_op%d_ndist%d%s" % (op, 0 if d is None else 5, "_masks" if m else ""), (op, d, m)) for op in (255, 128) for d in (None, dist5)
            for m in (False, True)]
    legs += [("rectify_ndist5", None), ("copy_d2d", None)]
    sample = slice(None, None, max(n // 8, 1))
    torch.cuda.synchronize()
    for name, cfg in legs:
        fn = (lambda: composite(*cfg)) if cfg else (rectify if name.startswith("rectify") else copy)
        with torch.cuda.stream(stream):
            frames.copy_(pristine)
            fn()
            torch.cuda.synchronize()
            painted = float((frames[sample] != pristine[sample]).float().mean()) if cfg else None
            fn()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            for _ in range(args.calls):
                fn()
            t1.record(stream)
            t1.synchronize()
        ms = t0.elapsed_time(t1) / args.calls
        if cfg:
            # a random texture on random frames leaves one painted byte in 256 unchanged (fewer at opacity 128): close enough for the byte count
            nbytes = int(painted * image * (1 if cfg[0] == 255 else 2)) + (image if cfg[2] else 0) + T * T + n * 76
        else:
            nbytes = 2 * image + (n * 76 if name.startswith("rectify") else 0)
        print(json.dumps({"leg": name, "frames": n, "size": [W, H], "texture": [T, T], "calls": args.calls, "ms_per_call": round(ms, 3), "painted": painted,
                          "bytes": nbytes, "GBps": round(nbytes / ms / 1e6, 1)}), flush=True)
    signal.alarm(0)
    h.close()


if __name__ == "__main__":
    main()
