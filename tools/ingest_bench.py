#!/usr/bin/env python3
"""What camera-native input costs and buys ("Camera-native input"). One process, N frames of 1920 x 1080 of synth.make_stream
encoded into every format, the default detector, warmed, alternating, event-timed legs (the median of --runs per leg), as tools/ab_variants.sh
alternates settings on one box.

--mode device (default): frames resident in HBM. Per format arucohip_convert_batch to device grey + arucohip_detect_batch on the result,
  beside arucohip_detect_batch_bgr on BGR frames of the same content and arucohip_detect_batch on the grey frames; GRAY8 and the Y plane
  of NV12 also in place (no conversion). ratio_to_bgr above 1 = faster than the BGR path.
--mode host: frames in pinned host memory, results left on the device. Bayer, NV12 and YUYV (raw bytes up, converted on the device) beside
  BGR frames through arucohip_detect_batch_bgr; the expectation is a ratio near the byte ratio (3, 3 and 1.5).
--mode kernel: arucohip_convert_batch alone, device to device, grey and B,G,R, with the achieved bytes per second (bytes in + bytes out,
  counted from shapes). The leg also runs arucohip_detect_batch_bgr --runs times, so that under
  `rocprofv3 --kernel-trace --stats -- python tools/ingest_bench.py --mode kernel` bgr2gray_kernel's own time stands beside ingest_kernel's.
--mode export: the way out, arucohip_export_batch alone, device to device: grey and B,G,R frames to every destination format, with the
  achieved bytes per second (bytes in + bytes out, counted from shapes). Beside them bgr2gray_kernel's from the same run: the batch time of
  arucohip_detect_batch_bgr minus that of arucohip_detect_batch on the grey frames it computes (the B,G,R frames carry the grey value in
  all three channels, so the detection work is the same), over its 4 bytes per pixel; a `rocprofv3 --kernel-trace --stats` run of this
  mode shows the kernel's own time beside egress_kernel's. With few frames the difference is within the noise of the two detection legs.
The BGR legs run the library this process loaded: ARUCOHIP_LIB=<a build of the parent commit> gives the parent's numbers for them.
Prints one JSON line with arucohip_build_info()."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from aruco_amd import capi, synth

W, H, CAP = 1920, 1080, 64
IN_BYTES = {"GRAY8": 1, "BGR8": 3, "RGB8": 3, "BGRA8": 4, "RGBA8": 4, "GRAY16": 2, "YUYV": 2, "UYVY": 2, "NV12": 1.5,
            "BAYER_RGGB": 1, "BAYER_BGGR": 1, "BAYER_GRBG": 1, "BAYER_GBRG": 1}   # per pixel


def encode(name, g):
    """grey frames [N][H][W] (uint8 tensor) -> raw frames [N][rows][row bytes] of format `name` that carry them: all three channels, Y with
    neutral chroma, the top byte of 16 bits, or the mosaic of the grey image itself"""
    n, h, w = g.shape
    if name == "GRAY8" or name.startswith("BAYER_"):
        return g.clone()
    if name in ("BGR8", "RGB8"):
        return g[..., None].expand(n, h, w, 3).reshape(n, h, 3 * w).contiguous()
    if name in ("BGRA8", "RGBA8"):
        return g[..., None].expand(n, h, w, 4).reshape(n, h, 4 * w).contiguous()
    if name == "GRAY16":   # little-endian, bits = 16: low byte 0, high byte the grey value
        return torch.stack([torch.zeros_like(g), g], dim=-1).reshape(n, h, 2 * w).contiguous()
    if name in ("YUYV", "UYVY"):
        c = torch.full_like(g, 128)
        return torch.stack([g, c] if name == "YUYV" else [c, g], dim=-1).reshape(n, h, 2 * w).contiguous()
    assert name == "NV12"
    return torch.cat([g, torch.full((n, h // 2, w), 128, dtype=torch.uint8, device=g.device)], dim=1).contiguous()


def fmt_of(name):
    return capi.frame_format(name, bits=16 if name == "GRAY16" else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["device", "host", "kernel", "export"], default="device")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ingest_bench.py needs a GPU"
    N = a.frames
    grey, _ = synth.make_stream(N, seed=4711, device="cuda")
    h = capi.Handle(W, H, max_batch=N)
    stream = torch.cuda.ExternalStream(h.get_stream())
    d_gray = torch.zeros((N, H, W), dtype=torch.uint8, device="cuda")
    d_bgr = torch.zeros((N, H, W, 3), dtype=torch.uint8, device="cuda")
    out = torch.zeros((N, CAP * capi.MARKER_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(N, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def detect_grey(ptr, rs=W, fs=W * H, on_device=True):
        h._chk(h.L.arucohip_detect_batch(h.h, C.c_void_p(ptr), N, W, H, rs, fs, int(on_device), None, None, 0, -1.0, 0, C.c_void_p(out.data_ptr()), CAP,
                                         C.c_void_p(cnt.data_ptr()), 1))

    def detect_bgr(ptr, on_device=True):
        h._chk(h.L.arucohip_detect_batch_bgr(h.h, C.c_void_p(ptr), N, W, H, 3 * W, 3 * W * H, int(on_device), None, None, 0, -1.0, 0,
                                             C.c_void_p(out.data_ptr()), CAP, C.c_void_p(cnt.data_ptr()), 1))

    def convert(name, src, channels, on_device=True):
        rows, rb = src.shape[1], src.shape[2]
        h.convert_device(src.data_ptr(), fmt_of(name), N, W, H, rb, rows * rb, channels, (d_gray if channels == 1 else d_bgr).data_ptr(),
                         src_on_device=on_device)

    def run_legs(legs):
        times = {k: [] for k in legs}
        for i in range(a.warmup + a.runs):
            for k, fn in legs.items():   # alternating: every leg sees the same drift of the machine
                ms = timed(fn)
                if i >= a.warmup:
                    times[k].append(ms)
        h.batch_status()
        return {k: float(np.median(v)) for k, v in times.items()}, times

    res = {"mode": a.mode, "frames": N, "width": W, "height": H, "runs": a.runs, "build_info": capi.build_info(),
           "device": torch.cuda.get_device_name(0)}
    names = capi.PIX_NAMES
    if a.mode == "device":
        raw = {n: encode(n, grey) for n in names}
        torch.cuda.synchronize()
        legs = {"bgr_path": lambda: detect_bgr(raw["BGR8"].data_ptr()), "grey_path": lambda: detect_grey(grey.data_ptr()),
                "NV12_in_place": lambda: detect_grey(raw["NV12"].data_ptr(), W, W * H * 3 // 2),
                "GRAY8_in_place": lambda: detect_grey(raw["GRAY8"].data_ptr())}
        for n in names:
            legs[n] = (lambda n=n: (convert(n, raw[n], 1), detect_grey(d_gray.data_ptr())))
        med, runs = run_legs(legs)
        res["legs"] = {k: {"ms_per_batch": round(ms, 3), "frames_per_s": round(N / ms * 1e3, 1), "ratio_to_bgr": round(med["bgr_path"] / ms, 3),
                           "ratio_to_grey": round(med["grey_path"] / ms, 3), "runs_ms": [round(t, 3) for t in runs[k]]} for k, ms in med.items()}
    elif a.mode == "host":
        use = ("BGR8", "BAYER_RGGB", "NV12", "YUYV")
        raw = {n: encode(n, grey).cpu().pin_memory() for n in use}
        torch.cuda.synchronize()
        legs = {"bgr_path": lambda: detect_bgr(raw["BGR8"].data_ptr(), on_device=False)}
        for n in use[1:]:
            legs[n] = (lambda n=n: (convert(n, raw[n], 1, on_device=False), detect_grey(d_gray.data_ptr())))
        med, runs = run_legs(legs)
        res["legs"] = {k: {"ms_per_batch": round(ms, 3), "frames_per_s": round(N / ms * 1e3, 1), "ratio_to_bgr": round(med["bgr_path"] / ms, 3),
                           "byte_ratio": 1.0 if k == "bgr_path" else round(3 / IN_BYTES[k], 3), "runs_ms": [round(t, 3) for t in runs[k]]}
                       for k, ms in med.items()}
    elif a.mode == "export":
        dests = ("GRAY8", "BGR8", "RGB8", "BGRA8", "RGBA8", "YUYV", "UYVY", "NV12")
        src = {1: grey, 3: encode("BGR8", grey)}
        d_out = torch.zeros(N * H * W * 4, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def export(name, c):
            h.export_batch_ptr(src[c].data_ptr(), c, N, W, H, fmt_of(name), d_out.data_ptr())

        legs = {"bgr_path_detect": lambda: detect_bgr(src[3].data_ptr()), "grey_path_detect": lambda: detect_grey(grey.data_ptr())}
        for n in dests:
            for c in (1, 3):
                legs["%d_to_%s" % (c, n)] = (lambda n=n, c=c: export(n, c))
        med, runs = run_legs(legs)
        res["legs"] = {}
        for k, ms in med.items():
            if k.endswith("_detect"):
                continue
            c, n = k.split("_to_", 1)
            nbytes = int(N * W * H * (int(c) + IN_BYTES[n]))
            res["legs"][k] = {"ms": round(ms, 4), "bytes_in_plus_out": nbytes, "tb_per_s": round(nbytes / ms / 1e9, 3),
                              "runs_ms": [round(t, 4) for t in runs[k]]}
        ms = med["bgr_path_detect"] - med["grey_path_detect"]
        res["bgr2gray_kernel_by_difference"] = {"ms": round(ms, 4), "bytes_in_plus_out": N * W * H * 4,
                                                "tb_per_s": round(N * W * H * 4 / ms / 1e9, 3) if ms > 0 else None}
    else:
        raw = {n: encode(n, grey) for n in names}
        torch.cuda.synchronize()
        legs = {"bgr_path_detect": lambda: detect_bgr(raw["BGR8"].data_ptr())}   # puts bgr2gray_kernel into a kernel trace of this run
        for n in names:
            for c in (1, 3):
                legs["%s_to_%d" % (n, c)] = (lambda n=n, c=c: convert(n, raw[n], c))
        med, runs = run_legs(legs)
        res["legs"] = {}
        for k, ms in med.items():
            if k == "bgr_path_detect":
                continue
            n, c = k.rsplit("_to_", 1)
            nbytes = int(N * W * H * ((1 if (n == "NV12" and c == "1") else IN_BYTES[n]) + int(c)))
            res["legs"][k] = {"ms": round(ms, 4), "bytes_in_plus_out": nbytes, "tb_per_s": round(nbytes / ms / 1e9, 3),
                              "runs_ms": [round(t, 4) for t in runs[k]]}
    print(json.dumps(res))
    h.close()


if __name__ == "__main__":
    main()
