"""The threshold stage restated in NumPy int64, for tests/test_gpu_thr_edges.py (pinned on the CPU by tests/test_thr_ref_cpu.py against the oracle).

adaptive / fixed: the thresholded bytes of cv::adaptiveThreshold(MEAN_C, BINARY_INV, block, C) and cv::threshold(BINARY_INV) on a stack of frames
[F][H][W], in integers only: the rounded mean is never formed, 255 where (g + floor(C)) * n <= S + n // 2 with S the block sum under replicated borders
(n is odd, so the mean's rounding has no ties and this is the oracle's `g - round(S / n) <= -floor(C)`).
tiles_of / bitmap_of: the contour image as the device keeps it (aruco_amd/csrc/bits_tiles.h, internal.h) from those bytes.
near_ties: how many pixels of an input sit within one grey level of the decision on either side: what makes an input able to see an off-by-one.
The generators at the end make the input families of the edge tests; every frame of a batch has a seed of its own."""
import math

import numpy as np


def _frames(frames):
    f = np.asarray(frames)
    assert f.dtype == np.uint8 and f.ndim in (2, 3)
    return f[None] if f.ndim == 2 else f


def block_sums(frames, block):
    """S [F][H][W] int64: sum of the block x block window around every pixel, borders replicated."""
    f = _frames(frames).astype(np.int64)
    r = block // 2
    assert block % 2 == 1 and block >= 3
    p = np.pad(f, ((0, 0), (r, r), (r, r)), mode="edge")
    c = np.cumsum(p, axis=1)
    c = np.concatenate([np.zeros_like(c[:, :1]), c], axis=1)
    v = c[:, block:] - c[:, :-block]                      # [F][H][W + 2r]
    c = np.cumsum(v, axis=2)
    c = np.concatenate([np.zeros_like(c[:, :, :1]), c], axis=2)
    return c[:, :, block:] - c[:, :, :-block]


def _margin(frames, block, C):
    """d = S + n // 2 - (g + floor(C)) * n: white (255) where d >= 0."""
    f = _frames(frames)
    n = block * block
    return block_sums(f, block) + n // 2 - (f.astype(np.int64) + int(math.floor(C))) * n


def adaptive(frames, block, C):
    d = _margin(frames, block, C)
    out = np.where(d >= 0, 255, 0).astype(np.uint8)
    return out[0] if np.asarray(frames).ndim == 2 else out


def fixed(frames, thr):
    f = np.asarray(frames)
    return np.where(f.astype(np.int64) <= int(math.floor(thr)), 255, 0).astype(np.uint8)


def near_ties(frames, block, C):
    """(pixels with 0 <= d < n, pixels with -n <= d < 0): one grey level more turns the first kind black, one less the second kind white."""
    d = _margin(frames, block, C)
    n = block * block
    return int(((d >= 0) & (d < n)).sum()), int(((d < 0) & (d >= -n)).sum())


def tiles_xy(W, H):
    return max(4, (W + 7) // 8 + 1), max(4, (H + 7) // 8 + 1)


def tiles_of(thr):
    """uint64 [..][tiles_y][tiles_x]: bit (y & 7) * 8 + (x & 7) of tile (y >> 3, x >> 3) = pixel (x, y) of the thresholded image with its first
    and last row and column cleared; pad tiles and the bits of rows >= H and columns >= W are zero."""
    t = np.asarray(thr)
    lead = t.shape[:-2]
    H, W = t.shape[-2:]
    tnx, tny = tiles_xy(W, H)
    b = np.zeros(lead + (tny * 8, tnx * 8), np.uint64)
    b[..., 1:H - 1, 1:W - 1] = (t[..., 1:H - 1, 1:W - 1] != 0)
    b = b.reshape(lead + (tny, 8, tnx, 8))
    w = (np.uint64(1) << (np.arange(8, dtype=np.uint64)[:, None, None] * np.uint64(8) + np.arange(8, dtype=np.uint64)[None, None, :]))   # [8][1][8]
    return (b * w).sum(axis=(-3, -1), dtype=np.uint64)


def bitmap_of(tiles, W):
    """uint64 [..][tiles_y][2 * ceil(W / 1024)]: per strip of 128 tiles the even word (bit i: tile 128 s + 2 i is not zero) and the odd word
    (tile 128 s + 2 i + 1); tiles at or beyond ceil(W / 8) have no bit."""
    t = np.asarray(tiles)
    ntx, ns = (W + 7) // 8, (W + 1023) // 1024
    full = np.zeros(t.shape[:-1] + (128 * ns,), bool)
    k = min(ntx, t.shape[-1])
    full[..., :k] = t[..., :k] != 0
    full = full.reshape(t.shape[:-1] + (ns, 64, 2))
    w = np.uint64(1) << np.arange(64, dtype=np.uint64)
    words = (full.astype(np.uint64) * w[:, None]).sum(axis=-2, dtype=np.uint64)   # [..][ns][2]
    return words.reshape(t.shape[:-1] + (2 * ns,))


def first_diff(a, b):
    """(x, y) of the first differing element of two equal-shaped 2-D arrays in raster order, None if they are equal."""
    ne = np.argwhere(np.asarray(a) != np.asarray(b))
    return None if len(ne) == 0 else (int(ne[0][1]), int(ne[0][0]))


# ---- input families

def blocky(H, W, seed, noise=20, cell=8):
    """cell x cell squares of random level plus +-noise per pixel (test_threshold_wide_kernel_strip_edges builds its frames this way)."""
    rng = np.random.RandomState(seed)
    base = rng.randint(0, 256, size=(H // cell + 2, W // cell + 2)).astype(np.float32)
    g = np.kron(base, np.ones((cell, cell), np.float32))[:H, :W] + rng.randint(-noise, noise + 1, size=(H, W))
    return np.clip(g, 0, 255).astype(np.uint8)


def contrast(H, W, seed, negative=False):
    """Dark pixels (0..60) on a bright ground (200..255), their density ramped along the diagonal from 0.5 % to 60 %: g - mean sweeps the whole range down to -250 in steps below one grey level. negative:
    255 - g, the same sweep upwards."""
    rng = np.random.RandomState(seed)
    ramp = 0.005 + 0.6 * np.linspace(0.0, 1.0, W + H) ** 2          # half of the frame below 15 %: |g - mean| around 200 needs lone pixels
    p = ramp[np.arange(H)[:, None] + np.arange(W)[None, :]]
    dark = rng.random_sample((H, W)) < p
    g = np.where(dark, rng.randint(0, 61, size=(H, W)), rng.randint(200, 256, size=(H, W))).astype(np.uint8)
    return (255 - g).astype(np.uint8) if negative else g


def const(H, W, v):
    return np.full((H, W), v, np.uint8)


def checker(H, W):
    """the hard checkerboard of test_threshold_wide_kernel_strip_edges: 5 x 3 pixel fields of 0 and 255"""
    return (((np.arange(H)[:, None] // 3 + np.arange(W)[None, :] // 5) % 2) * 255).astype(np.uint8)


def lines(H, W, seed, kind):
    """A blocky interior inside four border lines of 0 (kind 0), 255 (kind 1) or alternating 0 / 255 (kind 2)."""
    g = blocky(H, W, seed)
    if kind < 2:
        v = 0 if kind == 0 else 255
        g[0, :] = v; g[-1, :] = v; g[:, 0] = v; g[:, -1] = v
    else:
        g[0, :] = (np.arange(W) % 2) * 255; g[-1, :] = ((np.arange(W) + 1) % 2) * 255
        g[:, 0] = (np.arange(H) % 2) * 255; g[:, -1] = ((np.arange(H) + 1) % 2) * 255
    return g


FAMILIES = {
    "blocky": lambda H, W, s, f: blocky(H, W, s),
    "tame": lambda H, W, s, f: blocky(H, W, s, noise=3, cell=16),       # noise below C = 7: few, long contours
    "lines": lambda H, W, s, f: blocky(H, W, s) if f % 4 == 0 else lines(H, W, s, f % 4 - 1),
    "mix": lambda H, W, s, f: (contrast(H, W, s), contrast(H, W, s, True), const(H, W, 0), const(H, W, 255), checker(H, W))[f % 5],
    "levels": lambda H, W, s, f: np.random.RandomState(s).randint(0, 256, size=(H, W)).astype(np.uint8),   # FIXED: every grey level
}


def frame_of(family, f, H, W, seed):
    """frame f of a batch: made from seed * 4099 + f, so that no two frames of a case are alike"""
    return FAMILIES[family](H, W, seed * 4099 + f, f)


def batch(family, nframes, H, W, seed):
    return np.stack([frame_of(family, f, H, W, seed) for f in range(nframes)])


# ---- the cases of the edge tests (tests/test_gpu_thr_edges.py runs them on the device, tests/test_thr_ref_cpu.py holds their inputs to the
# coverage condition and this file's functions to the oracle on them)

def seg_rule(W, H, nframes):
    """rows per wave of the 16-pixel-per-lane kernels (thr_plan.h), restated"""
    waves128 = ((W + 1023) // 1024) * ((H + 127) // 128) * nframes
    return 128 if waves128 >= 512 else 32 if waves128 >= 128 else 16


def frames_for_seg(W, H, seg):
    """the fewest frames of W x H that reach a segment height (16 rows: six, so that the smallest frames together hold enough near ties)"""
    per = ((W + 1023) // 1024) * ((H + 127) // 128)
    return {16: 6, 32: -(-128 // per), 128: -(-512 // per)}[seg]


SEG_HEIGHTS = {seg: [(H, None) for H in (seg - 1, seg, seg + 1, seg + 7, seg + 8, seg + 9, 2 * seg + 1)] for seg in (16, 32, 128)}
SEG_HEIGHTS[16].append((129, 63))                      # the rule's edges at H = 129: waves128 = 2 * frames
SEG_HEIGHTS[32] += [(129, 64), (129, 255)]
SEG_HEIGHTS[128].append((129, 256))
SEG_W = 48

STRIP_GEOMS = [(1040, 40, 5, 16), (1040, 72, 65, 32), (2064, 136, 86, 128)]       # W, H, frames, seg
WIDTHS = [16, 32, 1008, 1024, 1040, 2048, 2064]
WIDTH_H = 41
BLOCK_WIDTHS = [272, 268, 267]                          # 16-byte rows, dword rows, byte-wise rows
BLOCK_H = 140
BLOCK_CS = [7.0, -3.5, 0.0, 0.999]
BOUNDARY_CASES = ([(9, s * 148.0) for s in (1, -1)] + [(9, s * 149.0) for s in (1, -1)] + [(11, s * 14.0) for s in (1, -1)] +
                  [(11, s * 15.0) for s in (1, -1)] + [(7, s * 200.0) for s in (1, -1)] + [(7, s * 201.0) for s in (1, -1)] + [(7, -200.5)] +
                  [(7, s * 412.0) for s in (1, -1)] + [(7, s * 413.0) for s in (1, -1)] + [(5, s * 300.0) for s in (1, -1)] +
                  [(3, s * 1000.0) for s in (1, -1)] + [(7, s * 1000.0) for s in (1, -1)])
FIXED_THRS = [-1.0, 0.0, 99.5, 254.0, 255.0, 300.0]
RANGE_CASES = [(7, 1, [7, 7, 9]), (7, 2, [5, 7, 9, 11, 13]), (9, 2, [7, 9, 11, 13, 15])]    # thres_param1, range, the planes' blocks
RANGE_GEOMS = [(272, 140), (1040, 137)]
STRIDE_CASE = (272, BLOCK_H, 3, 800)                                    # W, H, frames, seed
# one handle across geometries, six frames each, seed SHARED_SEED + step; the last step is lower than 17 rows: tiles_y()'s floor of 4 gives it
# a third tile row that no threshold kernel writes and the start-candidate kernel reads
SHARED_STEPS = [(2064, 136), (1024, 64), (48, 129), (2064, 136), (48, 16)]
SHARED_FRAMES, SHARED_SEED = 6, 900
TIMING_CASE = (SEG_W, 137, 256, 1000, (7, 5))                           # W, H, frames, seed + block, blocks
PRODUCTION_GEOMS = [(48, 129, 256, 128), (1040, 72, 65, 32)]            # W, H, frames, seg; seed PRODUCTION_SEED + W
PRODUCTION_SEED = 1100
HOOKS_CASE = (272, BLOCK_H, 3, 1200, [7, 7, 9])                         # W, H, frames, seed, the planes' blocks


def adaptive_cases():
    """(name, family, frames, H, W, seed, block, C) of every adaptive input batch the edge tests use"""
    out = []
    for seg in (16, 32, 128):
        for H, nf in SEG_HEIGHTS[seg]:
            nf = nf or frames_for_seg(SEG_W, H, seg)
            for block in (7, 3, 5, 9):
                out.append(("seg%d-H%d-F%d-b%d" % (seg, H, nf, block), "blocky", nf, H, SEG_W, 100 + seg + H, block, 7.0))
    for W, H, nf, seg in STRIP_GEOMS:
        for block in (7, 5):
            out.append(("strips-%dx%dx%d-b%d" % (W, H, nf, block), "blocky", nf, H, W, 200 + seg, block, 7.0))
    for W in WIDTHS:
        for seg in (128, 16):
            nf = 3 if seg == 16 else frames_for_seg(W, WIDTH_H, 128)
            for block in (7, 3):
                out.append(("width%d-seg%d-b%d" % (W, seg, block), "lines", nf, WIDTH_H, W, 300 + W, block, 7.0))
    for W in BLOCK_WIDTHS:
        for block in range(3, 32, 2):
            for c in BLOCK_CS:
                out.append(("block%d-C%g-W%d" % (block, c, W), "blocky", 3, BLOCK_H, W, 400 + W, block, c))
        for block, c in BOUNDARY_CASES:
            out.append(("bound%d-C%g-W%d" % (block, c, W), "mix", 5, BLOCK_H, W, 500 + W, block, c))
    for p1, r, blocks in RANGE_CASES:
        for W, H in RANGE_GEOMS:
            for t, block in enumerate(blocks):
                out.append(("range-p%d-r%d-%dx%d-t%d" % (p1, r, W, H, t), "blocky", 3, H, W, 600 + W, block, 7.0))
    W, H, nf, seed = STRIDE_CASE
    out.append(("strides-%dx%dx%d" % (W, H, nf), "blocky", nf, H, W, seed, 7, 7.0))
    for i, (W, H) in enumerate(SHARED_STEPS):
        out.append(("shared-step%d-%dx%d" % (i, W, H), "blocky", SHARED_FRAMES, H, W, SHARED_SEED + i, 7, 7.0))
    W, H, nf, seed, blocks = TIMING_CASE
    for block in blocks:
        out.append(("timing-%dx%dx%d-b%d" % (W, H, nf, block), "blocky", nf, H, W, seed + block, block, 7.0))
    for W, H, nf, seg in PRODUCTION_GEOMS:
        out.append(("production-%dx%dx%d" % (W, H, nf), "tame", nf, H, W, PRODUCTION_SEED + W, 7, 7.0))
    W, H, nf, seed, blocks = HOOKS_CASE
    for block in sorted(set(blocks)):
        out.append(("hooks-%dx%dx%d-b%d" % (W, H, nf, block), "tame", nf, H, W, seed, block, 7.0))
    return out
