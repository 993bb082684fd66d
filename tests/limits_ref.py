"""Frames whose demand on each fixed-capacity device list is known from a reference, and that reference.

The detector keeps start candidates, waypoints, long-walk rings, border descriptors, border points, quads, candidates and the flat decode list in
lists of fixed capacity (include/arucohip.h lists the capacities). The frames here load one list each with a demand that the oracle or a numpy
reference gives - never the code under test - so that a test can set the capacity to exactly the demand, or one below it.

  squares(nx, ny, side, pitch, margin)   black squares on white: per threshold plane one kept border and one quad a square, one candidate a square
  checker(h, w)                          one-pixel checkerboard: with a fixed threshold every clear pixel of the interior is a hole start
  dominoes(h, w)                         two-pixel vertical bars: with a fixed threshold every bar is an outer start
  mixed()                                one large square, whose two borders are followed by the late generations, and a block of small ones
  marked(seed, h, w)                     two or three real markers: the neighbour whose bytes must not change
"""
import numpy as np

from aruco_amd import synth

CK = 16                # steps between two checkpoints of a walk: a kept border of n points takes ceil(n / CK) pool words in front of its points
LATE_POINTS = 960      # borders above this many points are kept by the late walker generations (the top of the descriptor array)
MIN_SIZE, MAX_SIZE = 0.04, 0.5


def squares(nx, ny, side, pitch, margin):
    g = np.full((2 * margin + ny * pitch, 2 * margin + nx * pitch), 255, np.uint8)
    o = margin + (pitch - side) // 2
    for j in range(ny):
        for i in range(nx):
            g[o + j * pitch:o + j * pitch + side, o + i * pitch:o + i * pitch + side] = 0
    return g


def checker(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.where((x + y) & 1, 255, 0).astype(np.uint8)


def dominoes(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.where(((x & 1) == 0) & ((y & 3) < 2), 0, 255).astype(np.uint8)


MIXED_W, MIXED_H, MIXED_BIG, MIXED_SMALL = 640, 480, 262, 28


def mixed():
    g = np.full((MIXED_H, MIXED_W), 255, np.uint8)
    g[20:20 + MIXED_BIG, 20:20 + MIXED_BIG] = 0
    for j in range(10):
        for i in range(7):
            x0, y0 = 310 + i * 44, 20 + j * 44
            g[y0:y0 + MIXED_SMALL, x0:x0 + MIXED_SMALL] = 0
    return g


def marked(seed, h, w):
    """two or three upright markers of 5 or 6 pixels a cell (7 or 8 in a frame of 256 pixels or more), black on white, at places the seed chooses"""
    rng = np.random.RandomState(seed)
    g = np.full((h, w), 255, np.uint8)
    n = 2 + int(rng.randint(2)) if w >= 3 * 56 else 2
    slot = w // n
    for i in range(n):
        cell = (5 if max(h, w) < 256 else 7) + int(rng.randint(2))
        side = 7 * cell
        mx, my = 4 + w // 32, 4 + h // 32                      # clear of the frame's edge, where the detector drops markers (border distance)
        x0 = i * slot + mx + int(rng.randint(max(slot - side - 2 * mx, 1)))
        y0 = my + int(rng.randint(max(h - side - 2 * my, 1)))
        bits = synth.marker_bits(int(rng.randint(1024)))
        g[y0:y0 + side, x0:x0 + side] = np.kron(bits, np.ones((cell, cell), np.uint8)) * 255
    return g


def size_filter(width, height):
    """(lo, hi): a border of n points is kept when lo < n < hi (default min / max size, float arithmetic as the detector's)"""
    m = max(width, height)
    return int(np.float32(MIN_SIZE) * np.float32(m) * np.float32(4)), min(int(np.float32(MAX_SIZE) * np.float32(m) * np.float32(4)), 16383)


def kept_borders(thresholded):
    """the borders of one thresholded plane that pass the size filter, in the reference's order: [{"hole", "pts"}]"""
    from oracle import orc

    h, w = thresholded.shape
    lo, hi = size_filter(w, h)
    return [c for c in orc.find_contours(thresholded) if lo < len(c["pts"]) < hi]


def plane_of(gray, fixed=None, p1=7, p2=7.0):
    """the thresholded plane the detector works on: adaptive (block p1, offset p2) or, with fixed = level, the fixed threshold"""
    from oracle import orc

    if fixed is None:
        return orc.adaptive_threshold(gray, int(p1), float(p2))
    return np.where(gray > fixed, 0, 255).astype(np.uint8)   # THRESH_BINARY_INV


def pool_bounds(borders):
    """(least, most) pool words of the kept borders: the points, and at most one checkpoint word per CK points in front of them"""
    n = [len(c["pts"]) for c in borders]
    return sum(n), sum(k + (k + CK - 1) // CK for k in n)


def quad_demand(borders):
    """quads of the kept borders of one plane before the near-duplicate removal (quad_ref.border_quad)"""
    from tests import quad_ref

    return sum(quad_ref.border_quad([tuple(p) for p in c["pts"].tolist()]) is not None for c in borders)


def oracle_candidates(gray, **params):
    from oracle import orc

    o = orc.Oracle(**params)
    o.detect(gray)
    return o.candidates()
