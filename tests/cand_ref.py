"""Numpy restatement of the border-start candidates (candidates_sparse_kernel, walker mode) and the hand-made frames that reach its paths.

Input is the binary image cv::findContours sees (set = non-zero, the 1-px frame cleared: binary_of()). The rules, pixel by pixel:
  start rule   outer: pixel set, W / NW / N / NE clear.  hole: pixel clear, W and N set, x <= W-2, y <= H-2.
  drop_single  an outer start with no set neighbour at all is a 1-point border; it is dropped unless it lies in row 7 of its 8x8 tile (whose lower
               neighbours are in another tile row).
  run rule     with `avail` pixels of the row at hand from x on: outer - L = run of set pixels from x (at most avail), no set pixel in the row above at
               columns x+2 .. x+min(L, avail-1); hole - L = run of clear pixels from x, every pixel of the row above at columns x+1 .. x+min(L-1, avail-1)
               set. First with the 16 pixels of the tile and its right neighbour (avail = 16 - (x & 7)); a run that leaves them (L == avail) is decided at
               once on 8 * min(8, tnx - tx) - (x & 7) pixels (at most 64, never past the pad tile column). A longer run keeps the candidate.
The rule is necessary, never sufficient: every border start of the sequential scan is in the set, most of the set is no border start.
"""
import numpy as np


def binary_of(thresholded):
    """The image the contour stage sees: non-zero = set, the 1-pixel frame cleared."""
    b = np.asarray(thresholded) != 0
    b = b.copy()
    b[0, :] = b[-1, :] = False
    b[:, 0] = b[:, -1] = False
    return b


def _tiles(n):
    return max((n + 7) // 8 + 1, 4)


def _rule(mid, up, kind):
    """(passes, run length) on the `avail = len(mid)` pixels at hand."""
    avail = len(mid)
    stop = np.flatnonzero(mid if kind else ~mid)
    run = int(stop[0]) if len(stop) else avail
    if kind:
        hi = min(run - 1, avail - 1)
        return bool(up[1:hi + 1].all()), run
    hi = min(run, avail - 1)
    return not bool(up[2:hi + 1].any()), run


def start_candidates(binimg, drop_single=True):
    """{"outer", "hole": sorted uint32 arrays of y << 16 | x (hole: the clear pixel), "n_start": start-rule pixels (after drop_single),
    "n64": candidates the 64-pixel test decided, "n_long": of them runs longer than its horizon, "n_empty_tile": start-rule pixels in a tile without
    a set pixel, "kept_empty_tile": of them survivors}"""
    b = np.asarray(binimg) != 0
    H, W = b.shape
    tnx, tny = _tiles(W), _tiles(H)
    Hp, Wp = 8 * tny, 8 * tnx
    full = np.zeros((Hp + 2, Wp + 2), bool)      # full[y + 1, x + 1] = pixel (x, y); everything outside the image is clear
    full[1:H + 1, 1:W + 1] = b
    c = full[1:-1, 1:-1]
    Wn, E = full[1:-1, :-2], full[1:-1, 2:]
    N, NW, NE = full[:-2, 1:-1], full[:-2, :-2], full[:-2, 2:]
    S, SW, SE = full[2:, 1:-1], full[2:, :-2], full[2:, 2:]
    ys, xs = np.mgrid[0:Hp, 0:Wp]
    outer = c & ~(Wn | NW | N | NE)
    hole = ~c & Wn & N & (xs <= W - 2) & (ys <= H - 2)
    if drop_single:
        outer &= ~(~(E | S | SW | SE) & ((ys & 7) != 7))
    tile_set = c.reshape(tny, 8, tnx, 8).any(axis=(1, 3))
    res = {0: [], 1: []}
    n64 = n_long = n_empty = kept_empty = 0
    cy, cx = np.nonzero(outer | hole)
    for y, x in zip(cy.tolist(), cx.tolist()):
        kind = 1 if hole[y, x] else 0
        tx, j = x >> 3, x & 7
        assert tx < tnx - 1 and y >> 3 < tny - 1
        empty = not tile_set[y >> 3, tx]
        n_empty += empty
        avail = 16 - j
        ok, run = _rule(full[y + 1, x + 1:x + 1 + avail], full[y, x + 1:x + 1 + avail], kind)
        if not ok:
            continue
        if run == avail:
            avail = 8 * min(8, tnx - tx) - j
            ok, run = _rule(full[y + 1, x + 1:x + 1 + avail], full[y, x + 1:x + 1 + avail], kind)
            n64 += 1
            n_long += run == avail
            if not ok:
                continue
        kept_empty += empty
        res[kind].append((y << 16) | x)
    return {"outer": np.array(sorted(res[0]), np.uint32), "hole": np.array(sorted(res[1]), np.uint32), "n_start": int(len(cy)), "n64": int(n64),
            "n_long": int(n_long), "n_empty_tile": int(n_empty), "kept_empty_tile": int(kept_empty)}


def queued_tiles(binimg):
    """The tiles the kernel evaluates, at the granularity of the non-empty-tile bitmap: a tile that holds a pixel, or an empty one whose left AND
    upper neighbours both do (only pixel (0, 0) of an empty tile can start anything, a hole, and needs both). Returns (that mask over the real
    tiles, the wider mask "it, its left or its upper neighbour holds a pixel", the mask of tiles holding a start-rule pixel before drop_single)."""
    b = np.asarray(binimg) != 0
    H, W = b.shape
    tnx, tny = _tiles(W), _tiles(H)
    full = np.zeros((8 * tny + 1, 8 * tnx + 2), bool)
    full[1:H + 1, 1:W + 1] = b
    c = full[1:, 1:-1]
    ys, xs = np.mgrid[0:8 * tny, 0:8 * tnx]
    start = (c & ~(full[1:, :-2] | full[:-1, :-2] | full[:-1, 1:-1] | full[:-1, 2:])) | (~c & full[1:, :-2] & full[:-1, 1:-1] & (xs <= W - 2) & (ys <= H - 2))
    per_tile = lambda a: a.reshape(tny, 8, tnx, 8).any(axis=(1, 3))[:tny - 1, :tnx - 1]
    own = per_tile(c)
    left = np.zeros_like(own)
    left[:, 1:] = own[:, :-1]
    up = np.zeros_like(own)
    up[1:] = own[:-1]
    return own | (left & up), own | left | up, per_tile(start)


# ---- hand-made binary frames (set = True); a test feeds them as gray = 0 where set, 255 elsewhere under a FIXED threshold of 128

def bars_frame(W=1100, H=40):
    """Horizontal runs of 10, 17, 70 and 200 pixels that start at column 0 and column 7 of a tile, as outer starts (a bar, rows 2 + 3i) and as hole
    starts (a slot in a 3-row slab, rows 18 + 4i), each three times: alone, with a blocker the rule must see (the last column it looks at, or column 30
    of a run longer than the horizon) and with one just outside (one column further, or the first column past the horizon). Then runs of 17 and 70 that
    cross x = 1024 and that end in the last admissible column. Returns (image, {kind: [(x, y, expected to survive)]})."""
    b = np.zeros((H, W), bool)
    want = {0: [], 1: []}
    cursor = {0: [8, 2], 1: [8, 18]}     # next free x and the band's row, per kind

    def place(kind, L, x, y, blk):
        horizon = 8 * min(8, _tiles(W) - (x >> 3)) - (x & 7)
        if kind == 0:
            b[y, x:x + L] = True
            if blk is not None:
                b[y - 1, x + blk] = True
            keep = blk is None or blk < 2 or blk > min(L, horizon - 1)
        else:
            b[y - 1:y + 2, x - 1:x + L + 1] = True
            b[y, x:x + L] = False
            if blk is not None:
                b[y - 1, x + blk] = False
            keep = blk is None or blk < 1 or blk > min(L - 1, horizon - 1)
        want[kind].append((x, y, keep))

    def put(kind, L, j, blk):
        cur = cursor[kind]
        x = (cur[0] + 7) // 8 * 8 + j
        if x + L + 12 > 1000:               # the columns from 1000 on belong to the seam and last-column runs below
            cur[0], cur[1] = 8, cur[1] + (3 if kind == 0 else 4)
            x = 8 + j
        place(kind, L, x, cur[1], blk)
        cur[0] = x + max(L, blk or 0) + 4

    for kind in (0, 1):
        for j in (0, 7):
            for L in (10, 17, 70, 200):
                last = L if kind == 0 else L - 1          # the last column of the row above the rule looks at, for a run inside the horizon
                for blk in ((None, last, last + 1) if L < 57 else (None, 30, 64 - j)):
                    put(kind, L, j, blk)
    assert cursor[0][1] <= 14 and cursor[1][1] <= 34, cursor
    # across the strip seam (x = 1024) and into the last admissible column (W - 2), on bands of their own rows
    for kind, rows in ((0, (2, 5, 8, 11)), (1, (18, 22, 26, 30))):
        end = W - 2 if kind == 0 else W - 3          # a slot needs its closing pixel inside the frame
        place(kind, 17, 1015, rows[0], None)
        place(kind, 70, 1016, rows[1], 30)
        place(kind, 17, end - 16, rows[2], None)
        place(kind, 70, end - 69, rows[3], None)
        place(kind, 17, 1040, rows[0], 17 if kind == 0 else 16)
    assert not b[0].any() and not b[-1].any() and not b[:, 0].any() and not b[:, -1].any()
    return b, want


def _empty_tile_case(b, tx, ty, left=True, upper=True, exact=True):
    """Tile (tx, ty) stays empty; its pixel (0, 0) is a hole start that survives when both the left tile's (row 0, column 7) and the upper tile's
    (row 7, column 0) are set (the row above the clear run is set up to the run's end in the right neighbour tile)."""
    x0, y0 = 8 * tx, 8 * ty
    if left:
        b[y0 if exact else y0 + 1, x0 - 1] = True
    if upper:
        if exact:
            b[y0 - 1, x0:x0 + 9] = True
        else:
            b[y0 - 1, x0 + 1:x0 + 9] = True
    if exact and left and upper:
        b[y0, x0 + 8] = True          # ends the clear run after 8 pixels
    return (y0 << 16) | x0


def empty_tile_frame():
    """64 x 64: a hole start at pixel (0, 0) of an empty tile (3, 3), and the near misses: only the left neighbour non-empty (tile (1, 6)), only the
    upper one (tile (6, 1)), both non-empty but not at the two pixels that matter (tile (5, 5)). Returns (image, the one expected hole start)."""
    b = np.zeros((64, 64), bool)
    hit = _empty_tile_case(b, 3, 3)
    _empty_tile_case(b, 1, 6, upper=False)
    _empty_tile_case(b, 6, 1, left=False)
    _empty_tile_case(b, 5, 5, exact=False)
    return b, hit


def empty_tile_seam_frame():
    """1040 x 64: the same at the strip seam, tile column 128 (its left neighbour is the previous strip's last tile): the start in tile row 2, only
    the left neighbour non-empty in tile row 4, only the upper one in tile row 6. Returns (image, the one expected hole start)."""
    b = np.zeros((64, 1040), bool)
    hit = _empty_tile_case(b, 128, 2)
    _empty_tile_case(b, 128, 4, upper=False)
    _empty_tile_case(b, 128, 6, left=False)
    return b, hit


def last_column_row_frame(W, H):
    """Outer and hole start-rule pixels in the last admissible column (W - 2) and row (H - 2), and in the first ones (1)."""
    b = np.zeros((H, W), bool)
    b[5, W - 2] = b[6, W - 3] = True                     # outer start in column W - 2
    b[H - 2, 9] = b[H - 2, 10] = True                    # outer start in row H - 2 (row H - 1 is the frame)
    b[12, W - 3] = b[11, W - 3] = b[11, W - 2] = True    # hole start-rule pixel (W - 2, 12)
    b[H - 3, 20:24] = True
    b[H - 2, 20] = b[H - 2, 23] = True                   # hole start (21, H - 2): the clear run 21..22 under set pixels
    b[1, 1] = b[1, 2] = True                             # outer start at (1, 1)
    b[3, 1] = b[3, 2] = b[4, 1] = b[4, 3] = True         # hole start (2, 4)
    return b
