"""NumPy restatement of the 5x5 fiducial marker generators (src/arucofidmarkers.cpp:40-61, :214-430), the pixel-to-metre conversion
(utils/aruco_board_pix2meters.cpp:54-63) and the optimal marker selection (utils/aruco_selectoptimalmarkers.cpp:53-205), written
from their description. Test infrastructure: the library never imports it."""
import numpy as np

ROW_WORDS = (0x10, 0x17, 0x09, 0x0E)   # the four Hamming(5,3) words of a marker row, bit 4 = leftmost cell
PANEL, CHESSBOARD, FRAME = 0, 1, 2
INT_MAX = 2**31 - 1


def marker_mat(mid):
    """getMarkerMat: 5 x 5 uint8 of 0 / 1"""
    assert 0 <= mid < 1024
    m = np.zeros((5, 5), np.uint8)
    for y in range(5):
        val = ROW_WORDS[(mid >> (2 * (4 - y))) & 3]
        for x in range(5):
            m[y, x] = (val >> (4 - x)) & 1
    return m


def marker_side(size, locked=False):
    return size + 2 * int(np.float32(size) * np.float32(0.25)) if locked else size


def marker_image(mid, size, locked=False):
    """createMarkerImage(id, size, false, locked)"""
    sw = size // 7
    img = np.zeros((size, size), np.uint8)
    bits = marker_mat(mid)
    for y in range(5):
        for x in range(5):
            if bits[y, x]:
                img[(y + 1) * sw:(y + 2) * sw, (x + 1) * sw:(x + 2) * sw] = 255
    if not locked:
        return img
    q = int(np.float32(size) * np.float32(0.25))
    out = np.full((size + 2 * q, size + 2 * q), 255, np.uint8)
    if q:
        out[:q, :q] = 0
        out[-q:, :q] = 0
        out[-q:, -q:] = 0
        out[:q, -q:] = 0
    out[q:q + size, q:q + size] = img
    return out


class RNG:
    """cv::RNG: multiply with carry; operator()(N) = next() % N"""

    def __init__(self, state=0xFFFFFFFF):
        self.state = int(state)

    def next(self):
        self.state = ((self.state & 0xFFFFFFFF) * 4164903690 + (self.state >> 32)) & 0xFFFFFFFFFFFFFFFF
        return self.state & 0xFFFFFFFF

    def __call__(self, n):
        return self.next() % n


def shuffle_ids(rng, n, excluded=()):
    """getListOfValidMarkersIds_random: std::random_shuffle (libstdc++) of 0..1023 with the excluded ids set to -1"""
    assert n + len(excluded) <= 1024
    lst = list(range(1024))
    for e in excluded:
        lst[e] = -1
    for i in range(1, 1024):
        j = rng(i + 1)
        if i != j:
            lst[i], lst[j] = lst[j], lst[i]
    out = []
    k = 0
    while len(out) < n:
        if lst[k] != -1:
            out.append(lst[k])
        k += 1
    return out


def board_layout(btype, gw, gh, size, dist):
    """(width, height, ids drawn from the shuffle, [(x, y) grid cell of every placed marker in order], pitch)"""
    if btype == PANEL:
        cells = [(x, y) for y in range(gh) for x in range(gw)]
        return gw * size + (gw - 1) * dist, gh * size + (gh - 1) * dist, gw * gh, cells, size + dist
    if btype == CHESSBOARD:
        cells = []
        for y in range(gh):
            to_write = y % 2 != 0
            for x in range(gw):
                to_write = not to_write
                if to_write:
                    cells.append((x, y))
        return gw * size, gh * size, 3 * (gw * gh) // 4, cells, size
    assert btype == FRAME
    cells = [(x, y) for y in range(gh) for x in range(gw) if y == 0 or y == gh - 1 or x == 0 or x == gw - 1]
    return gw * size + (gw - 1) * dist, gh * size + (gh - 1) * dist, 2 * gh * 2 * gw, cells, size + dist


def board_image(btype, gw, gh, size, dist, ids, centered=True):
    """(image, ids used, objPoints float32 [markers][4][3]); None when the chessboard places more markers than it draws ids"""
    W, H, drawn, cells, pitch = board_layout(btype, gw, gh, size, dist)
    if btype == CHESSBOARD and len(cells) > drawn:
        return None
    assert len(ids) >= len(cells)
    img = np.full((H, W), 255, np.uint8)
    obj = np.zeros((len(cells), 4, 3), np.float32)
    cx, cy = W // 2, H // 2
    for k, (x, y) in enumerate(cells):
        x0, y0 = x * pitch, y * pitch
        img[y0:y0 + size, x0:x0 + size] = marker_image(ids[k], size)
        c = np.array([[x0, y0, 0], [x0 + size, y0, 0], [x0 + size, y0 + size, 0], [x0, y0 + size, 0]], np.float32)
        if btype == PANEL or centered:
            c = c - np.array([cx, cy, 0], np.float32)
        obj[k] = c
    return img, list(ids[:len(cells)]), obj


def pix_to_meters(obj, marker_size_m):
    obj = np.asarray(obj, np.float32)
    d = (obj[0, 0] - obj[0, 1]).astype(np.float64)
    px = int(np.sqrt(np.sum(d * d)))
    pix = np.float32(marker_size_m) / np.float32(px)
    return (obj * pix).astype(np.float32)


# ---- aruco_selectoptimalmarkers

def entropy(m):
    e = 0
    for y in range(5):
        for x in range(5):
            for yy in range(max(y - 1, 0), min(y + 1, 5)):
                for xx in range(max(x - 1, 0), min(x + 1, 5)):
                    e += int(m[y, x] != m[yy, xx])
    return e


def rotate(m):
    out = m.copy()
    for i in range(5):
        for j in range(5):
            out[i, j] = m[5 - j - 1, i]
    return out


def distance_matrix():
    """[1024][1024] int32: the minimum over the four rotations of the first marker of the 25-cell Hamming distance"""
    mats = np.stack([marker_mat(i) for i in range(1024)]).reshape(1024, 25).astype(np.int32)
    best = np.full((1024, 1024), 99, np.int32)
    rot = np.stack([marker_mat(i) for i in range(1024)])
    for _ in range(4):
        r = rot.reshape(1024, 25).astype(np.int32)
        # Hamming distance of 0/1 vectors: |a| + |b| - 2 a.b
        d = r.sum(1)[:, None] + mats.sum(1)[None, :] - 2 * (r @ mats.T)
        best = np.minimum(best, d)
        rot = np.stack([rotate(m) for m in rot])
    return best.astype(np.int32)


def entropies():
    return np.array([entropy(marker_mat(i)) for i in range(1024)], np.int32)


def select(n_markers, min_entropy=0, dist=None, ent=None):
    """(ok, sorted ids, min pairwise distance); ok False where the reference prints COUDL NOT ADD ANY MARKER (ids: those found so far)"""
    dist = distance_matrix() if dist is None else dist
    ent = entropies() if ent is None else ent
    best = 0
    for i in range(1024):
        if ent[i] > ent[best]:
            best = i
    selected = [best]
    used = ent < min_entropy
    used[best] = True
    ok = True
    run_min = dist[best].copy()   # every marker's minimum distance to the selected set
    for _ in range(1, n_markers):
        cand = np.where(used, 0, run_min)
        best_marker = int(np.argmax(cand))   # the first of the largest: strict > keeps the lowest id
        if cand[best_marker] > 1:
            selected.append(best_marker)
            used[best_marker] = True
            run_min = np.minimum(run_min, dist[best_marker])
        else:
            ok = False
            break
    selected.sort()
    md = INT_MAX
    for a in range(len(selected) - 1):
        for b in range(a + 1, len(selected)):
            md = min(md, int(dist[selected[a], selected[b]]))
    return ok, selected, md
