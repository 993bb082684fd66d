"""NumPy restatement of the reference's highly reliable marker tools (src/highlyreliablemarkers.cpp): glibc's rand() stream after
srand(seed), MarkerGenerator::generateMarker, MarkerCode's rotations / ids / distances, createDicitionary and createBoardImage.
It does not call the library. The device code (k_hrm.hip) is checked against it.

Codes are uint64 with bit y*n + x = cell (y, x), the layout of arucohip_set_dictionary. The dictionary walk is the reference's
sequential accept / reject loop; candidates are made in blocks and screened with NumPy, which changes no decision (a candidate's
bits and distances do not depend on tau)."""
import numpy as np

U32 = 0xFFFFFFFF
LIMIT = 100000


# ---- glibc rand(): r[i] = r[i-3] + r[i-31] mod 2^32, output k = r[k + 344] >> 1

def glibc_seed_words(seed):
    """r[0..343]: srand(seed) (16807 LCG by Schrage with C's truncating division) and the 310 discarded outputs."""
    s = seed & U32
    s = s - (1 << 32) if s >= (1 << 31) else s
    if s == 0:
        s = 1
    r = [s]
    for _ in range(1, 31):
        w = r[-1]
        hi = abs(w) // 127773 * (1 if w >= 0 else -1)
        lo = w - hi * 127773
        w = 16807 * lo - 2836 * hi
        if w < 0:
            w += 2147483647
        r.append(w)
    r = [x & U32 for x in r]
    r += r[0:3]
    for i in range(34, 344):
        r.append((r[i - 31] + r[i - 3]) & U32)
    return r


def state_at0(seed):
    """The 31 words r[313..343]: the state from which output 0 is made."""
    return np.array(glibc_seed_words(seed)[313:344], np.uint64)


def rand_python(seed, count):
    """The first `count` outputs, one at a time (the literal definition)."""
    r = glibc_seed_words(seed)
    out = []
    for k in range(count):
        i = k + 344
        r.append((r[i - 31] + r[i - 3]) & U32)
        out.append(r[i] >> 1)
    return out


def _matmul(A, B):
    """(A @ B) mod 2^32 for uint64 arrays holding 32-bit words, in 16-bit halves so that no sum passes 2^64."""
    lo, hi = A & 0xFFFF, A >> 16
    return ((lo @ B) + (((hi @ B) & 0xFFFF) << 16)) & U32


def step_matrix():
    """M: state (r[i-31] .. r[i-1]) -> (r[i-30] .. r[i])."""
    M = np.zeros((31, 31), np.uint64)
    for j in range(30):
        M[j, j + 1] = 1
    M[30, 0] = M[30, 28] = 1
    return M


def matpow(k):
    R = np.eye(31, dtype=np.uint64)
    P = step_matrix()
    while k:
        if k & 1:
            R = _matmul(R, P)
        P = _matmul(P, P)
        k >>= 1
    return R


def stream(seed, offset, count, run=4096):
    """Outputs [offset, offset + count): lanes of `run` consecutive outputs, each lane started by a jump of the state."""
    if count <= 0:
        return np.zeros(0, np.uint32)
    lanes = (count + run - 1) // run
    s = _matmul(matpow(offset), state_at0(seed)[:, None])[:, 0]
    J = matpow(run)
    st = np.zeros((31, lanes), np.uint64)
    for l in range(lanes):
        st[:, l] = s
        s = _matmul(J, s[:, None])[:, 0]
    out = np.zeros((run, lanes), np.uint64)
    for t in range(run):
        v = (st[t % 31] + st[(t + 28) % 31]) & U32
        st[t % 31] = v
        out[t] = v >> 1
    return out.T.reshape(-1)[:count].astype(np.uint32)


# ---- MarkerGenerator::generateMarker: n rows of n outputs each

def generate(values, n):
    """Codes of the candidates whose n*n outputs are the rows of values (shape (N, n*n))."""
    v = np.asarray(values, np.int64).reshape(-1, n, n)
    N = v.shape[0]
    total = (n - 1) * (n - 2) // 2
    code = np.zeros(N, np.uint64)
    ar = np.arange(N)
    for w in range(n):
        rnd = v[:, w, 0] % total
        # first k with weight k > rnd, else nTransitions - 1
        nt = np.minimum(rnd + 1, n - 2)
        perm = np.tile(np.arange(n - 1), (N, 1))
        for i in range(1, n - 1):   # libstdc++ random_shuffle
            j = v[:, w, i] % (i + 1)
            a, b = perm[ar, i].copy(), perm[ar, j].copy()
            perm[ar, i], perm[ar, j] = b, a
        trans = np.zeros((N, n), bool)
        for k in range(n - 1):
            sel = k < nt
            trans[ar[sel], perm[sel, k]] = True
        cur = (v[:, w, n - 1] % 2).astype(np.uint64)
        for k in range(n):
            code |= cur << np.uint64(w * n + k)
            cur = np.where(trans[:, k], 1 - cur, cur).astype(np.uint64)
    return code


def rot_pos(n, r, y, x):
    """MarkerCode::set: position of cell (y, x) in rotation r"""
    if r == 1:
        y, x = x, n - y - 1
    elif r == 2:
        y, x = n - y - 1, n - x - 1
    elif r == 3:
        y, x = n - x - 1, y
    return y * n + x


def rotations(code, n):
    """(N, 4) uint64: the four rotations of each code"""
    c = np.atleast_1d(np.asarray(code, np.uint64))
    out = np.zeros((c.size, 4), np.uint64)
    for y in range(n):
        for x in range(n):
            b = (c >> np.uint64(y * n + x)) & np.uint64(1)
            for r in range(4):
                out[:, r] |= b << np.uint64(rot_pos(n, r, y, x))
    return out


def get_id(code, n, rot=0):
    """getId(rot): sum of 2 << pos over the 1 bits (the reference's int shift: defined for n <= 5 only)"""
    assert n <= 5
    c = int(rotations(code, n)[0, rot])
    return sum(2 << p for p in range(n * n) if (c >> p) & 1)


def popcount(x):
    return np.bitwise_count(np.asarray(x, np.uint64)).astype(np.int64)


def self_distance(code, n):
    rot = rotations(code, n)
    return np.min(popcount(rot[:, 1:] ^ rot[:, :1]), axis=1)


def distance(a, b, n):
    """MarkerCode::distance: min over the rotations of b of the Hamming distance to a's rotation 0"""
    return int(np.min(popcount(rotations(b, n)[0] ^ np.uint64(a))))


def dict_distance(D, cand, n):
    """Dictionary::distance for many candidates: min over D's markers (rotation 0) and the candidates' rotations; n*n when D is empty"""
    rot = rotations(cand, n)
    out = np.full(rot.shape[0], n * n, np.int64)
    for m in D:
        out = np.minimum(out, np.min(popcount(rot ^ np.uint64(m)), axis=1))
    return out


def minimum_distance(D, n):
    """Dictionary::minimunDistance"""
    if len(D) == 0:
        return 0
    best = n * n
    for i, m in enumerate(D):
        best = min(best, int(self_distance(m, n)[0]))
        for m2 in D[i + 1:]:
            best = min(best, distance(m, m2, n))
    return best


def initial_tau(n):
    return 2 * ((4 * ((n * n) // 4)) // 3)


class TauZero(Exception):
    pass


def create_dictionary(n, size, seed, block=65536, events=None):
    """createDicitionary after srand(seed): (codes uint64, tau0, candidates examined). Raises TauZero where the reference raises
    CV_Error. events (a list): gets (candidate index, |D|, new limit) for every tau decrement."""
    tau = initial_tau(n)
    limit, count = LIMIT, 0
    D = []
    base = 0
    while True:
        vals = stream(seed, base * n * n, block * n * n)
        cand = generate(vals.reshape(block, n * n), n)
        selfd = self_distance(cand, n)
        dmin = dict_distance(D, cand, n)
        k = 0
        while k < block:
            last = k + (limit - count) - 1   # the candidate at which the unproductive count reaches the limit
            stop = min(block, last + 1)
            hit = np.flatnonzero((selfd[k:stop] >= tau) & (dmin[k:stop] >= tau))
            if hit.size:
                a = k + int(hit[0])
                D.append(int(cand[a]))
                count = 0
                if len(D) == size:
                    return np.array(D, np.uint64), tau, base + a + 1
                dmin[a + 1:] = np.minimum(dmin[a + 1:], dict_distance([D[-1]], cand[a + 1:], n))
                k = a + 1
            elif last < block:
                tau -= 1
                count = 0
                if tau == 0:
                    raise TauZero(base + last + 1)
                limit = LIMIT if len(D) >= 2 else LIMIT // 15
                if events is not None:
                    events.append((base + last, len(D), limit))
                k = last + 1
            else:
                count += block - k
                k = block
        base += block


def create_dictionary_literal(n, size, rand):
    """createDicitionary one candidate at a time in plain Python, from a rand() callable (small cases only)"""
    pos = [[rot_pos(n, r, y, x) for y in range(n) for x in range(n)] for r in range(4)]

    def rotate(c, r):
        return sum(1 << pos[r][i] for i in range(n * n) if (c >> i) & 1)

    total = (n - 1) * (n - 2) // 2
    tau = initial_tau(n)
    limit, count = LIMIT, 0
    D = []
    k = 0
    while len(D) < size:
        c = 0
        for w in range(n):
            nt = min(rand() % total + 1, n - 2)
            perm = list(range(n - 1))
            for i in range(1, n - 1):
                j = rand() % (i + 1)
                perm[i], perm[j] = perm[j], perm[i]
            sel = set(perm[:nt])
            cur = rand() % 2
            for x in range(n):
                c |= cur << (w * n + x)
                if x in sel:
                    cur = 1 - cur
        k += 1
        rots = [rotate(c, r) for r in range(4)]
        selfd = min(bin(c ^ rots[r]).count("1") for r in (1, 2, 3))
        dist = min([n * n] + [bin(m ^ rr).count("1") for m in D for rr in rots])
        if selfd >= tau and dist >= tau:
            D.append(c)
            count = 0
        else:
            count += 1
            if count == limit:
                tau -= 1
                count = 0
                if tau == 0:
                    raise TauZero(k)
                limit = LIMIT if len(D) >= 2 else LIMIT // 15
    return np.array(D, np.uint64), tau, k


# ---- createBoardImage

def board_geometry(n, gw, gh):
    ms = (n + 2) * 20
    gap = ms // 5
    return ms, gap, gw * ms + (gw - 1) * gap, gh * ms + (gh - 1) * gap


def marker_image(code, n, pix):
    """getImg(pix): black border, white = bit 1"""
    rows = n + 2
    if pix % rows:
        pix = pix + rows - pix % rows
    cell = pix // rows
    img = np.zeros((pix, pix), np.uint8)
    for i in range(n):
        for j in range(n):
            if (int(code) >> (i * n + j)) & 1:
                img[(i + 1) * cell:(i + 2) * cell, (j + 1) * cell:(j + 2) * cell] = 255
    return img


def board_image(codes, n, gw, gh, chromatic=False):
    """(image, ids or None for n >= 6, obj (gw*gh, 4, 3) float32)"""
    ms, gap, sx, sy = board_geometry(n, gw, gh)
    cx, cy = np.float32(sx / 2.0), np.float32(sy / 2.0)
    img = np.full((sy, sx), 255, np.uint8)
    ids, obj = [], []
    idp = 0
    for y in range(gh):
        for x in range(gw):
            ox, oy = x * (gap + ms), y * (gap + ms)
            img[oy:oy + ms, ox:ox + ms] = marker_image(codes[idp], n, ms)
            if n <= 5:
                ids.append(get_id(codes[idp], n))
            corners = [(ox, oy), (ox + ms, oy), (ox + ms, oy + ms), (ox, oy + ms)]
            obj.append([[np.float32(np.float32(px) - cx), -np.float32(np.float32(py) - cy), np.float32(0)] for px, py in corners])
            idp += 1
    if chromatic:
        out = np.empty((sy + 2 * gap, sx + 2 * gap, 3), np.uint8)
        out[:] = (250, 134, 4)
        inner = out[gap:gap + sy, gap:gap + sx]
        inner[img == 0] = (0, 255, 0)
        img = out
    return img, (np.array(ids, np.int64) if n <= 5 else None), np.array(obj, np.float32)
