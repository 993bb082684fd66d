// Highly reliable marker dictionaries and boards (src/highlyreliablemarkers.cpp: MarkerGenerator :58-116, createDicitionary
// :567-608, createBoardImage :498-565), DESIGN.md "HRM dictionary and board generation".
//
// glibc's rand() after srand(seed) is the additive recurrence r[i] = r[i-3] + r[i-31] mod 2^32, output k = r[k + 344] >> 1. The state
// at output p is the 31 words r[p + 313 .. p + 343]; the state at p + k is M^k times it, with M the step matrix. The host computes
// the jump matrices, so every lane starts its run of consecutive outputs from the window's state by at most one matrix-vector
// product per set bit of its lane index. A candidate consumes exactly n*n outputs, so candidate c is a pure function of outputs
// [c n^2, (c + 1) n^2).
//
// Dictionary walk, one window of HRM_WINDOW candidates at a time:
//   hrm_gen_kernel    the window's codes and self distances (one lane per HRM_LANE_CANDS consecutive candidates)
//   hrm_dmin_kernel   each candidate's distance to the current dictionary (one thread per candidate)
//   hrm_decide_kernel one workgroup: the reference's sequential accept / reject loop over the window. The next acceptance is the first
//                     candidate from the current one with self >= tau and dmin >= tau; it is compared with the candidate at which the
//                     unproductive count reaches the limit. An acceptance updates the window's later candidates against the new marker
//                     alone. The kernel then advances the stream state by one window.
#include "internal.h"

namespace ah {

// state s <- J_b s for every set bit b of k (J_b = tab + b * 961, row-major, mod 2^32)
__device__ __forceinline__ void hrm_jump(const uint32_t* __restrict__ tab, uint64_t k, int nbits, uint32_t s[HRM_STATE]) {
    for (int b = 0; b < nbits; b++) {
        if (!((k >> b) & 1)) continue;
        const uint32_t* J = tab + (size_t)b * HRM_STATE * HRM_STATE;
        uint32_t t[HRM_STATE];
#pragma unroll
        for (int i = 0; i < HRM_STATE; i++) {
            uint32_t acc = 0;
#pragma unroll
            for (int j = 0; j < HRM_STATE; j++) acc += J[i * HRM_STATE + j] * s[j];
            t[i] = acc;
        }
#pragma unroll
        for (int i = 0; i < HRM_STATE; i++) s[i] = t[i];
    }
}

// A lane's run of outputs from its state, in an LDS ring indexed by the lane's own step t (the same for every lane of the block):
// slot t % 31 holds r[t - 31], slot (t + 28) % 31 holds r[t - 3].
struct HrmRing {
    uint32_t (*ring)[HRM_GEN_BLOCK];
    int tid, t, t3;
    __device__ __forceinline__ uint32_t next() {
        const uint32_t v = ring[t][tid] + ring[t3][tid];
        ring[t][tid] = v;
        t = t == HRM_STATE - 1 ? 0 : t + 1;
        t3 = t3 == HRM_STATE - 1 ? 0 : t3 + 1;
        return v >> 1;
    }
};

// MarkerCode::set: the position of cell (y, x) in rotation r
__device__ __host__ __forceinline__ int hrm_rot_pos(int n, int r, int y, int x) {
    return r == 0 ? y * n + x : r == 1 ? x * n + (n - 1 - y) : r == 2 ? (n - 1 - y) * n + (n - 1 - x) : (n - 1 - x) * n + y;
}

__device__ __forceinline__ uint64_t hrm_rotate(uint64_t c, int n, int r) {
    uint64_t o = 0;
    for (int y = 0; y < n; y++)
        for (int x = 0; x < n; x++) o |= ((c >> (y * n + x)) & 1ull) << hrm_rot_pos(n, r, y, x);
    return o;
}

// MarkerGenerator::generateMarker from the ring: per row rand() % totalWeight, random_shuffle of the n - 1 transition indices
// (libstdc++: j = rand() % (i + 1) for i = 1 .. n - 2), rand() % 2. The permutation is kept as nibbles.
__device__ __forceinline__ uint64_t hrm_generate(HrmRing& g, int n) {
    const uint32_t total = (uint32_t)((n - 1) * (n - 2) / 2);
    uint64_t code = 0;
    for (int w = 0; w < n; w++) {
        const uint32_t rnd = g.next() % total;
        const int nt = (int)min(rnd + 1u, (uint32_t)(n - 2));   // the first weight k > rnd, else nTransitions - 1
        uint32_t perm = 0;
        for (int i = 0; i < n - 1; i++) perm |= (uint32_t)i << (4 * i);
        for (int i = 1; i < n - 1; i++) {
            const int j = (int)(g.next() % (uint32_t)(i + 1));
            const uint32_t pi = (perm >> (4 * i)) & 15u, pj = (perm >> (4 * j)) & 15u;
            perm &= ~((15u << (4 * i)) | (15u << (4 * j)));
            perm |= (pj << (4 * i)) | (pi << (4 * j));
        }
        uint32_t trans = 0;
        for (int k = 0; k < nt; k++) trans |= 1u << ((perm >> (4 * k)) & 15u);
        uint32_t cur = g.next() % 2u;
        for (int k = 0; k < n; k++) {
            code |= (uint64_t)cur << (w * n + k);
            cur ^= (trans >> k) & 1u;
        }
    }
    return code;
}

__global__ __launch_bounds__(HRM_GEN_BLOCK) void hrm_gen_kernel(int n, const uint32_t* __restrict__ state, const uint32_t* __restrict__ jumps,
                                                                uint64_t* __restrict__ code, uint8_t* __restrict__ selfd) {
    __shared__ uint32_t ring[HRM_STATE][HRM_GEN_BLOCK];
    const int tid = threadIdx.x;
    const int lane = blockIdx.x * HRM_GEN_BLOCK + tid;
    uint32_t s[HRM_STATE];
#pragma unroll
    for (int i = 0; i < HRM_STATE; i++) s[i] = state[i];
    hrm_jump(jumps, (uint64_t)lane, HRM_LANE_BITS, s);
#pragma unroll
    for (int i = 0; i < HRM_STATE; i++) ring[i][tid] = s[i];
    HrmRing g{ring, tid, 0, HRM_STATE - 3};
    for (int c = 0; c < HRM_LANE_CANDS; c++) {
        const uint64_t c0 = hrm_generate(g, n);
        int sd = n * n;
        for (int r = 1; r < 4; r++) sd = min(sd, __popcll(c0 ^ hrm_rotate(c0, n, r)));
        const int k = lane * HRM_LANE_CANDS + c;
        code[k] = c0;
        selfd[k] = (uint8_t)sd;
    }
}

// Dictionary::distance against the current dictionary (4 rotations per marker): n*n when it is empty
__global__ __launch_bounds__(256) void hrm_dmin_kernel(int n, const uint64_t* __restrict__ code, const uint64_t* __restrict__ dict,
                                                       const HrmCtl* __restrict__ ctl, uint8_t* __restrict__ dmin) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    const uint64_t c = code[k];
    const int nd = ctl->dsize;
    int d = n * n;
    for (int i = 0; i < nd; i++) {
        const uint64_t* m = dict + 4 * (size_t)i;
        d = min(d, min(min(__popcll(c ^ m[0]), __popcll(c ^ m[1])), min(__popcll(c ^ m[2]), __popcll(c ^ m[3]))));
    }
    dmin[k] = (uint8_t)d;
}

__global__ __launch_bounds__(HRM_DECIDE_BLOCK) void hrm_decide_kernel(int n, int target, const uint64_t* __restrict__ code,
                                                                      const uint8_t* __restrict__ selfd, uint8_t* __restrict__ dmin,
                                                                      uint64_t* __restrict__ dict, HrmCtl* __restrict__ ctl,
                                                                      uint32_t* __restrict__ state, const uint32_t* __restrict__ jump_window) {
    __shared__ HrmCtl c;
    __shared__ int found;
    __shared__ uint64_t rot[4];
    __shared__ uint32_t s_old[HRM_STATE];
    const int tid = threadIdx.x;
    if (tid == 0) c = *ctl;
    __syncthreads();
    if (c.status != HRM_RUNNING) return;
    int start = 0;
    // every pass accepts a marker, lowers tau or leaves the window: at most target + tau + 1 passes
    const int passes = target + c.tau + 1;
    int pass = 0;
    for (; pass < passes; pass++) {
        const int tau = c.tau;
        const int64_t last = (int64_t)start + (c.limit - c.count) - 1;   // the candidate at which the unproductive count reaches the limit
        const int stop = (int)min((int64_t)HRM_WINDOW, last + 1);
        if (tid == 0) found = HRM_WINDOW;
        __syncthreads();
        for (int c0 = start; c0 < stop; c0 += HRM_DECIDE_BLOCK) {
            const int k = c0 + tid;
            if (k < stop && selfd[k] >= tau && dmin[k] >= tau) atomicMin(&found, k);
            __syncthreads();
            const bool hit = found < HRM_WINDOW;
            __syncthreads();   // every thread has read `found` before the next chunk can lower it
            if (hit) break;
        }
        const int a = found;
        __syncthreads();
        if (a < HRM_WINDOW) {   // accept candidate a
            if (tid < 4) rot[tid] = hrm_rotate(code[a], n, tid);
            __syncthreads();
            if (tid == 0) {
                uint64_t* m = dict + 4 * (size_t)c.dsize;
                reinterpret_cast<ulonglong2*>(m)[0] = make_ulonglong2(rot[0], rot[1]);
                reinterpret_cast<ulonglong2*>(m)[1] = make_ulonglong2(rot[2], rot[3]);
                c.dsize++;
                c.count = 0;
                c.examined = c.base + a + 1;
                c.accepted++;
                if (c.dsize == target) c.status = HRM_DONE;
            }
            const uint64_t r0 = rot[0], r1 = rot[1], r2 = rot[2], r3 = rot[3];
            for (int k = a + 1 + tid; k < HRM_WINDOW; k += HRM_DECIDE_BLOCK) {
                const uint64_t x = code[k];
                const int d = min(min(__popcll(x ^ r0), __popcll(x ^ r1)), min(__popcll(x ^ r2), __popcll(x ^ r3)));
                if (d < dmin[k]) dmin[k] = (uint8_t)d;
            }
            start = a + 1;
        } else if (last < HRM_WINDOW) {   // the limit is reached at candidate `last`: lower tau
            if (tid == 0) {
                c.tau--;
                c.count = 0;
                c.examined = c.base + last + 1;
                c.decrements++;
                if (c.tau == 0)
                    c.status = HRM_TAU_ZERO;
                else
                    c.limit = c.dsize >= 2 ? HRM_LIMIT : HRM_LIMIT / 15;
            }
            start = (int)last + 1;
        } else {   // neither inside the window
            if (tid == 0) c.count += HRM_WINDOW - start;
            start = HRM_WINDOW;
        }
        __syncthreads();
        if (c.status != HRM_RUNNING || start >= HRM_WINDOW) break;
    }
    if (pass == passes && tid == 0) c.status = HRM_INTERNAL;
    // the next window's state: J_window times this one
    if (tid < HRM_STATE) s_old[tid] = state[tid];
    __syncthreads();
    if (tid < HRM_STATE) {
        uint32_t acc = 0;
        for (int j = 0; j < HRM_STATE; j++) acc += jump_window[tid * HRM_STATE + j] * s_old[j];
        state[tid] = acc;
    }
    if (tid == 0) {
        c.base += HRM_WINDOW;
        c.windows++;
        *ctl = c;
    }
}

// outputs [offset + lane * HRM_DBG_RUN, ...) of the stream whose state at output 0 is state0; pow2 = M^(2^b), b < HRM_POW_BITS
__global__ __launch_bounds__(HRM_GEN_BLOCK) void hrm_stream_kernel(const uint32_t* __restrict__ state0, const uint32_t* __restrict__ pow2,
                                                                   uint64_t offset, int count, uint32_t* __restrict__ out) {
    __shared__ uint32_t ring[HRM_STATE][HRM_GEN_BLOCK];
    const int tid = threadIdx.x;
    const int lane = blockIdx.x * HRM_GEN_BLOCK + tid;
    uint32_t s[HRM_STATE];
#pragma unroll
    for (int i = 0; i < HRM_STATE; i++) s[i] = state0[i];
    hrm_jump(pow2, offset + (uint64_t)lane * HRM_DBG_RUN, HRM_POW_BITS, s);
#pragma unroll
    for (int i = 0; i < HRM_STATE; i++) ring[i][tid] = s[i];
    HrmRing g{ring, tid, 0, HRM_STATE - 3};
    for (int t = 0; t < HRM_DBG_RUN; t++) {
        const uint32_t v = g.next();
        const int k = lane * HRM_DBG_RUN + t;
        if (k < count) out[k] = v;
    }
}

void launch_hrm_window(hipStream_t s, int n, int target, const HrmBufs& b) {
    hipLaunchKernelGGL(hrm_gen_kernel, dim3(HRM_WINDOW / HRM_LANE_CANDS / HRM_GEN_BLOCK), dim3(HRM_GEN_BLOCK), 0, s, n, b.state, b.jumps, b.code,
                       b.selfd);
    hipLaunchKernelGGL(hrm_dmin_kernel, dim3(HRM_WINDOW / 256), dim3(256), 0, s, n, b.code, b.dict, b.ctl, b.dmin);
    hipLaunchKernelGGL(hrm_decide_kernel, dim3(1), dim3(HRM_DECIDE_BLOCK), 0, s, n, target, b.code, b.selfd, b.dmin, b.dict, b.ctl, b.state,
                       b.jumps + (size_t)HRM_LANE_BITS * HRM_STATE * HRM_STATE);
}

void launch_hrm_stream(hipStream_t s, const uint32_t* state0, const uint32_t* pow2, uint64_t offset, int count, uint32_t* out) {
    const int lanes = (count + HRM_DBG_RUN - 1) / HRM_DBG_RUN;
    hipLaunchKernelGGL(hrm_stream_kernel, dim3((lanes + HRM_GEN_BLOCK - 1) / HRM_GEN_BLOCK), dim3(HRM_GEN_BLOCK), 0, s, state0, pow2, offset, count,
                       out);
}

// ---- createBoardImage. One thread writes 16 bytes of a row (row stride a multiple of 16).
// Gray: white background, each marker getImg(MarkerSize) (20-pixel cells, black border, white = bit 1). Chromatic: a gap-wide margin,
// (250,134,4) everywhere except the gray image's black pixels, which become (0,255,0) (B, G, R).
__device__ __forceinline__ int hrm_board_gray(const uint64_t* codes, int n, int gw, int gh, int x, int y) {
    const int ms = (n + 2) * 20, pitch = ms + ms / 5;
    const int gx = x / pitch, ox = x - gx * pitch, gy = y / pitch, oy = y - gy * pitch;
    if (ox >= ms || oy >= ms) return 255;
    const int i = oy / 20 - 1, j = ox / 20 - 1;
    if (i < 0 || j < 0 || i >= n || j >= n) return 0;
    return ((codes[gy * gw + gx] >> (i * n + j)) & 1ull) ? 255 : 0;
}

__global__ __launch_bounds__(256) void hrm_board_kernel(const uint64_t* __restrict__ codes, int n, int gw, int gh, int chromatic, int W, int H,
                                                        int row_bytes, size_t stride, uint8_t* __restrict__ out) {
    const int chunks = (row_bytes + 15) / 16;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= chunks * H) return;
    const int y = idx / chunks, b0 = (idx - y * chunks) * 16;
    const int gap = (n + 2) * 20 / 5;
    uint32_t w[4] = {0, 0, 0, 0};
    for (int q = 0; q < 16; q++) {
        const int b = b0 + q;
        if (b >= row_bytes) break;
        int v;
        if (!chromatic) {
            v = hrm_board_gray(codes, n, gw, gh, b, y);
        } else {
            const int x = b / 3, ch = b - 3 * x, tx = x - gap, ty = y - gap;
            const bool green = tx >= 0 && ty >= 0 && tx < W - 2 * gap && ty < H - 2 * gap && hrm_board_gray(codes, n, gw, gh, tx, ty) == 0;
            v = green ? (ch == 1 ? 255 : 0) : (ch == 0 ? 250 : ch == 1 ? 134 : 4);
        }
        w[q >> 2] |= (uint32_t)v << (8 * (q & 3));
    }
    *reinterpret_cast<uint4*>(out + (size_t)y * stride + b0) = make_uint4(w[0], w[1], w[2], w[3]);
}

void launch_hrm_board(hipStream_t s, const uint64_t* codes, int n, int gw, int gh, int chromatic, int W, int H, int channels, size_t stride,
                      uint8_t* out) {
    const int row_bytes = W * channels, chunks = (row_bytes + 15) / 16;
    const long total = (long)chunks * H;
    hipLaunchKernelGGL(hrm_board_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, codes, n, gw, gh, chromatic, W, H, row_bytes,
                       stride, out);
}

}  // namespace ah
