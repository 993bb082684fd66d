// The default 5x5 Hamming markers made on the device (src/arucofidmarkers.cpp: createMarkerImage :214-260, createBoardImage* :290-430;
// utils/aruco_selectoptimalmarkers.cpp :53-205), DESIGN.md "Fiducial marker, board and marker-set generation".
//
//   fid_paint_kernel    every pixel of n images of one layout (FidLayout): a grid of markers on white, or one marker inside the
//                       "locked" frame. A thread owns one 16-byte aligned group of a row's ADDRESSES, so the caller's row stride needs
//                       no alignment: a group that lies wholly inside the row is one 16-byte store, a row's head and tail are byte
//                       stores. The cell under a pixel is found by division once per group and stepped from there.
//   fid_distance_kernel the 1024 x 1024 matrix: minimum over the four rotations of the 25-cell Hamming distance (xor + popcount)
//   fid_select_kernel   the greedy selection, one workgroup of 1024 threads: thread j keeps marker j's minimum distance to the
//                       selected set in a register; every round is one (distance, lowest id) arg-max reduction
#include "internal.h"

namespace ah {

// the four words of a marker row with bit x = cell x ({0x10, 0x17, 0x09, 0x0e} read from the left), 5 bits each
constexpr uint32_t FID_ROWS = 0x01u | (0x1du << 5) | (0x12u << 10) | (0x0eu << 15);

// cells 0..6 of cell row cy of marker `id` as a bit mask (bit cx set = white); the border cells and everything past them are black
__device__ __forceinline__ uint32_t fid_row_mask(int id, int cy) {
    if (cy < 1 || cy > 5) return 0u;
    return ((FID_ROWS >> (5 * ((id >> (2 * (5 - cy))) & 3))) & 31u) << 1;
}

// the 25 cells of marker `id`, bit 5 y + x = cell (y, x)
__device__ __forceinline__ uint32_t fid_word(int id) {
    uint32_t w = 0;
    for (int y = 0; y < 5; y++) w |= ((FID_ROWS >> (5 * ((id >> (2 * (4 - y))) & 3))) & 31u) << (5 * y);
    return w;
}

// the selection utility's rotate(): out(i, j) = in(4 - j, i)
__device__ __forceinline__ uint32_t fid_rotate(uint32_t w) {
    uint32_t o = 0;
    for (int i = 0; i < 5; i++)
        for (int j = 0; j < 5; j++) o |= ((w >> (5 * (4 - j) + i)) & 1u) << (5 * i + j);
    return o;
}

__global__ __launch_bounds__(256) void fid_paint_kernel(FidLayout L, const int32_t* __restrict__ slots, uint8_t* __restrict__ out, size_t row_stride,
                                                        size_t image_stride) {
    const int gpr = L.W / 16 + 2;   // aligned groups that can touch a row of W bytes at any alignment
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= gpr * L.H) return;
    const int y = idx / gpr, g = idx - y * gpr, img = blockIdx.y;
    uint8_t* row = out + (size_t)img * image_stride + (size_t)y * row_stride;
    const int mis = (int)((uintptr_t)row & 15);
    const int x0 = 16 * g - mis;   // the group covers x0 .. x0 + 15
    const int lo = max(x0, 0), hi = min(x0 + 16, L.W);
    if (lo >= hi) return;
    const int32_t* slot = slots + (size_t)img * L.gw * L.gh;
    if (L.sq > 0) {   // a chessboard with the markers inside its white squares: painted once per board, a division per pixel is affordable
        const int sy = y / L.sq, oy = y - sy * L.sq - L.moff;
        uint32_t w[4] = {0, 0, 0, 0};
        for (int x = lo; x < hi; x++) {
            const int sx = x / L.sq, ox = x - sx * L.sq - L.moff;
            uint32_t v = 0u;
            if ((sx + sy) & 1) {
                v = 255u;
                if (ox >= 0 && ox < L.M && oy >= 0 && oy < L.M) v = ((fid_row_mask(slot[sy * L.gw + sx], oy / L.sw) >> (ox / L.sw)) & 1u) ? 255u : 0u;
            }
            const int q = x - x0;
            w[q >> 2] |= v << (8 * (q & 3));
        }
        if (hi - lo == 16) {
            *reinterpret_cast<uint4*>(row + x0) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            for (int x = lo; x < hi; x++) {
                const int q = x - x0;
                row[x] = (uint8_t)(w[q >> 2] >> (8 * (q & 3)));
            }
        }
        return;
    }
    // the row: background only, or cell row cy of grid row gy
    const int ty = y - L.off, pitch = L.pitch;
    bool marker_row = ty >= 0 && ty < L.GH;
    int gy = 0, cy = 0;
    if (marker_row) {
        gy = ty / pitch;
        const int oy = ty - gy * pitch;
        marker_row = oy < L.M;
        cy = oy / L.sw;
    }
    const bool corner_row = L.off > 0 && (y < L.off || y >= L.H - L.off);   // the locked frame's black squares
    uint32_t w[4] = {0, 0, 0, 0};
    bool walking = false;
    int gx = 0, ox = 0, cx = 0, rx = 0;
    uint32_t mask = 0;
    bool placed = false;
    for (int x = lo; x < hi; x++) {
        const int tx = x - L.off;
        uint32_t v;
        if (!marker_row || tx < 0 || tx >= L.GW) {
            v = corner_row && (x < L.off || x >= L.W - L.off) ? 0u : 255u;
        } else {
            if (!walking) {   // the first pixel of this group inside the grid: the only divisions
                gx = tx / pitch, ox = tx - gx * pitch;
                cx = ox / L.sw, rx = ox - cx * L.sw;
                walking = true;
                const int id = slot[gy * L.gw + gx];
                placed = id >= 0, mask = placed ? fid_row_mask(id, cy) : 0u;
            }
            v = ox >= L.M || !placed ? 255u : ((mask >> cx) & 1u) ? 255u : 0u;
            if (++rx == L.sw) rx = 0, cx++;
            if (++ox == pitch) {
                ox = cx = rx = 0, gx++;
                if (gx < L.gw) {
                    const int id = slot[gy * L.gw + gx];
                    placed = id >= 0, mask = placed ? fid_row_mask(id, cy) : 0u;
                }
            }
        }
        const int q = x - x0;
        w[q >> 2] |= v << (8 * (q & 3));
    }
    if (hi - lo == 16) {
        *reinterpret_cast<uint4*>(row + x0) = make_uint4(w[0], w[1], w[2], w[3]);   // row + x0 is 16-byte aligned by construction
    } else {
        for (int x = lo; x < hi; x++) {
            const int q = x - x0;
            row[x] = (uint8_t)(w[q >> 2] >> (8 * (q & 3)));
        }
    }
}

void launch_fid_paint(hipStream_t s, const FidLayout& L, const int32_t* slots, int nimages, uint8_t* out, size_t row_stride, size_t image_stride) {
    const long total = (long)(L.W / 16 + 2) * L.H;
    hipLaunchKernelGGL(fid_paint_kernel, dim3((unsigned)((total + 255) / 256), (unsigned)nimages), dim3(256), 0, s, L, slots, out, row_stride,
                       image_stride);
}

__global__ __launch_bounds__(256) void fid_distance_kernel(int32_t* __restrict__ dist) {
    __shared__ uint32_t rot[4];
    const int i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (threadIdx.x == 0) {
        uint32_t w = fid_word(i);
        for (int r = 0; r < 4; r++) rot[r] = w, w = fid_rotate(w);
    }
    __syncthreads();
    const uint32_t c = fid_word(j);
    dist[(size_t)i * 1024 + j] = min(min(__popc(rot[0] ^ c), __popc(rot[1] ^ c)), min(__popc(rot[2] ^ c), __popc(rot[3] ^ c)));
}

void launch_fid_distances(hipStream_t s, int32_t* dist) {
    hipLaunchKernelGGL(fid_distance_kernel, dim3(4, 1024), dim3(256), 0, s, dist);
}

// entropy(): over every cell, the cells of the 2 x 2 block that ends at it (upper / left neighbours and itself) that differ from it
__device__ __forceinline__ int fid_entropy(uint32_t w) {
    int e = 0;
    for (int y = 0; y < 5; y++)
        for (int x = 0; x < 5; x++) {
            const uint32_t c = (w >> (5 * y + x)) & 1u;
            for (int yy = max(y - 1, 0); yy <= y; yy++)
                for (int xx = max(x - 1, 0); xx <= x; xx++) e += (int)(((w >> (5 * yy + xx)) & 1u) ^ c);
        }
    return e;
}

// max over the workgroup of 1024 threads; every thread gets the result. red: 16 words of LDS
__device__ __forceinline__ uint32_t fid_block_max(uint32_t key, uint32_t* red) {
    for (int d = 32; d >= 1; d >>= 1) key = max(key, (uint32_t)__shfl_xor((int)key, d, 64));
    const int wave = threadIdx.x >> 6;
    __syncthreads();   // the previous round's readers are done with red
    if ((threadIdx.x & 63) == 0) red[wave] = key;
    __syncthreads();
    uint32_t m = red[0];
    for (int k = 1; k < 16; k++) m = max(m, red[k]);
    return m;
}

// res: [0] markers selected, [1] 1 = all n_markers found, [2] smallest pairwise distance of the selection (INT_MAX for one marker),
// [3] the largest entropy; sel: the selection in ascending order
__global__ __launch_bounds__(1024) void fid_select_kernel(int n_markers, int min_entropy, int32_t* __restrict__ sel, int32_t* __restrict__ res) {
    __shared__ uint32_t red[16];
    __shared__ uint32_t chosen[1024 / 32];
    const int j = threadIdx.x;
    const uint32_t c = fid_word(j);
    const int ent = fid_entropy(c);
    if (j < 32) chosen[j] = 0;
    // an arg-max key: value in the high bits, 1023 - id below, so that the largest key is the largest value at the lowest id
    uint32_t best = fid_block_max(((uint32_t)ent << 10) | (uint32_t)(1023 - j), red);
    const int max_entropy = (int)(best >> 10);
    bool used = ent < min_entropy;
    int run_min = 0x7fffffff, count = 0, complete = 1;
    for (int round = 0; round < n_markers; round++) {
        if (round > 0) {
            best = fid_block_max(used ? 0u : ((uint32_t)run_min << 10) | (uint32_t)(1023 - j), red);
            if ((best >> 10) <= 1u) {   // nothing available at a distance above 1
                complete = 0;
                break;
            }
        }
        const int b = 1023 - (int)(best & 1023u);
        uint32_t w = fid_word(b);
        int d = 25;
        for (int r = 0; r < 4; r++) d = min(d, __popc(w ^ c)), w = fid_rotate(w);
        run_min = min(run_min, d);
        if (j == b) used = true, atomicOr(&chosen[j >> 5], 1u << (j & 31));
        count++;
    }
    __syncthreads();
    // ascending order: a selected marker's position is the number of selected markers below it
    const bool mine = (chosen[j >> 5] >> (j & 31)) & 1u;
    int md = 0x7fffffff;
    if (mine) {
        int pos = __popc(chosen[j >> 5] & ((1u << (j & 31)) - 1u));
        for (int k = 0; k < (j >> 5); k++) pos += __popc(chosen[k]);
        sel[pos] = j;
        // the smallest distance to another selected marker
        for (int k = 0; k < 1024; k++) {
            if (k == j || !((chosen[k >> 5] >> (k & 31)) & 1u)) continue;
            uint32_t w = fid_word(k);
            for (int r = 0; r < 4; r++) md = min(md, __popc(w ^ c)), w = fid_rotate(w);
        }
    }
    // min as the max of the complement
    const uint32_t m = fid_block_max(0x7fffffffu - (uint32_t)md, red);
    if (j == 0) res[0] = count, res[1] = complete, res[2] = (int32_t)(0x7fffffffu - m), res[3] = max_entropy;
}

void launch_fid_select(hipStream_t s, int n_markers, int min_entropy, int32_t* sel, int32_t* res) {
    hipLaunchKernelGGL(fid_select_kernel, dim3(1), dim3(1024), 0, s, n_markers, min_entropy, sel, res);
}

}  // namespace ah
