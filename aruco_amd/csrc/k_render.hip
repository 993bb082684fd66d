// Mesh rendering: flat-shaded triangle meshes at marker and board poses, depth-tested, painted into frames that stay on the device
// (DESIGN.md "Mesh rendering"). The rule for a pixel is the one arucohip.h states at arucohip_render_markers_batch; tests/render_ref.py
// restates it. Steps per chunk of frames:
//   instances  a lane per marker slot (per board) leaves the internal instance record: pose, product of the scales, an empty box;
//   vertices   a lane per instance and vertex transforms, projects (pnp_device.h, double) and snaps to 1/16 pixel: once per instance;
//   triangles  a lane per instance and triangle tests its indices, culls, shades and leaves a 64-byte record in the order that makes the
//              interior positive; the instance's box grows by one atomic min / max per wave;
//   raster     one workgroup per 64 x 16 tile and frame GATHERS (the overlay's shape): the frame's instance boxes against the tile, then
//              the surviving instances' triangles, compacted in order into an LDS bin by ballot and prefix count. When the bin cannot take
//              another 256 it is walked: every lane carries the best 1 / z and colour of its four pixels in registers across the rounds.
//              A pixel has one owner lane: no atomics on pixels, no depth buffer, the same bytes on every run. A tile that no box touches
//              reads and writes no image byte.
// Every loop runs to a count known at launch (slots, ntris, the bin's fill).
#include <limits.h>
#include <stddef.h>

#include "convert_device.h"
#include "internal.h"
#include "pnp_device.h"

namespace ah {

constexpr double RD_LIMIT = 1048576.;   // a projection beyond +-2^20 pixels (or not finite) drops its triangles

struct RdInst {
    double r[3], t[3], s;        // rvec, tvec, scale * (ssize for a marker)
    int32_t valid;
    int32_t x0, y0, x1, y1;      // inclusive pixel box of the surviving triangles (x1 < x0: none)
    int32_t pad_;
};
struct RdVert {
    double cx, cy, cz;           // camera frame
    double iz;                   // 1 / cz
    int32_t X, Y;                // 1/16 pixel; X == INT_MIN: the vertex drops its triangles
};
// the triangle as the raster takes it: a, b, c reordered so that A > 0 and the interior has E_bc, E_ca, E_ab > 0
struct RdTri {
    double iz[3];
    int64_t A;
    int32_t X[3], Y[3];
    uint32_t color;              // shaded B | G << 8 | R << 16 | gray_of(B, G, R) << 24
    uint32_t live;               // 0: dropped
};
static_assert(offsetof(RdTri, X) == 32 && offsetof(RdTri, live) == 60, "the raster reads a record as four 16-byte words");
static_assert(sizeof(RdInst) == RD_INST_BYTES && sizeof(RdVert) == RD_VERT_BYTES && sizeof(RdTri) == RD_TRI_BYTES, "scratch layout (internal.h)");

__device__ inline void rd_inst(RdInst* o, bool valid, const double* r, const double* t, double s) {
    RdInst v = {{r[0], r[1], r[2]}, {t[0], t[1], t[2]}, s, valid ? 1 : 0, INT_MAX, INT_MAX, INT_MIN, INT_MIN, 0};
    *o = v;
}

// lane = slot `gid` of the chunk's nframes * cap slots. A frame whose count is negative (given up) or zero has no instance.
__global__ __launch_bounds__(64) void render_instances_markers_kernel(const arucohip_marker_t* markers, const int32_t* counts, int nframes, int cap,
                                                                      double scale, RdInst* insts) {
    const uint32_t gid = blockIdx.x * 64u + threadIdx.x;
    if (gid >= (uint32_t)nframes * (uint32_t)cap) return;
    const int f = (int)(gid / (uint32_t)cap), i = (int)(gid % (uint32_t)cap);
    const double zero[3] = {0., 0., 0.};
    if (i < min(counts[f], cap)) {
        const arucohip_marker_t m = markers[gid];
        rd_inst(insts + gid, m.has_pose != 0, m.rvec, m.tvec, scale * (double)m.ssize);
    } else {
        rd_inst(insts + gid, false, zero, zero, 0.);
    }
}

__global__ __launch_bounds__(64) void render_instances_boards_kernel(const arucohip_board_t* boards, int nframes, double scale, RdInst* insts) {
    const uint32_t gid = blockIdx.x * 64u + threadIdx.x;
    if (gid >= (uint32_t)nframes) return;
    const arucohip_board_t b = boards[gid];
    rd_inst(insts + gid, b.has_pose != 0, b.rvec, b.tvec, scale);
}

// grid (instances, ceil(nverts / 256)): the instances on x, which has no 65535 limit
__global__ __launch_bounds__(256) void render_vertices_kernel(const RdInst* insts, CamModel cam, const float* vertices, int nverts, RdVert* verts) {
    __shared__ double s_R[9];
    const RdInst in = insts[blockIdx.x];
    if (!in.valid) return;   // uniform over the workgroup
    if (threadIdx.x == 0) {
        double R[9];
        rodrigues_vec2mat(in.r, R, nullptr);
        for (int k = 0; k < 9; k++) s_R[k] = R[k];
    }
    __syncthreads();
    const int i = blockIdx.y * 256 + threadIdx.x;
    if (i >= nverts) return;
    double R[9];
    for (int k = 0; k < 9; k++) R[k] = s_R[k];
    const double X = in.s * (double)vertices[3 * i], Y = in.s * (double)vertices[3 * i + 1], Z = in.s * (double)vertices[3 * i + 2];
    RdVert v;
    v.cx = R[0] * X + R[1] * Y + R[2] * Z + in.t[0];
    v.cy = R[3] * X + R[4] * Y + R[5] * Z + in.t[1];
    v.cz = R[6] * X + R[7] * Y + R[8] * Z + in.t[2];
    v.iz = 1. / v.cz;
    double mx, my;
    project_point(X, Y, Z, R, nullptr, in.t, cam.K, cam.k, &mx, &my, nullptr, nullptr);
    const bool ok = v.cz > 0. && fabs(mx) <= RD_LIMIT && fabs(my) <= RD_LIMIT;   // false for NaN and infinities
    v.X = ok ? (int32_t)rint(mx * 16.) : INT_MIN;
    v.Y = ok ? (int32_t)rint(my * 16.) : 0;
    verts[(size_t)blockIdx.x * nverts + i] = v;
}

__device__ inline int rd_wave_min(int v) {
    for (int o = 32; o; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ inline int rd_wave_max(int v) {
    for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// grid (instances, ceil(ntris / 256))
__global__ __launch_bounds__(256) void render_triangles_kernel(RdInst* insts, RdMesh mesh, RdStyle st, const RdVert* verts, RdTri* tris) {
    const RdInst in = insts[blockIdx.x];
    if (!in.valid) return;   // uniform: the raster never looks at the triangles of an instance whose box is empty
    const int t = blockIdx.y * 256 + threadIdx.x;
    int bx0 = INT_MAX, by0 = INT_MAX, bx1 = INT_MIN, by1 = INT_MIN;
    if (t < mesh.ntris) {
        RdTri o;
        o.live = 0;
        const uint32_t ia = (uint32_t)mesh.triangles[3 * t], ib = (uint32_t)mesh.triangles[3 * t + 1], ic = (uint32_t)mesh.triangles[3 * t + 2];
        const uint32_t nv = (uint32_t)mesh.nverts;
        if (ia < nv && ib < nv && ic < nv) {   // a device mesh cannot be checked on the host: no index leaves the vertex array
            const RdVert* vb = verts + (size_t)blockIdx.x * mesh.nverts;
            const RdVert a = vb[ia], b = vb[ib], c = vb[ic];
            if (a.X != INT_MIN && b.X != INT_MIN && c.X != INT_MIN) {
                const int64_t A = (int64_t)(b.X - a.X) * (int64_t)(c.Y - a.Y) - (int64_t)(b.Y - a.Y) * (int64_t)(c.X - a.X);
                if (A != 0 && !((st.flags & ARUCOHIP_RENDER_CULL_BACK) && A > 0)) {
                    int q = 255;
                    if (!(st.flags & ARUCOHIP_RENDER_UNLIT)) {
                        const double ux = b.cx - a.cx, uy = b.cy - a.cy, uz = b.cz - a.cz, vx = c.cx - a.cx, vy = c.cy - a.cy, vz = c.cz - a.cz;
                        const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
                        const double len = sqrt(nx * nx + ny * ny + nz * nz);
                        double d = nx * st.light[0] + ny * st.light[1] + nz * st.light[2];
                        if (A > 0) d = -d;   // the outward normal points away: turn it towards the camera
                        double lam = d / len;
                        if (!(lam > 0.)) lam = 0.;   // also NaN (a triangle of no extent in space)
                        q = min(max((int)rint((double)st.ambient + (double)(255 - st.ambient) * lam), 0), 255);
                    }
                    uint32_t base = st.color;
                    if (mesh.colors) base = (uint32_t)mesh.colors[3 * t] | (uint32_t)mesh.colors[3 * t + 1] << 8 | (uint32_t)mesh.colors[3 * t + 2] << 16;
                    const uint32_t cb = ((base & 255u) * q + 127u) / 255u, cg = ((base >> 8 & 255u) * q + 127u) / 255u,
                                   cr = ((base >> 16 & 255u) * q + 127u) / 255u;
                    o.color = cb | cg << 8 | cr << 16 | gray_of(cb, cg, cr) << 24;
                    const RdVert &p = A < 0 ? c : b, &r = A < 0 ? b : c;   // A < 0: swap b and c
                    o.A = A < 0 ? -A : A;
                    o.X[0] = a.X, o.X[1] = p.X, o.X[2] = r.X, o.Y[0] = a.Y, o.Y[1] = p.Y, o.Y[2] = r.Y;
                    o.iz[0] = a.iz, o.iz[1] = p.iz, o.iz[2] = r.iz;
                    // the pixels (u, v) whose centres (16 u, 16 v) lie in the box of the snapped vertices
                    const int x0 = (min(min(a.X, b.X), c.X) + 15) >> 4, x1 = max(max(a.X, b.X), c.X) >> 4;
                    const int y0 = (min(min(a.Y, b.Y), c.Y) + 15) >> 4, y1 = max(max(a.Y, b.Y), c.Y) >> 4;
                    if (x0 <= x1 && y0 <= y1) o.live = 1, bx0 = x0, by0 = y0, bx1 = x1, by1 = y1;
                }
            }
        }
        if (!o.live) o.A = 1, o.color = 0, o.X[0] = o.X[1] = o.X[2] = o.Y[0] = o.Y[1] = o.Y[2] = 0, o.iz[0] = o.iz[1] = o.iz[2] = 0.;
        tris[(size_t)blockIdx.x * mesh.ntris + t] = o;
    }
    bx0 = rd_wave_min(bx0), by0 = rd_wave_min(by0), bx1 = rd_wave_max(bx1), by1 = rd_wave_max(by1);
    if ((threadIdx.x & 63) == 0 && bx0 <= bx1) {
        RdInst* g = insts + blockIdx.x;
        atomicMin(&g->x0, bx0), atomicMin(&g->y0, by0), atomicMax(&g->x1, bx1), atomicMax(&g->y1, by1);
    }
}

constexpr int RD_TW = 64, RD_TH = 16, RD_PX = 4;   // the overlay's tile: 64 x 16 pixels, four pixels of one row a lane
constexpr int RD_BIN = 512;                        // triangle records of the LDS bin (32 KiB)

// The edge functions are integers below 2^53: T = double and T = int64_t both evaluate them exactly (arucohip.h, step 4).
template <typename T>
__device__ inline T rd_owned(T dx, T dy) {   // the smallest value of E that covers: 0 on a left or top edge, else 1
    return (dy < (T)0 || (dy == (T)0 && dx > (T)0)) ? (T)0 : (T)1;
}

// the lane's four pixels (px .. px + 3, py) against bin[0 .. n), in order
template <typename T>
__device__ __forceinline__ void rd_walk(const RdTri* bin, int n, int px, int py, double* best, uint32_t* col, uint32_t* cov) {
    const int PX0 = 16 * px, PY = 16 * py;
    for (int k = 0; k < n; k++) {
        const RdTri r = bin[k];
        const int lo_x = min(min(r.X[0], r.X[1]), r.X[2]), hi_x = max(max(r.X[0], r.X[1]), r.X[2]);
        const int lo_y = min(min(r.Y[0], r.Y[1]), r.Y[2]), hi_y = max(max(r.Y[0], r.Y[1]), r.Y[2]);
        if (PY < lo_y || PY > hi_y || PX0 + 16 * (RD_PX - 1) < lo_x || PX0 > hi_x) continue;
        const T ax = (T)r.X[0], ay = (T)r.Y[0], bx = (T)r.X[1], by = (T)r.Y[1], cx = (T)r.X[2], cy = (T)r.Y[2], Px = (T)PX0, Py = (T)PY;
        const T d0x = cx - bx, d0y = cy - by, d1x = ax - cx, d1y = ay - cy, d2x = bx - ax, d2y = by - ay;
        T e0 = d0x * (Py - by) - d0y * (Px - bx);   // E_bc, paired with 1 / z_a
        T e1 = d1x * (Py - cy) - d1y * (Px - cx);   // E_ca, 1 / z_b
        T e2 = d2x * (Py - ay) - d2y * (Px - ax);   // E_ab, 1 / z_c
        const T t0 = rd_owned(d0x, d0y), t1 = rd_owned(d1x, d1y), t2 = rd_owned(d2x, d2y);
        const T s0 = d0y * (T)16, s1 = d1y * (T)16, s2 = d2y * (T)16;
        const double A = (double)r.A;
#pragma unroll
        for (int j = 0; j < RD_PX; j++) {
            if (e0 >= t0 && e1 >= t1 && e2 >= t2) {
                const double iz = ((double)e0 / A) * r.iz[0] + ((double)e1 / A) * r.iz[1] + ((double)e2 / A) * r.iz[2];
                if (!(*cov >> j & 1u) || iz > best[j]) best[j] = iz, col[j] = r.color, *cov |= 1u << j;
            }
            e0 -= s0, e1 -= s1, e2 -= s2;
        }
    }
}

template <int CH, typename T>
__global__ __launch_bounds__(256) void render_raster_kernel(uint8_t* frames, int W, int H, size_t row_stride, size_t frame_stride, const uint8_t* masks,
                                                            size_t mask_row, size_t mask_frame, const RdInst* insts, const RdTri* tris, int slots,
                                                            int ntris, int opacity) {
    __shared__ RdTri s_bin[RD_BIN];
    __shared__ uint64_t s_mask[4];
    __shared__ int s_wcnt[2][4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int tx0 = blockIdx.x * RD_TW, ty0 = blockIdx.y * RD_TH, tx1 = min(tx0 + RD_TW, W) - 1, ty1 = min(ty0 + RD_TH, H) - 1;
    const size_t slot0 = (size_t)blockIdx.z * slots;
    const int px = tx0 + (t % (RD_TW / RD_PX)) * RD_PX, py = ty0 + t / (RD_TW / RD_PX);
    double best[RD_PX] = {0., 0., 0., 0.};
    uint32_t col[RD_PX] = {0, 0, 0, 0}, cov = 0;
    int nbin = 0, par = 0;   // the same in every lane
    for (int base = 0; base < slots; base += 256) {
        bool hit = false;
        if (base + t < slots) {
            const RdInst* g = insts + slot0 + base + t;
            hit = g->valid && g->x0 <= tx1 && g->x1 >= tx0 && g->y0 <= ty1 && g->y1 >= ty0;
        }
        const uint64_t bal = __ballot(hit);
        if (lane == 0) s_mask[wave] = bal;
        __syncthreads();
        for (int w4 = 0; w4 < 4; w4++) {
            uint64_t mask = s_mask[w4];   // the same in every lane: the loops and barriers below are uniform
            while (mask) {
                const int mi = base + w4 * 64 + __builtin_ctzll(mask);
                mask &= mask - 1;
                const RdTri* tr = tris + (slot0 + mi) * (size_t)ntris;
                for (int tb = 0; tb < ntris; tb += 256) {
                    if (nbin + 256 > RD_BIN) {   // the bin cannot take another 256: a round
                        __syncthreads();
                        rd_walk<T>(s_bin, nbin, px, py, best, col, &cov);
                        __syncthreads();
                        nbin = 0;
                    }
                    // the record as four 16-byte words: q2 = X0 X1 X2 Y0, q3 = Y1 Y2 colour live
                    uint4 q0 = {0, 0, 0, 0}, q1 = q0, q2 = q0, q3 = q0;
                    bool keep = false;
                    if (tb + t < ntris) {
                        const uint4* g = (const uint4*)(tr + tb + t);
                        q0 = g[0], q1 = g[1], q2 = g[2], q3 = g[3];
                        const int X0 = (int)q2.x, X1 = (int)q2.y, X2 = (int)q2.z, Y0 = (int)q2.w, Y1 = (int)q3.x, Y2 = (int)q3.y;
                        keep = q3.w != 0u && min(min(X0, X1), X2) <= 16 * tx1 && max(max(X0, X1), X2) >= 16 * tx0 && min(min(Y0, Y1), Y2) <= 16 * ty1 &&
                               max(max(Y0, Y1), Y2) >= 16 * ty0;
                    }
                    // compaction keeps instance order, then triangle order. s_wcnt alternates between two sets: a wave that runs ahead
                    // writes the other set, and cannot reach this one again before every wave has passed the next barrier
                    const uint64_t kb = __ballot(keep);
                    if (lane == 0) s_wcnt[par][wave] = __popcll(kb);
                    __syncthreads();
                    const int c0 = s_wcnt[par][0], c1 = s_wcnt[par][1], c2 = s_wcnt[par][2], c3 = s_wcnt[par][3];
                    const int before = (wave > 0 ? c0 : 0) + (wave > 1 ? c1 : 0) + (wave > 2 ? c2 : 0);
                    if (keep) {
                        uint4* d = (uint4*)(s_bin + nbin + before + __popcll(kb & ((1ull << lane) - 1ull)));
                        d[0] = q0, d[1] = q1, d[2] = q2, d[3] = q3;
                    }
                    nbin += c0 + c1 + c2 + c3, par ^= 1;
                }
            }
        }
        __syncthreads();   // every wave has read s_mask before the next 256 slots replace it
    }
    if (nbin) {
        __syncthreads();
        rd_walk<T>(s_bin, nbin, px, py, best, col, &cov);
    }
    if (!cov || py >= H) return;
    if (masks) {
        const uint8_t* mk = masks + (size_t)blockIdx.z * mask_frame + (size_t)py * mask_row + px;
#pragma unroll
        for (int j = 0; j < RD_PX; j++)
            if ((cov >> j & 1u) && px + j < W && mk[j] == 0) cov &= ~(1u << j);
    }
    if (opacity == 0) cov = 0;   // out = frame: nothing to write
    if (!cov) return;
    uint8_t* q = frames + (size_t)blockIdx.z * frame_stride + (size_t)py * row_stride + (size_t)px * CH;
    const uint32_t op = (uint32_t)opacity;
    if (px + RD_PX <= W && ((uintptr_t)q & 3u) == 0) {
        // the lane's own 4 * CH bytes as whole dwords: read, patch the painted pixels, write once
        constexpr int ND = RD_PX * CH / 4;
        uint32_t v[ND];
        uint32_t* q4 = (uint32_t*)q;
#pragma unroll
        for (int d = 0; d < ND; d++) v[d] = (cov == 15u && op == 255u) ? 0u : q4[d];
        uint8_t* b = (uint8_t*)v;
#pragma unroll
        for (int j = 0; j < RD_PX; j++)
            if (cov >> j & 1u)
                for (int c = 0; c < CH; c++) {
                    const uint32_t C = CH == 1 ? col[j] >> 24 : (col[j] >> (8 * c) & 255u);
                    b[j * CH + c] = (uint8_t)((C * op + (uint32_t)b[j * CH + c] * (255u - op) + 127u) / 255u);
                }
#pragma unroll
        for (int d = 0; d < ND; d++) q4[d] = v[d];
        return;
    }
    for (int j = 0; j < RD_PX; j++)
        if ((cov >> j & 1u) && px + j < W)
            for (int c = 0; c < CH; c++) {
                const uint32_t C = CH == 1 ? col[j] >> 24 : (col[j] >> (8 * c) & 255u);
                q[j * CH + c] = (uint8_t)((C * op + (uint32_t)q[j * CH + c] * (255u - op) + 127u) / 255u);
            }
}

void launch_render_instances_markers(hipStream_t s, const arucohip_marker_t* markers, const int32_t* counts, int nframes, int cap, double scale,
                                     void* insts) {
    const uint32_t n = (uint32_t)nframes * (uint32_t)cap;
    hipLaunchKernelGGL(render_instances_markers_kernel, dim3((n + 63) / 64), dim3(64), 0, s, markers, counts, nframes, cap, scale, (RdInst*)insts);
}

void launch_render_instances_boards(hipStream_t s, const arucohip_board_t* boards, int nframes, double scale, void* insts) {
    hipLaunchKernelGGL(render_instances_boards_kernel, dim3((nframes + 63) / 64), dim3(64), 0, s, boards, nframes, scale, (RdInst*)insts);
}

void launch_render_build(hipStream_t s, void* insts, int ninst, const CamModel& cam, const RdMesh& mesh, const RdStyle& style, void* verts, void* tris) {
    hipLaunchKernelGGL(render_vertices_kernel, dim3(ninst, (mesh.nverts + 255) / 256), dim3(256), 0, s, (const RdInst*)insts, cam, mesh.vertices,
                       mesh.nverts, (RdVert*)verts);
    hipLaunchKernelGGL(render_triangles_kernel, dim3(ninst, (mesh.ntris + 255) / 256), dim3(256), 0, s, (RdInst*)insts, mesh, style,
                       (const RdVert*)verts, (RdTri*)tris);
}

template <int CH, typename T>
static void rd_launch_raster(hipStream_t s, const dim3& grid, uint8_t* frames, int width, int height, size_t row_stride, size_t frame_stride,
                             const uint8_t* masks, size_t mask_row, size_t mask_frame, const void* insts, const void* tris, int slots, int ntris,
                             int opacity) {
    hipLaunchKernelGGL((render_raster_kernel<CH, T>), grid, dim3(256), 0, s, frames, width, height, row_stride, frame_stride, masks, mask_row,
                       mask_frame, (const RdInst*)insts, (const RdTri*)tris, slots, ntris, opacity);
}

void launch_render_raster(hipStream_t s, uint8_t* frames, int nframes, int width, int height, int channels, size_t row_stride, size_t frame_stride,
                          const uint8_t* masks, size_t mask_row, size_t mask_frame, const void* insts, const void* tris, int slots, int ntris,
                          const RdStyle& style) {
    const dim3 grid((width + RD_TW - 1) / RD_TW, (height + RD_TH - 1) / RD_TH, nframes);
    const bool i64 = (style.flags & ARUCOHIP_RENDER_EDGES_INT64) != 0;
#define RD_ARGS s, grid, frames, width, height, row_stride, frame_stride, masks, mask_row, mask_frame, insts, tris, slots, ntris, style.opacity
    if (channels == 3)
        i64 ? rd_launch_raster<3, int64_t>(RD_ARGS) : rd_launch_raster<3, double>(RD_ARGS);
    else
        i64 ? rd_launch_raster<1, int64_t>(RD_ARGS) : rd_launch_raster<1, double>(RD_ARGS);
#undef RD_ARGS
}

}  // namespace ah
