// Overlays: Marker::draw, CvDrawingUtils::draw3dAxis / draw3dCube (markers and boards) painted into frames that stay on the device
// (DESIGN.md "Overlay"). Two steps per call:
//   build   a lane per marker (per board) turns it into at most OV_SLOTS primitives - lines with a width, glyphs of the 5 x 7 font - in
//           painting order, and leaves the box that holds them all;
//   raster  one workgroup per 64 x 16 tile and frame GATHERS: it tests the frame's marker boxes against its tile, then the primitives of
//           the markers that are left, and every lane walks the survivors in order over its four pixels with the closed-form coverage
//           test. "The last primitive that covers a pixel wins" then needs no ordering between workgroups and no atomics: a pixel has one
//           owner. A tile that no box touches reads and writes no image byte.
#include <limits.h>

#include "internal.h"
#include "overlay_font.h"
#include "pnp_device.h"

namespace ah {

enum { OV_LINE = 1, OV_GLYPH = 2 };
constexpr float OV_LIMIT = 1048576.f;   // an endpoint beyond +-2^20 (or not finite) drops its primitive

// 32 bytes. OV_LINE: (x0, y0) - (x1, y1), w = width 1..7. OV_GLYPH: (x0, y0) = top-left pixel of the glyph, w = scale, bits = its 35 cells
// (bit 5 * row + 4 - column).
struct OvPrim {
    int32_t x0, y0, x1, y1;
    uint32_t color;   // B | G << 8 | R << 16
    uint32_t kind_w;  // kind | w << 8
    uint32_t bits_lo, bits_hi;
};
static_assert(sizeof(OvPrim) == 32, "OvPrim is two 16-byte words");
// one per marker slot: the inclusive box of every pixel its primitives can paint (x1 < x0: nothing), and how many there are
struct OvRec {
    int32_t x0, y0, x1, y1, count, pad_[3];
};
static_assert(sizeof(OvRec) == OV_REC_BYTES && sizeof(OvPrim) * OV_SLOTS == OV_PRIM_BYTES, "scratch layout (internal.h)");

struct OvPt {
    int x, y;
    bool ok;
};

__device__ inline bool ov_ok(float v) { return fabsf(v) <= OV_LIMIT; }   // false for NaN and infinities
// Point2f -> cv::Point: cvRound, ties to even
__device__ inline OvPt ov_round(float x, float y) { return {__float2int_rn(x), __float2int_rn(y), true}; }
__device__ inline OvPt ov_point(float x, float y) {
    if (!(ov_ok(x) && ov_ok(y))) return {0, 0, false};
    return ov_round(x, y);
}

struct OvEmit {
    OvPrim* out;
    int n, bx0, by0, bx1, by1;
    __device__ void grow(int x0, int y0, int x1, int y1) { bx0 = min(bx0, x0), by0 = min(by0, y0), bx1 = max(bx1, x1), by1 = max(by1, y1); }
    __device__ void line(OvPt a, OvPt b, uint32_t color, int w) {
        if (!(a.ok && b.ok) || n >= OV_SLOTS) return;
        out[n++] = {a.x, a.y, b.x, b.y, color, (uint32_t)OV_LINE | (uint32_t)w << 8, 0u, 0u};
        const int o = (w - 1) / 2;
        grow(min(a.x, b.x) - o, min(a.y, b.y) - o, max(a.x, b.x) - o + w - 1, max(a.y, b.y) - o + w - 1);
    }
    __device__ void rect(OvPt a, OvPt b, uint32_t color, int w) {
        const OvPt ab = {b.x, a.y, true}, ba = {a.x, b.y, true};
        line(a, ab, color, w), line(ab, b, color, w), line(b, ba, color, w), line(ba, a, color, w);
    }
    // glyph number k of a text anchored (bottom-left) at (ax, ay)
    __device__ void glyph(int ax, int ay, int k, int g, uint32_t color, int s) {
        if (n >= OV_SLOTS) return;
        uint64_t bits = 0;
        for (int r = 0; r < 7; r++) bits |= (uint64_t)(OVERLAY_FONT[g][r] & 31u) << (5 * r);
        const int x0 = ax + 6 * s * k, y0 = ay - 7 * s + 1;
        out[n++] = {x0, y0, 0, 0, color, (uint32_t)OV_GLYPH | (uint32_t)s << 8, (uint32_t)bits, (uint32_t)(bits >> 32)};
        grow(x0, y0, x0 + 5 * s - 1, y0 + 7 * s - 1);
    }
    __device__ void finish(OvRec* rec) const { *rec = {bx0, by0, bx1, by1, n, {0, 0, 0}}; }
};

// cv::projectPoints of one float object point, narrowed to Point2f and rounded. A point in the camera's plane (depth exactly 0) has no
// projection: it drops its primitives like a non-finite one.
__device__ inline OvPt ov_project(float X, float Y, float Z, const double* R, const double* t, const CamModel& cam) {
    const double z = R[6] * X + R[7] * Y + R[8] * Z + t[2];
    double mx, my;
    project_point(X, Y, Z, R, nullptr, t, cam.K, cam.k, &mx, &my, nullptr, nullptr);
    if (z == 0.) return {0, 0, false};
    return ov_point((float)mx, (float)my);
}

__device__ inline void ov_axis(OvEmit& e, const double* R, const double* t, const CamModel& cam, float len, int w, int scale, int first_glyph) {
    const uint32_t col[3] = {0xFF0000u, 0x00FF00u, 0x0000FFu};   // (0,0,255) (0,255,0) (255,0,0) as B G R
    const OvPt o = ov_project(0.f, 0.f, 0.f, R, t, cam);
    OvPt p[3];
    for (int i = 0; i < 3; i++) p[i] = ov_project(i == 0 ? len : 0.f, i == 1 ? len : 0.f, i == 2 ? len : 0.f, R, t, cam);
    for (int i = 0; i < 3; i++) e.line(o, p[i], col[i], w);
    for (int i = 0; i < 3; i++)
        if (p[i].ok) e.glyph(p[i].x, p[i].y, 0, first_glyph + i, col[i], scale);
}

__device__ inline void ov_cube_lines(OvEmit& e, const OvPt* p) {
    for (int i = 0; i < 4; i++) e.line(p[i], p[(i + 1) % 4], 0xFF0000u, 1);
    for (int i = 0; i < 4; i++) e.line(p[i + 4], p[4 + (i + 1) % 4], 0xFF0000u, 1);
    for (int i = 0; i < 4; i++) e.line(p[i], p[i + 4], 0xFF0000u, 1);
}

// the primitives of one marker: Marker::draw (marker.cpp:54-81), then draw3dAxis, then draw3dCube (cvdrawingutils.cpp:41-144)
__device__ inline void ov_marker(OvEmit& e, const arucohip_marker_t& m, const CamModel& cam, int flags, int lw, uint32_t color) {
    OvPt c[4];
    for (int i = 0; i < 4; i++) c[i] = ov_point(m.corners[2 * i], m.corners[2 * i + 1]);
    if (flags & ARUCOHIP_DRAW_OUTLINE) {
        for (int i = 0; i < 4; i++) e.line(c[i], c[(i + 1) % 4], color, lw);
        const uint32_t col[3] = {0xFF0000u, 0x00FF00u, 0x0000FFu};
        for (int i = 0; i < 3; i++) {
            const OvPt a = ov_point(m.corners[2 * i] - 2.f, m.corners[2 * i + 1] - 2.f), b = ov_point(m.corners[2 * i] + 2.f, m.corners[2 * i + 1] + 2.f);
            if (a.ok && b.ok) e.rect(a, b, col[i], lw);
        }
    }
    if ((flags & ARUCOHIP_DRAW_IDS) && c[0].ok && c[1].ok && c[2].ok && c[3].ok) {
        // Point cent(0, 0); cent.x += corner.x: an int accumulator, truncated after every float addition; then cent.x /= 4.
        int cx = 0, cy = 0;
        for (int i = 0; i < 4; i++) cx = (int)((float)cx + m.corners[2 * i]), cy = (int)((float)cy + m.corners[2 * i + 1]);
        cx = (int)((double)cx / 4.), cy = (int)((double)cy / 4.);
        const uint32_t inv = ~color & 0xFFFFFFu;
        int k = 0;
        e.glyph(cx, cy, k++, 10, inv, 2), e.glyph(cx, cy, k++, 11, inv, 2), e.glyph(cx, cy, k++, 12, inv, 2);
        uint32_t mag = m.id < 0 ? 0u - (uint32_t)m.id : (uint32_t)m.id;
        if (m.id < 0) e.glyph(cx, cy, k++, 19, inv, 2);
        uint32_t div = 1;
        while (mag / div >= 10) div *= 10;
        for (; div; div /= 10) e.glyph(cx, cy, k++, (int)(mag / div % 10), inv, 2);
    }
    if (!m.has_pose || !(flags & (ARUCOHIP_DRAW_AXIS | ARUCOHIP_DRAW_CUBE))) return;
    double R[9];
    rodrigues_vec2mat(m.rvec, R, nullptr);
    if (flags & ARUCOHIP_DRAW_AXIS) ov_axis(e, R, m.tvec, cam, m.ssize * 3.f, 1, 2, 13);
    if (flags & ARUCOHIP_DRAW_CUBE) {
        const float hs = (float)(double)(m.ssize / 2.f), s = m.ssize;
        OvPt p[8];
        for (int i = 0; i < 8; i++) {
            const float a = (i & 3) == 0 || (i & 3) == 3 ? -hs : hs, b = (i & 3) < 2 ? -hs : hs, up = i < 4 ? 0.f : s;
            p[i] = (flags & ARUCOHIP_DRAW_Y_PERPENDICULAR) ? ov_project(a, up, b, R, m.tvec, cam) : ov_project(a, b, up, R, m.tvec, cam);
        }
        ov_cube_lines(e, p);
    }
}

// the primitives of one board: draw3dAxis, then draw3dCube (cvdrawingutils.cpp:151-255)
__device__ inline void ov_board(OvEmit& e, const arucohip_board_t& b, const CamModel& cam, int flags, float size) {
    if (!b.has_pose) return;
    double R[9];
    rodrigues_vec2mat(b.rvec, R, nullptr);
    if (flags & ARUCOHIP_DRAW_AXIS) ov_axis(e, R, b.tvec, cam, 2.f * size, 2, 3, 16);
    if (flags & ARUCOHIP_DRAW_CUBE) {
        const float t0 = -size / 2.f, t1 = t0 + size;
        OvPt p[8];
        for (int i = 0; i < 8; i++) {
            const float x = (i & 3) == 0 || (i & 3) == 3 ? t0 : t1;
            if (flags & ARUCOHIP_DRAW_Y_PERPENDICULAR)
                p[i] = ov_project(x, (i & 3) < 2 ? 0.f : size, i < 4 ? t0 : t1, R, b.tvec, cam);
            else
                p[i] = ov_project(x, i < 4 ? t0 : t1, (i & 3) < 2 ? 0.f : -size, R, b.tvec, cam);
        }
        ov_cube_lines(e, p);
    }
}

// lane = slot `gid` of the chunk's nframes * cap slots. A frame whose count is negative (given up) or zero leaves empty boxes.
__global__ __launch_bounds__(64) void overlay_build_markers_kernel(const arucohip_marker_t* markers, const int32_t* counts, int nframes, int cap,
                                                                   CamModel cam, int flags, int lw, uint32_t color, OvRec* recs, OvPrim* prims) {
    const uint32_t gid = blockIdx.x * 64u + threadIdx.x;
    if (gid >= (uint32_t)nframes * (uint32_t)cap) return;
    const int f = (int)(gid / (uint32_t)cap), i = (int)(gid % (uint32_t)cap);
    OvEmit e = {prims + (size_t)gid * OV_SLOTS, 0, INT_MAX, INT_MAX, INT_MIN, INT_MIN};
    if (i < min(counts[f], cap)) ov_marker(e, markers[gid], cam, flags, lw, color);
    e.finish(recs + gid);
}

__global__ __launch_bounds__(64) void overlay_build_boards_kernel(const arucohip_board_t* boards, int nframes, CamModel cam, int flags, float size,
                                                                  OvRec* recs, OvPrim* prims) {
    const uint32_t gid = blockIdx.x * 64u + threadIdx.x;
    if (gid >= (uint32_t)nframes) return;
    OvEmit e = {prims + (size_t)gid * OV_SLOTS, 0, INT_MAX, INT_MAX, INT_MIN, INT_MIN};
    ov_board(e, boards[gid], cam, flags, size);
    e.finish(recs + gid);
}

// ---- coverage. A line from (x0, y0) to (x1, y1): n = max(|dx|, |dy|), pixel i = 0..n advances the major coordinate (x when |dx| >= |dy|)
// by one and has minor = minor0 + sign(dminor) * floor((2 i |dminor| + n) / (2n)). Width w stamps a w x w square whose top-left is
// (w - 1) / 2 left of and above each of these pixels: pixel q is painted when some line pixel lies in [q + o - w + 1, q + o] on both axes.
struct OvLine {
    int M0, m0, sM, sm, n;
    uint32_t adm;
    bool xmajor;
};
__device__ inline OvLine ov_line_setup(const OvPrim& p) {
    const int dx = p.x1 - p.x0, dy = p.y1 - p.y0, adx = abs(dx), ady = abs(dy);
    OvLine l;
    l.xmajor = adx >= ady;
    l.n = l.xmajor ? adx : ady;
    l.M0 = l.xmajor ? p.x0 : p.y0, l.m0 = l.xmajor ? p.y0 : p.x0;
    const int dM = l.xmajor ? dx : dy, dm = l.xmajor ? dy : dx;
    l.sM = dM < 0 ? -1 : 1, l.sm = dm < 0 ? -1 : 1, l.adm = (uint32_t)abs(dm);
    return l;
}
__device__ inline int ov_minor(const OvLine& l, int i) {
    if (l.n == 0) return l.m0;
    // endpoints lie within +-2^20: n, |dminor| <= 2^21. Below 2^15 the numerator fits 32 bits
    const uint32_t n = (uint32_t)l.n;
    const int step = n < 32768u ? (int)((2u * (uint32_t)i * l.adm + n) / (2u * n)) : (int)((2ull * (uint32_t)i * l.adm + n) / (2ull * n));
    return l.m0 + l.sm * step;
}
// the pixels i of the line whose major coordinate lies in [lo, hi]
__device__ inline void ov_range(const OvLine& l, int lo, int hi, int* i0, int* i1) {
    *i0 = max(l.sM > 0 ? lo - l.M0 : l.M0 - hi, 0);
    *i1 = min(l.sM > 0 ? hi - l.M0 : l.M0 - lo, l.n);
}
// may the line paint a pixel of [x0, x1] x [y0, y1]? Exact on the major axis; on the minor one the range between the ends of the clipped
// run (the minor coordinate is monotonic in i)
__device__ inline bool ov_line_hits(const OvPrim& p, int x0, int y0, int x1, int y1) {
    const OvLine l = ov_line_setup(p);
    const int w = (int)(p.kind_w >> 8), o = (w - 1) / 2;
    const int Mlo = (l.xmajor ? x0 : y0) + o - w + 1, Mhi = (l.xmajor ? x1 : y1) + o;
    const int mlo = (l.xmajor ? y0 : x0) + o - w + 1, mhi = (l.xmajor ? y1 : x1) + o;
    int i0, i1;
    ov_range(l, Mlo, Mhi, &i0, &i1);
    if (i0 > i1) return false;
    const int a = ov_minor(l, i0), b = ov_minor(l, i1);
    return max(a, b) >= mlo && min(a, b) <= mhi;
}
__device__ inline bool ov_glyph_hits(const OvPrim& p, int x0, int y0, int x1, int y1) {
    const int s = (int)(p.kind_w >> 8);
    return p.x0 <= x1 && p.x0 + 5 * s - 1 >= x0 && p.y0 <= y1 && p.y0 + 7 * s - 1 >= y0;
}

constexpr int OV_TW = 64, OV_TH = 16, OV_PX = 4;   // tile: 64 x 16 pixels (a row = 192 bytes = three 64-byte pieces at 3 channels); 4 pixels a lane

template <int CH>
__global__ __launch_bounds__(256) void overlay_raster_kernel(uint8_t* frames, int W, int H, size_t row_stride, size_t frame_stride, const OvRec* recs,
                                                             const OvPrim* prims, int cap) {
    __shared__ uint64_t s_mask[4];
    __shared__ OvPrim s_surv[OV_SLOTS];
    __shared__ int s_n;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int tx0 = blockIdx.x * OV_TW, ty0 = blockIdx.y * OV_TH, tx1 = min(tx0 + OV_TW, W) - 1, ty1 = min(ty0 + OV_TH, H) - 1;
    const size_t slot0 = (size_t)blockIdx.z * cap;
    const int px = tx0 + (t % (OV_TW / OV_PX)) * OV_PX, py = ty0 + t / (OV_TW / OV_PX);
    uint32_t col[OV_PX] = {0, 0, 0, 0}, cov = 0;
    for (int base = 0; base < cap; base += 256) {
        bool hit = false;
        if (base + t < cap) {
            const OvRec r = recs[slot0 + base + t];
            hit = r.count > 0 && r.x0 <= tx1 && r.x1 >= tx0 && r.y0 <= ty1 && r.y1 >= ty0;
        }
        const uint64_t bal = __ballot(hit);
        if (lane == 0) s_mask[wave] = bal;
        __syncthreads();
        for (int w4 = 0; w4 < 4; w4++) {
            uint64_t mask = s_mask[w4];   // the same in every lane: the loop and its barriers are uniform
            while (mask) {
                const int mi = base + w4 * 64 + __builtin_ctzll(mask);
                mask &= mask - 1;
                // the first wave culls the marker's primitives against the tile; the ballot keeps their order
                if (wave == 0) {
                    const int cnt = min(recs[slot0 + mi].count, OV_SLOTS);
                    bool keep = false;
                    OvPrim p;
                    if (lane < cnt) {
                        p = prims[(slot0 + mi) * OV_SLOTS + lane];
                        keep = (p.kind_w & 255u) == OV_LINE ? ov_line_hits(p, tx0, ty0, tx1, ty1) : ov_glyph_hits(p, tx0, ty0, tx1, ty1);
                    }
                    const uint64_t kb = __ballot(keep);
                    if (keep) s_surv[__popcll(kb & ((1ull << lane) - 1ull))] = p;
                    if (lane == 0) s_n = __popcll(kb);
                }
                __syncthreads();
                const int ns = s_n;
                for (int k = 0; k < ns; k++) {
                    const OvPrim p = s_surv[k];
                    const int w = (int)(p.kind_w >> 8);
                    if ((p.kind_w & 255u) == OV_LINE) {
                        const OvLine l = ov_line_setup(p);
                        const int o = (w - 1) / 2;
#pragma unroll
                        for (int j = 0; j < OV_PX; j++) {
                            const int qM = l.xmajor ? px + j : py, qm = l.xmajor ? py : px + j;
                            int i0, i1;
                            ov_range(l, qM + o - w + 1, qM + o, &i0, &i1);
                            bool in = false;
                            for (int i = i0; i <= i1; i++) {   // at most w pixels of the line
                                const int mn = ov_minor(l, i);
                                in = in || (mn >= qm + o - w + 1 && mn <= qm + o);
                            }
                            if (in) col[j] = p.color, cov |= 1u << j;
                        }
                    } else {
                        const uint64_t bits = (uint64_t)p.bits_hi << 32 | p.bits_lo;
                        const int cy = py - p.y0;
                        if (cy >= 0 && cy < 7 * w) {
                            const int r = cy / w;
#pragma unroll
                            for (int j = 0; j < OV_PX; j++) {
                                const int cx = px + j - p.x0;
                                if (cx >= 0 && cx < 5 * w && (bits >> (5 * r + 4 - cx / w) & 1ull)) col[j] = p.color, cov |= 1u << j;
                            }
                        }
                    }
                }
                __syncthreads();
            }
        }
        __syncthreads();
    }
    if (!cov || py >= H) return;
    uint8_t* q = frames + (size_t)blockIdx.z * frame_stride + (size_t)py * row_stride + (size_t)px * CH;
    if (px + OV_PX <= W && ((uintptr_t)q & 3u) == 0) {
        // the lane's own 4 * CH bytes as whole dwords: read, patch the painted pixels, write once
        constexpr int ND = OV_PX * CH / 4;
        uint32_t v[ND];
        uint32_t* q4 = (uint32_t*)q;
#pragma unroll
        for (int d = 0; d < ND; d++) v[d] = cov == 15u ? 0u : q4[d];
        uint8_t* b = (uint8_t*)v;
#pragma unroll
        for (int j = 0; j < OV_PX; j++)
            if (cov >> j & 1u)
                for (int c = 0; c < CH; c++) b[j * CH + c] = (uint8_t)(col[j] >> (8 * c));
#pragma unroll
        for (int d = 0; d < ND; d++) q4[d] = v[d];
        return;
    }
    for (int j = 0; j < OV_PX; j++)
        if ((cov >> j & 1u) && px + j < W)
            for (int c = 0; c < CH; c++) q[j * CH + c] = (uint8_t)(col[j] >> (8 * c));
}

void launch_overlay_build_markers(hipStream_t s, const arucohip_marker_t* markers, const int32_t* counts, int nframes, int cap, const CamModel& cam,
                                  int flags, int line_width, uint32_t color, void* recs, void* prims) {
    const uint32_t n = (uint32_t)nframes * (uint32_t)cap;
    hipLaunchKernelGGL(overlay_build_markers_kernel, dim3((n + 63) / 64), dim3(64), 0, s, markers, counts, nframes, cap, cam, flags, line_width, color,
                       (OvRec*)recs, (OvPrim*)prims);
}

void launch_overlay_build_boards(hipStream_t s, const arucohip_board_t* boards, int nframes, const CamModel& cam, int flags, float marker_size, void* recs,
                                 void* prims) {
    hipLaunchKernelGGL(overlay_build_boards_kernel, dim3((nframes + 63) / 64), dim3(64), 0, s, boards, nframes, cam, flags, marker_size, (OvRec*)recs,
                       (OvPrim*)prims);
}

void launch_overlay_raster(hipStream_t s, uint8_t* frames, int nframes, int width, int height, int channels, size_t row_stride, size_t frame_stride,
                           const void* recs, const void* prims, int cap) {
    const dim3 grid((width + OV_TW - 1) / OV_TW, (height + OV_TH - 1) / OV_TH, nframes);
    if (channels == 3)
        hipLaunchKernelGGL(overlay_raster_kernel<3>, grid, dim3(256), 0, s, frames, width, height, row_stride, frame_stride, (const OvRec*)recs,
                           (const OvPrim*)prims, cap);
    else
        hipLaunchKernelGGL(overlay_raster_kernel<1>, grid, dim3(256), 0, s, frames, width, height, row_stride, frame_stride, (const OvRec*)recs,
                           (const OvPrim*)prims, cap);
}

}  // namespace ah
