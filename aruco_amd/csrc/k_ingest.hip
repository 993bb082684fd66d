// Camera-native input (include/arucohip.h, "Camera-native input"): frames as cameras and decoders deliver them, turned into the 8-bit grey
// image the pipeline reads or into interleaved B,G,R. No reference counterpart: MarkerDetector::detect takes what cv::VideoCapture hands it.
//
// Streaming kernels of bgr2gray_kernel's shape (k_convert.hip): a lane turns 4 pixels of one row, block y is row y, block z the frame.
// A quad whose source dwords and destination dwords are whole and aligned is read with dword loads and written with one (grey) or three
// (B,G,R) dword stores; any other quad (unaligned base, stride or chroma offset, the last pixels of a row) goes byte by byte. Both paths
// fill the same little-endian words, so every definition below is written once, on words, and grey and B,G,R outputs share it.
// The Bayer kernel reads rows y-1, y, y+1: the lane's own three dwords plus the two columns beside them; the columns are the neighbour
// lanes' dwords (same cache lines, L1) and the rows are the neighbour rows' own reads (L2 / Infinity Cache), not further HBM traffic.
// Two instances restate work that exists elsewhere, on purpose, so that every format has the same strided destination: PACKED3 to grey
// with B first is bgr2gray_kernel's arithmetic (k_convert.hip; both call gray_of of convert_device.h), and GRAY8 / NV12 to grey is a 2-D
// copy. A change to one of a pair belongs in the other as well.
#include "convert_device.h"   // gray_of, ld32, byte_of, sat8
#include "internal.h"

namespace ah {

struct IngestArgs {
    const uint8_t* src;
    size_t row_stride, frame_stride, chroma_offset;
    uint8_t* dst;
    size_t drs, dfs;
    int width, height;
    int p0, p1;   // PACKED: p0 = 1 when the first byte is R; GRAY16: p0 = bits - 8; YUV422: p0 = byte of Y0 (0 YUYV, 1 UYVY); BAYER: parity of the red site (x, y)
    int fast;
};

enum IngestKind { IK_PACKED3 = 0, IK_PACKED4, IK_GRAY8, IK_GRAY16, IK_YUV422, IK_NV12, IK_BAYER };

// BT.601 video range in 20-bit fixed point: round(1.164, 1.596, 0.813, 0.391, 2.018 * 2^20); >> of a negative sum is the floor shift
__device__ __forceinline__ void yuv_to_bgr(int Y, int U, int V, uint32_t* b, uint32_t* g, uint32_t* r) {
    const int y = max(0, Y - 16) * 1220542, u = U - 128, v = V - 128;
    *r = sat8((y + 1673527 * v + 524288) >> 20);
    *g = sat8((y - 852492 * v - 409993 * u + 524288) >> 20);
    *b = sat8((y + 2116026 * u + 524288) >> 20);
}

// Bilinear demosaic of the site (x, y) from its 3 x 3 neighbourhood (already reflected at the borders); the mosaic's red sites are those with
// (x & 1, y & 1) = (red_x, red_y), the blue ones the opposite corner of the 2 x 2 block
__device__ __forceinline__ void bayer_bgr_at(int red_x, int red_y, int x, int y, uint32_t nw, uint32_t n, uint32_t ne, uint32_t w, uint32_t c, uint32_t e,
                                             uint32_t sw, uint32_t s, uint32_t se, uint32_t* b, uint32_t* g, uint32_t* r) {
    const bool red_row = (y & 1) == red_y, red_col = (x & 1) == red_x;
    if (red_row == red_col) {   // a red or a blue site
        const uint32_t cross = (n + s + e + w + 2) >> 2, diag = (nw + ne + sw + se + 2) >> 2;
        *g = cross;
        if (red_row) *r = c, *b = diag; else *b = c, *r = diag;
    } else {   // a green site: the row's other sites left and right, the column's above and below
        const uint32_t hor = (w + e + 1) >> 1, ver = (n + s + 1) >> 1;
        *g = c;
        if (red_row) *r = hor, *b = ver; else *b = hor, *r = ver;
    }
}

// Pixels x .. x + 3 of row y of the frame at sf (n of them exist). C = 3: b, g, r; C = 1: the grey value in b.
template <int KIND, int C>
__device__ __forceinline__ void quad_of(const IngestArgs& a, const uint8_t* sf, int x, int y, int n, bool whole, uint32_t* b, uint32_t* g, uint32_t* r) {
    const uint8_t* row = sf + (size_t)y * a.row_stride;
    if (KIND == IK_PACKED3 || KIND == IK_PACKED4) {
        constexpr int BPP = KIND == IK_PACKED3 ? 3 : 4;
        uint32_t w[BPP];
#pragma unroll
        for (int k = 0; k < BPP; k++) w[k] = ld32(row + (size_t)x * BPP + 4 * k, n * BPP - 4 * k, whole);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t c0 = byte_of(w, BPP * j), c1 = byte_of(w, BPP * j + 1), c2 = byte_of(w, BPP * j + 2);
            const uint32_t bb = a.p0 ? c2 : c0, rr = a.p0 ? c0 : c2;
            if (C == 1) b[j] = gray_of(bb, c1, rr); else b[j] = bb, g[j] = c1, r[j] = rr;
        }
    } else if (KIND == IK_GRAY8) {
        const uint32_t w = ld32(row + x, n, whole);
#pragma unroll
        for (int j = 0; j < 4; j++) b[j] = g[j] = r[j] = byte_of(&w, j);
    } else if (KIND == IK_GRAY16) {
        uint32_t w[2];
        w[0] = ld32(row + (size_t)x * 2, 2 * n, whole), w[1] = ld32(row + (size_t)x * 2 + 4, 2 * n - 4, whole);
#pragma unroll
        for (int j = 0; j < 4; j++) b[j] = g[j] = r[j] = min(((w[j >> 1] >> (16 * (j & 1))) & 0xFFFFu) >> a.p0, 255u);
    } else if (KIND == IK_YUV422) {
        uint32_t w[2];
        w[0] = ld32(row + (size_t)x * 2, 2 * n, whole), w[1] = ld32(row + (size_t)x * 2 + 4, 2 * n - 4, whole);
        const int ys = 8 * a.p0, us = 8 * (1 - a.p0), vs = 8 * (3 - a.p0);   // bit positions of Y0, U, V in a pair's word; Y1 is 16 above Y0
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const uint32_t y0 = (w[k] >> ys) & 0xFFu, y1 = (w[k] >> (ys + 16)) & 0xFFu;
            if (C == 1) {
                b[2 * k] = y0, b[2 * k + 1] = y1;
            } else {
                const int u = (w[k] >> us) & 0xFFu, v = (w[k] >> vs) & 0xFFu;
                yuv_to_bgr((int)y0, u, v, &b[2 * k], &g[2 * k], &r[2 * k]);
                yuv_to_bgr((int)y1, u, v, &b[2 * k + 1], &g[2 * k + 1], &r[2 * k + 1]);
            }
        }
    } else if (KIND == IK_NV12) {
        const uint32_t wy = ld32(row + x, n, whole);
        if (C == 1) {
#pragma unroll
            for (int j = 0; j < 4; j++) b[j] = byte_of(&wy, j);
        } else {
            const uint32_t wc = ld32(sf + a.chroma_offset + (size_t)(y >> 1) * a.row_stride + x, n, whole);   // U V of (x, x+1), U V of (x+2, x+3)
#pragma unroll
            for (int j = 0; j < 4; j++)
                yuv_to_bgr((int)byte_of(&wy, j), (int)byte_of(&wc, j & 2), (int)byte_of(&wc, (j & 2) + 1), &b[j], &g[j], &r[j]);
        }
    } else {   // IK_BAYER
        const int W = a.width, H = a.height;
        const int ym = y == 0 ? 1 : y - 1, yp = y == H - 1 ? H - 2 : y + 1;   // reflect-101; H >= 2
        const int xl = x == 0 ? 1 : x - 1;                                    // W >= 2
        const int xr = x + n == W ? W - 2 : x + n;                            // the column right of the quad's last pixel (n < 4 only in the row's last quad)
        const uint8_t* rows[3] = {sf + (size_t)ym * a.row_stride, row, sf + (size_t)yp * a.row_stride};
        uint32_t t[3][6];   // columns x - 1 .. x + 4 of the three rows
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const uint32_t w = ld32(rows[i] + x, n, whole);
            t[i][0] = rows[i][xl], t[i][5] = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) t[i][j + 1] = byte_of(&w, j);
            const uint32_t right = rows[i][xr];
            // right of pixel j is pixel j + 1, except for the quad's last pixel
#pragma unroll
            for (int j = 1; j <= 4; j++)
                if (j == n) t[i][j + 1] = right;
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            uint32_t bb, gg, rr;
            bayer_bgr_at(a.p0, a.p1, x + j, y, t[0][j], t[0][j + 1], t[0][j + 2], t[1][j], t[1][j + 1], t[1][j + 2], t[2][j], t[2][j + 1], t[2][j + 2], &bb, &gg, &rr);
            if (C == 1) b[j] = gray_of(bb, gg, rr); else b[j] = bb, g[j] = gg, r[j] = rr;
        }
    }
}

template <int KIND, int C>
__global__ __launch_bounds__(256) void ingest_kernel(IngestArgs a) {
    const int frame = blockIdx.z, y = blockIdx.y;
    const uint8_t* sf = a.src + (size_t)frame * a.frame_stride;
    uint8_t* drow = a.dst + (size_t)frame * a.dfs + (size_t)y * a.drs;
    const int quads = (a.width + 3) / 4;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += gridDim.x * blockDim.x) {
        const int x = 4 * q, n = min(4, a.width - x);
        const bool whole = a.fast && n == 4;   // source and destination start on dword boundaries and the quad is complete
        uint32_t b[4], g[4], r[4];
        quad_of<KIND, C>(a, sf, x, y, n, whole, b, g, r);
        if (C == 1) {
            if (whole) {
                *(uint32_t*)(drow + x) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
            } else {
                for (int j = 0; j < n; j++) drow[x + j] = (uint8_t)b[j];
            }
        } else {
            uint8_t* d = drow + (size_t)x * 3;
            if (whole) {
                uint32_t* dw = (uint32_t*)d;   // B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
                dw[0] = b[0] | (g[0] << 8) | (r[0] << 16) | (b[1] << 24);
                dw[1] = g[1] | (r[1] << 8) | (b[2] << 16) | (g[2] << 24);
                dw[2] = r[2] | (b[3] << 8) | (g[3] << 16) | (r[3] << 24);
            } else {
                for (int j = 0; j < n; j++) d[3 * j] = (uint8_t)b[j], d[3 * j + 1] = (uint8_t)g[j], d[3 * j + 2] = (uint8_t)r[j];
            }
        }
    }
}

template <int KIND>
static void launch_kind(hipStream_t s, const IngestArgs& a, int nframes, int C) {
    const int quads = (a.width + 3) / 4;
    dim3 grid((quads + 255) / 256, a.height, nframes);
    if (C == 1)
        hipLaunchKernelGGL((ingest_kernel<KIND, 1>), grid, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((ingest_kernel<KIND, 3>), grid, dim3(256), 0, s, a);
}

// the caller has validated fmt and the geometry (capi_ingest.hip: check_frame_format)
void launch_ingest(hipStream_t s, const FrameFmt& fmt, const uint8_t* src, size_t row_stride, size_t frame_stride, int width, int height, int nframes,
                   int dst_channels, uint8_t* dst, size_t dst_row_stride, size_t dst_frame_stride) {
    IngestArgs a{};
    a.src = src, a.row_stride = row_stride, a.frame_stride = frame_stride;
    a.chroma_offset = fmt.chroma_offset ? fmt.chroma_offset : row_stride * (size_t)height;
    a.dst = dst, a.drs = dst_row_stride, a.dfs = dst_frame_stride, a.width = width, a.height = height;
    // what decides the dword path: only strides and offsets the kernel uses (one frame: no frame stride; chroma only for NV12 in colour)
    size_t align = (uintptr_t)src | row_stride | (uintptr_t)dst | dst_row_stride;
    if (nframes > 1) align |= frame_stride | dst_frame_stride;
    if (fmt.format == ARUCOHIP_PIX_NV12 && dst_channels == 3) align |= a.chroma_offset;
    a.fast = (align & 3) == 0;
    switch (fmt.format) {
        case ARUCOHIP_PIX_GRAY8: launch_kind<IK_GRAY8>(s, a, nframes, dst_channels); break;
        case ARUCOHIP_PIX_BGR8: launch_kind<IK_PACKED3>(s, a, nframes, dst_channels); break;
        case ARUCOHIP_PIX_RGB8: a.p0 = 1; launch_kind<IK_PACKED3>(s, a, nframes, dst_channels); break;
        case ARUCOHIP_PIX_BGRA8: launch_kind<IK_PACKED4>(s, a, nframes, dst_channels); break;
        case ARUCOHIP_PIX_RGBA8: a.p0 = 1; launch_kind<IK_PACKED4>(s, a, nframes, dst_channels); break;
        case ARUCOHIP_PIX_GRAY16: a.p0 = fmt.bits - 8; launch_kind<IK_GRAY16>(s, a, nframes, dst_channels); break;
        case ARUCOHIP_PIX_YUYV: launch_kind<IK_YUV422>(s, a, nframes, dst_channels); break;
        case ARUCOHIP_PIX_UYVY: a.p0 = 1; launch_kind<IK_YUV422>(s, a, nframes, dst_channels); break;
        case ARUCOHIP_PIX_NV12: launch_kind<IK_NV12>(s, a, nframes, dst_channels); break;
        case ARUCOHIP_PIX_BAYER_RGGB: a.p0 = 0, a.p1 = 0; launch_kind<IK_BAYER>(s, a, nframes, dst_channels); break;
        case ARUCOHIP_PIX_BAYER_BGGR: a.p0 = 1, a.p1 = 1; launch_kind<IK_BAYER>(s, a, nframes, dst_channels); break;
        case ARUCOHIP_PIX_BAYER_GRBG: a.p0 = 1, a.p1 = 0; launch_kind<IK_BAYER>(s, a, nframes, dst_channels); break;
        case ARUCOHIP_PIX_BAYER_GBRG: a.p0 = 0, a.p1 = 1; launch_kind<IK_BAYER>(s, a, nframes, dst_channels); break;
        default: break;
    }
}

}  // namespace ah
