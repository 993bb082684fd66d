// Plane rectification: the fronto-parallel view of a board's plane, resampled from every frame with a map of its own. No reference
// counterpart; with an identity camera it is cv::warpPerspective(src, dst, M, size, INTER_LINEAR | WARP_INVERSE_MAP, BORDER_CONSTANT 0)
// up to OpenCV's own blocking (it interpolates the position inside blocks; here every pixel is projected).
//
// The rule for output pixel (u, v) of a frame with map M (row-major, double), in this order and in double, unfused (-ffp-contract=off):
//   X = (M0 u + M1 v) + M2, Y = (M3 u + M4 v) + M5, W = (M6 u + M7 v) + M8; !(W > 0): 0
//   x = X / W, y = Y / W; the camera: undist_map_kernel's Brown model (k_undistort.hip), or px = x, py = y without one
//   px or py not finite: 0
//   iu = rint_half_even(clamp(px * 32, -2^31, 2^31 - 1)), sx = iu >> 5, ax = iu & 31 (iv, sy, ay likewise); remap_bilinear at (sx, sy, ax, ay)
// tests/rectify_ref.py restates it in numpy.
#include "internal.h"
#include "plane_device.h"
#include "pnp_device.h"
#include "remap_device.h"

namespace ah {

// A wave covers 64 x 4 output pixels (16 lanes of 4 adjacent pixels by 4 rows), the four waves of a workgroup 64 x 16: the source
// footprint of a wave stays a compact patch, where a 256-pixel row segment would be a long thin line through the source.
constexpr int PW_TILE_W = 64, PW_TILE_H = 16;

// The fixed-point source position of output pixel (u, v); false: the pixel is 0. M and c are uniform (scalar registers).
template <bool DIST>
__device__ inline bool plane_position(const double* __restrict__ M, const PlaneWarp& c, int u, int v, int* iu, int* iv) {
    const double ud = (double)u, vd = (double)v;
    const double X = (M[0] * ud + M[1] * vd) + M[2], Y = (M[3] * ud + M[4] * vd) + M[5], Wd = (M[6] * ud + M[7] * vd) + M[8];
    if (!(Wd > 0)) return false;
    const double x = X / Wd, y = Y / Wd;
    double px, py;
    if (DIST) {
        const double k1 = c.k[0], k2 = c.k[1], p1 = c.k[2], p2 = c.k[3], k3 = c.k[4], k4 = c.k[5], k5 = c.k[6], k6 = c.k[7];
        const double x2 = x * x, y2 = y * y;
        const double r2 = x2 + y2, _2xy = 2 * x * y;
        const double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
        px = c.fx * (x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)) + c.cx;
        py = c.fy * (y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy) + c.cy;
    } else {
        // every coefficient 0: kr = 1 and both tangential terms are 0, so the polynomial's result is fx * x + cx bit for bit (where its
        // r2 overflows it gives NaN and this a position far outside the frame: 0 either way)
        px = c.fx * x + c.cx;
        py = c.fy * y + c.cy;
    }
    if (!isfinite(px) || !isfinite(py)) return false;
    *iu = __double2int_rn(fmax(-2147483648.0, fmin(2147483647.0, px * 32)));
    *iv = __double2int_rn(fmax(-2147483648.0, fmin(2147483647.0, py * 32)));
    return true;
}

template <bool DIST, int CN>
__global__ __launch_bounds__(256) void plane_warp_kernel(PlaneWarp a) {
    const int f = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = blockIdx.x * PW_TILE_W + (lane & 15) * 4, y = blockIdx.y * PW_TILE_H + wave * 4 + (lane >> 4);
    if (x0 >= a.out_width || y >= a.out_height) return;
    const int npx = min(4, a.out_width - x0);
    // the lane's 4 * CN bytes, packed as they lie in memory
    uint32_t word[CN];
#pragma unroll
    for (int k = 0; k < CN; k++) word[k] = 0;
    const bool live = !a.valid || a.valid[f] != 0;   // uniform: an invalid frame reads nothing
    if (live) {
        const double* __restrict__ M = a.maps + (size_t)f * 9;
        const uint8_t* src = a.src + (size_t)f * a.frame_stride;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            int iu, iv;
            if (i < npx && plane_position<DIST>(M, a, x0 + i, y, &iu, &iv)) {
#pragma unroll
                for (int c = 0; c < CN; c++) {
                    const int b = i * CN + c;
                    word[b >> 2] |= (uint32_t)remap_bilinear(src, a.row_stride, a.width, a.height, CN, iu >> 5, iv >> 5, iu & 31, iv & 31, c) << (8 * (b & 3));
                }
            }
        }
    }
    uint8_t* d = a.dst + (size_t)f * a.dst_frame_stride + (size_t)y * a.dst_row_stride + (size_t)x0 * CN;
    if (npx == 4 && ((uintptr_t)d & 3) == 0) {
#pragma unroll
        for (int k = 0; k < CN; k++) ((uint32_t*)d)[k] = word[k];
    } else {   // a row's tail, or a destination that is not dword aligned (odd base, odd stride, odd x0 * 3)
#pragma unroll
        for (int b = 0; b < 4 * CN; b++)
            if (b < npx * CN) d[b] = (uint8_t)(word[b >> 2] >> (8 * (b & 3)));
    }
}

// One lane per frame: M of plane_device.h, so that M (u, v, 1) is the camera-frame point of output pixel (u, v). A frame without a pose,
// or with an entry that is not finite, gets valid = 0 and a zero map.
__global__ __launch_bounds__(64) void plane_maps_kernel(const arucohip_board_t* boards, int nframes, arucohip_rectify_t win, double* maps, int32_t* valid) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nframes) return;
    const arucohip_board_t b = boards[f];
    double M[9];
    const bool ok = plane_map_of_board(b, win, M);
    for (int k = 0; k < 9; k++) maps[(size_t)f * 9 + k] = ok ? M[k] : 0.0;
    valid[f] = ok ? 1 : 0;
}

void launch_plane_warp(hipStream_t s, const PlaneWarp& args, int cn, bool dist, int nframes) {
    auto kernel = cn == 3 ? (dist ? plane_warp_kernel<true, 3> : plane_warp_kernel<false, 3>) : (dist ? plane_warp_kernel<true, 1> : plane_warp_kernel<false, 1>);
    const dim3 tiles((args.out_width + PW_TILE_W - 1) / PW_TILE_W, (args.out_height + PW_TILE_H - 1) / PW_TILE_H);
    for (int f0 = 0; f0 < nframes; f0 += 65535) {   // the grid's z limit
        PlaneWarp a = args;
        a.src += (size_t)f0 * a.frame_stride, a.dst += (size_t)f0 * a.dst_frame_stride, a.maps += (size_t)f0 * 9;
        if (a.valid) a.valid += f0;
        hipLaunchKernelGGL(kernel, dim3(tiles.x, tiles.y, std::min(65535, nframes - f0)), dim3(256), 0, s, a);
    }
}

void launch_plane_maps(hipStream_t s, const arucohip_board_t* boards, int nframes, const arucohip_rectify_t& win, double* maps, int32_t* valid) {
    hipLaunchKernelGGL(plane_maps_kernel, dim3((nframes + 63) / 64), dim3(64), 0, s, boards, nframes, win, maps, valid);
}

}  // namespace ah
